#!/usr/bin/env python
"""CPU only: the near-tie share of the float64 oracle alone for the rollout shape cases (tests/rollout_shapes.py).

For every case the plan, seed and weights of the GPU test are rolled out with the oracle env (oracle/env_ref.c) and
the float64 oracle DRQN (oracle/learner_ref.py): the test-mode run of episode 0 (greedy) and the train-mode run of
episode 1 (epsilon draws from the counter RNG, as the kernels make them). Counted: the greedy picks, and those whose
top-two masked Q lie within Q_TOL = 1e-4 -- the picks the GPU checkers would accept as near ties. A case's seed is
kept only if that share is at most 0.5 % (the GPU tests cap the accepted share at 1 %).

    python scripts/rollout_near_ties.py [case id ...] [--seed S]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ma-league_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import envref  # noqa: E402
import learner_ref as LR  # noqa: E402
import rollout_shapes as RS  # noqa: E402
from helpers import Q_TOL, ref_envs_for, shape_plan  # noqa: E402


def near_ties(plan, hidden, seed, self_play):
    """(greedy picks, near ties among them, epsilon draws) of the oracle over both runs of a case."""
    from maleague.envs.teams_env import TeamsEnvSpec
    spec = TeamsEnvSpec.from_env_args({"match_build_plan": shape_plan(plan, self_play), "grid_size": 20,
                                       "stochastic_spawns": True, "episode_limit": RS.EPISODE_LIMIT, "seed": seed})
    sides = 2 if self_play else 1
    N, A, B = spec.n_agents // sides, spec.n_actions, RS.B
    d_in = 8 * spec.U + A + N
    params = [{k: torch.from_numpy(v).double() for k, v in RS.agent_params(d_in, hidden, A, s).items()}
              for s in RS.side_seeds(seed, self_play)]
    eye = torch.eye(N, dtype=torch.float64).repeat(B, 1)
    picks = ties = draws = 0
    for episode, eps in ((0, (0.0, 0.0)), (1, (RS.EPS_HOME, RS.EPS_AWAY if self_play else RS.EPS_HOME))):
        refs = ref_envs_for(spec, B, seed=seed)
        for r in refs:
            r.episode = episode
            r.reset()
        h = [torch.zeros(B * N, hidden, dtype=torch.float64) for _ in range(sides)]
        last = np.zeros((B, sides * N, A))
        status = [0] * B  # 0 running, 1 terminated (one more pick is recorded), 2 finished
        t = 0
        while any(s < 2 for s in status):
            obs = np.stack([r.obs() for r in refs]).astype(np.float64)
            avail = np.stack([r.avail() for r in refs])
            acts = np.zeros((B, sides * N), np.int64)
            for s in range(sides):
                sl = slice(s * N, (s + 1) * N)
                x = torch.cat([torch.from_numpy(obs[:, sl].reshape(B * N, -1)),
                               torch.from_numpy(last[:, sl].reshape(B * N, A)), eye], dim=1)
                with torch.no_grad():
                    q, h[s] = LR.drqn_forward(params[s], x, h[s])
                q = q.numpy().reshape(B, N, A)
                for b in range(B):
                    if status[b] == 2:
                        continue
                    key = envref.env_key(seed, b)
                    for n in range(N):
                        av = avail[b, s * N + n]
                        if eps[s] > 0 and envref.u01(envref.rng(key, envref.ctr(episode, t, 2, s * N + n))) \
                                < np.float32(eps[s]):
                            r2 = envref.rng(key, envref.ctr(episode, t, 3, s * N + n))
                            acts[b, s * N + n] = envref.random_available(av.tolist(), r2)
                            draws += 1
                            continue
                        m = np.where(av == 0, -np.inf, q[b, n])
                        srt = np.sort(m)
                        picks += 1
                        ties += int(not srt[-1] - srt[-2] > Q_TOL)
                        acts[b, s * N + n] = int(np.argmax(m))
            last[:] = 0
            np.put_along_axis(last, acts[:, :, None], 1.0, axis=2)
            for b, r in enumerate(refs):
                if status[b] == 0:
                    _, done, _ = r.step(acts[b])
                    status[b] = 1 if done else 0
                elif status[b] == 1:
                    status[b] = 2
            t += 1
    return picks, ties, draws


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", help="case ids (default: all)")
    ap.add_argument("--seed", type=int, default=None, help="try this seed instead of the case's own")
    a = ap.parse_args()
    for cases, sp in ((RS.ROLLOUT_CASES, False), (RS.SELFPLAY_CASES, True)):
        for cid, hidden, plan, arm, seed in cases:
            if a.cases and cid not in a.cases:
                continue
            seed = seed if a.seed is None else a.seed
            picks, ties, draws = near_ties(plan, hidden, seed, sp)
            share = 100.0 * ties / picks
            print(f"{cid:18s} H={hidden:<3d} {plan:13s} {arm:15s} seed {seed}: {ties} near ties of {picks} greedy "
                  f"picks = {share:.3f} % ({draws} epsilon draws){'' if share <= 0.5 else '   > 0.5 %: REJECT'}")


if __name__ == "__main__":
    main()
