#!/usr/bin/env python
"""CPU only: the near-tie share of the float64 oracle alone for the distinct-network self-play rollout cases
(tests/distinct_selfplay_shapes.py).

For every case the plan, seed and both sides' per-agent weights of the GPU test are rolled out with the oracle env
(oracle/env_ref.c, both teams policy-controlled) and the float64 per-agent oracle (tests/distinct_ref.py): the
test-mode run of episode 0 (greedy) and the train-mode run of episode 1 (epsilon draws from the counter RNG as the
kernel makes them: one epsilon per side, the global agent index s * nh + ln as the stream index). Counted: the greedy
picks of both sides, and those whose top-two masked Q lie within Q_TOL = 1e-4 -- the picks the GPU checker would accept
as near ties. A case's (seed, fc2_scale) is kept only if that share is at most 0.5 % (the GPU tests cap the accepted
share at 1 %).

    python scripts/distinct_selfplay_near_ties.py [case id ...] [--seed S] [--fc2-scale X]
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
import distinct_selfplay_shapes as DSP  # noqa: E402
import learner_ref as LR  # noqa: E402
from helpers import Q_TOL, ref_envs_for  # noqa: E402


def near_ties(plan, hidden, last_action, seed, fc2_scale):
    """(greedy picks, near ties among them, epsilon draws) of the oracle over both runs of a case, both sides."""
    spec = DSP.spec_of(plan, seed)
    N, A, B = spec.n_agents, spec.n_actions, DSP.B
    nh = N // 2
    d_in = 8 * spec.U + (A if last_action else 0)
    sides = DSP.side_params(nh, d_in, hidden, A, seed, fc2_scale)
    # global agent a = s * nh + ln acts with network ln of side s
    ps = [{k: torch.from_numpy(v).double() for k, v in p.items()} for side in sides for p in side]
    picks = ties = draws = 0
    for episode, eps in ((0, (0.0, 0.0)), (1, (DSP.EPS, DSP.EPS_AWAY))):
        refs = ref_envs_for(spec, B, seed=seed)
        for r in refs:
            r.episode = episode
            r.reset()
        last = np.zeros((B, N, A))
        h = [torch.zeros(B, hidden, dtype=torch.float64) for _ in range(N)]
        status = [0] * B  # 0 running, 1 terminated (one more pick is recorded), 2 finished
        t = 0
        while any(s < 2 for s in status):
            obs = torch.from_numpy(np.stack([r.obs() for r in refs]).astype(np.float64))
            avail = np.stack([r.avail() for r in refs])
            acts = np.zeros((B, N), np.int64)
            x = torch.cat([obs, torch.from_numpy(last)], dim=2) if last_action else obs
            q = np.zeros((B, N, A))
            with torch.no_grad():
                for i in range(N):
                    qi, h[i] = LR.drqn_forward(ps[i], x[:, i], h[i])
                    q[:, i] = qi.numpy()
            for b in range(B):
                if status[b] == 2:
                    continue
                key = envref.env_key(seed, b)
                for n in range(N):
                    av = avail[b, n]
                    e = eps[n >= nh]
                    if e > 0 and envref.u01(envref.rng(key, envref.ctr(episode, t, 2, n))) < np.float32(e):
                        acts[b, n] = envref.random_available(av.tolist(), envref.rng(key, envref.ctr(episode, t, 3, n)))
                        draws += 1
                        continue
                    m = np.where(av == 0, -np.inf, q[b, n])
                    srt = np.sort(m)
                    picks += 1
                    ties += int(not srt[-1] - srt[-2] > Q_TOL)
                    acts[b, n] = int(np.argmax(m))
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
    ap.add_argument("--fc2-scale", type=float, default=None, help="try this fc2 scale instead of the case's own")
    a = ap.parse_args()
    for cid, hidden, plan, la, arm, seed, scale in DSP.CASES:
        if a.cases and cid not in a.cases:
            continue
        seed = seed if a.seed is None else a.seed
        scale = scale if a.fc2_scale is None else a.fc2_scale
        picks, ties, draws = near_ties(plan, hidden, la, seed, scale)
        share = 100.0 * ties / picks
        print(f"{cid:18s} H={hidden:<3d} {plan:13s} {arm:17s} seed {seed} fc2 x{scale:g}: {ties} near ties of {picks} "
              f"greedy picks = {share:.3f} % ({draws} epsilon draws){'' if share <= 0.5 else '   > 0.5 %: REJECT'}",
              flush=True)


if __name__ == "__main__":
    main()
