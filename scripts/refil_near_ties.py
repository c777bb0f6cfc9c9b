#!/usr/bin/env python
"""CPU only: the near-tie share of the float64 oracle alone for the REFIL rollout shape cases (tests/refil_shapes.py).

For every case the plan, seed and weights of the GPU test are rolled out with the oracle entity env
(oracle/env_ref.c, envref.RefEntityEnv) and the float64 oracle agent (oracle/refil_ref.py entity_agent, one step at a
time with the hidden state carried): the test-mode run of episode 0 (greedy) and the train-mode run of episode 1
(epsilon 0.525, draws from the counter RNG, as the kernels make them). Counted: the decisions (greedy picks with at
least two available actions), and those whose top-two masked Q lie within Q_TOL = 1e-4 -- the picks the GPU checker
would accept as near ties. A case's seed is kept only if that share is at most 0.5 % (the GPU tests cap the accepted
share at 1 %).

    python scripts/refil_near_ties.py [case id ...] [--seed S]
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
import refil_ref as RR  # noqa: E402
import refil_shapes as FS  # noqa: E402
from helpers import Q_TOL, ref_entity_envs_for, refil_args  # noqa: E402


def near_ties(cid, seed):
    """(decisions, near ties among them, all greedy picks, epsilon draws) of the oracle over both runs of a case."""
    spec = FS.spec_for(cid, seed)
    NA, U, A, B = spec.n_agents, spec.U, spec.n_actions, FS.B
    args = refil_args(n_agents=NA, n_entities=U, n_actions=A, device="cpu")
    p = {k: torch.from_numpy(v).double() for k, v in FS.entity_agent_params(8 + A, A, seed).items()}
    decisions = ties = picks = draws = 0
    for episode, eps in ((0, 0.0), (1, FS.EPS)):
        refs = ref_entity_envs_for(spec, B, seed=seed)
        for r in refs:
            r.episode = episode
            r.reset()
        h = torch.zeros(B, NA, 64, dtype=torch.float64)
        last = np.zeros((B, U, A))
        status = [0] * B  # 0 running, 1 terminated (one more pick is recorded), 2 finished
        t = 0
        while any(s < 2 for s in status):
            obs = [r.entities() for r in refs]
            ent = np.concatenate([np.stack([o[0] for o in obs]).astype(np.float64), last], axis=2)
            om, em = np.stack([o[1] for o in obs]), np.stack([o[2] for o in obs])
            avail = np.stack([r.avail() for r in refs])
            with torch.no_grad():
                q, hs = RR.entity_agent(p, torch.from_numpy(ent)[:, None], torch.from_numpy(om)[:, None],
                                        torch.from_numpy(em)[:, None], h, args)
            h = hs[:, 0]
            q = q[:, 0].numpy()
            acts = np.zeros((B, NA), np.int64)
            for b in range(B):
                if status[b] == 2:
                    continue
                key = envref.env_key(seed, b)
                for n in range(NA):
                    av = avail[b, n]
                    if eps > 0 and envref.u01(envref.rng(key, envref.ctr(episode, t, 2, n))) < np.float32(eps):
                        r2 = envref.rng(key, envref.ctr(episode, t, 3, n))
                        acts[b, n] = envref.random_available(av.tolist(), r2)
                        draws += 1
                        continue
                    m = np.where(av == 0, -np.inf, q[b, n])
                    srt = np.sort(m)
                    picks += 1
                    if np.isfinite(srt[-2]):
                        decisions += 1
                        ties += int(not srt[-1] - srt[-2] > Q_TOL)
                    acts[b, n] = int(np.argmax(m))
            last[:] = 0
            np.put_along_axis(last[:, :NA], acts[:, :, None], 1.0, axis=2)
            for b, r in enumerate(refs):
                if status[b] == 0:
                    _, done, _ = r.step(acts[b])
                    status[b] = 1 if done else 0
                elif status[b] == 1:
                    status[b] = 2
            t += 1
    return decisions, ties, picks, draws


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", help="case ids (default: all)")
    ap.add_argument("--seed", type=int, default=None, help="try this seed instead of the case's own")
    a = ap.parse_args()
    done = {}
    for cid, codes, kmin, kmax, env, arm, seed in FS.REFIL_CASES:
        if a.cases and cid not in a.cases:
            continue
        seed = seed if a.seed is None else a.seed
        key = (codes, kmin, kmax, seed)  # the arm does not enter the oracle's rollout
        if key not in done:
            done[key] = near_ties(cid, seed)
        dec, ties, picks, draws = done[key]
        share = 100.0 * ties / dec
        print(f"{cid:14s} S={len(codes.split())} k {kmin}..{kmax} {arm:10s} seed {seed}: {ties} near ties of {dec} "
              f"decisions = {share:.3f} % ({picks} greedy picks, {draws} epsilon draws)"
              f"{'' if share <= 0.5 else '   > 0.5 %: REJECT'}", flush=True)


if __name__ == "__main__":
    main()
