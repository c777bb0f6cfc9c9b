#!/usr/bin/env python
"""CPU only: the near-tie share of the float64 oracle alone for the feed-forward self-play rollout cases
(tests/dqn_selfplay_shapes.py).

For every case the plan, seed and both sides' weights of the GPU test are rolled out with the oracle env
(oracle/env_ref.c, both teams policy-controlled) and the float64 feed-forward oracle (tests/dqn_ref.py): the test-mode
run of episode 0 (greedy) and the train-mode run of episode 1 (epsilon draws from the counter RNG as the kernel makes
them: one epsilon per side, the global agent index s * nh + ln as the stream index). Counted: the greedy picks of both
sides, and those whose top-two masked Q lie within Q_TOL = 1e-4 -- the picks the GPU checker would accept as near ties.
A case's (seed, fc2_scale) is kept only if that share is at most 0.5 % (the GPU tests cap the accepted share at 1 %).
The rollout itself is dqn_selfplay_shapes.near_ties, which tests/test_dqn_selfplay.py also runs for two cases.

    python scripts/dqn_selfplay_near_ties.py [case id ...] [--seed S] [--fc2-scale X]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ma-league_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import dqn_selfplay_shapes as FSP  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", help="case ids (default: all)")
    ap.add_argument("--seed", type=int, default=None, help="try this seed instead of the case's own")
    ap.add_argument("--fc2-scale", type=float, default=None, help="try this fc2 scale instead of the case's own")
    a = ap.parse_args()
    for cid, hidden, plan, la, ai, arm, seed, scale in FSP.CASES:
        if a.cases and cid not in a.cases:
            continue
        seed = seed if a.seed is None else a.seed
        scale = scale if a.fc2_scale is None else a.fc2_scale
        picks, ties, draws = FSP.near_ties(plan, hidden, la, ai, seed, scale)
        share = 100.0 * ties / picks
        print(f"{cid:18s} H={hidden:<3d} {plan:13s} {arm:17s} seed {seed} fc2 x{scale:g}: {ties} near ties of {picks} "
              f"greedy picks = {share:.3f} % ({draws} epsilon draws){'' if share <= 0.5 else '   > 0.5 %: REJECT'}",
              flush=True)


if __name__ == "__main__":
    main()
