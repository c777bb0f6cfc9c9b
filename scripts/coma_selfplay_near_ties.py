#!/usr/bin/env python
"""CPU only: the near-tie shares and the early-ending envs of the float64 oracle alone for the two-policy COMA rollout
cases (tests/coma_selfplay_shapes.py).

For every case and both values of mask_before_softmax, the plan, seed and weights of the GPU test are rolled out with
the oracle env (oracle/env_ref.c) and the float64 oracle policy of each side (oracle/learner_ref.py, tests/coma_ref.py)
as the greedy test-mode run of the GPU test makes it (episode 2, first-index argmax of the masked probabilities).
Counted per side: the picks, and those whose top two masked probabilities lie within DELTA = 2e-4 -- the picks the GPU
checker would accept as near ties; and the envs of 17 that end before the episode limit. A (case, mask) runs the greedy
check on the GPU only if the share is at most 1 % on each side (the GPU checker caps the accepted share at 2 %) and at
least 2 envs end early; the line says whether the case table lists it. Exit status 1 if a listed one misses.

    python scripts/coma_selfplay_near_ties.py [case id ...] [--all-modes]

--all-modes also prints the early-ending envs of the train-mode (episode 0) and draw (episode 1) runs.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ma-league_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import coma_selfplay_shapes as SP  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", help="case ids (default: all)")
    ap.add_argument("--all-modes", action="store_true")
    a = ap.parse_args()
    bad = 0
    for c in SP.CASES:
        if a.cases and c.id not in a.cases:
            continue
        for mask in (True, False):
            ep_len, picks, near = SP.oracle_run(c.plan, c.H, mask, "greedy", SP.EP_GREEDY)
            early = int((ep_len < SP.EPISODE_LIMIT).sum())
            shares = [near[s] / picks[s] for s in range(2)]
            listed = mask in c.greedy
            verdict = "runs the greedy check" if listed else "no greedy check"
            if listed and (max(shares) > SP.ORACLE_NEAR_TIE_CAP or early < SP.MIN_EARLY):
                verdict += "   > 1 % or < 2 early: REJECT"
                bad += 1
            extra = ""
            if a.all_modes:
                for mode, ep in (("train", SP.EP_TRAIN), ("draw", SP.EP_DRAW)):
                    L, _, _ = SP.oracle_run(c.plan, c.H, mask, mode, ep)
                    extra += f"   {mode}: {int((L < SP.EPISODE_LIMIT).sum())} early"
            print(f"{c.id:10s} H={c.H:<3d} A={SP.spec_of(c.plan).n_actions:<2d} mask={int(mask)}: near ties home "
                  f"{near[0]}/{picks[0]} = {100 * shares[0]:.3f} %, away {near[1]}/{picks[1]} = {100 * shares[1]:.3f} %; "
                  f"{early} of {SP.B} envs end early (lengths {int(ep_len.min())}..{int(ep_len.max())})   {verdict}{extra}",
                  flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
