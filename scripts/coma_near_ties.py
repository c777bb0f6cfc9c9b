#!/usr/bin/env python
"""CPU only: the near-tie share of the float64 oracle alone for the COMA policy rollout cases (tests/coma_shapes.py).

For every case and both values of mask_before_softmax, the plan, seed and weights of the GPU test are rolled out with
the oracle env (oracle/env_ref.c) and the float64 oracle policy (oracle/learner_ref.py, tests/coma_ref.py) as the
greedy test-mode run of the GPU test makes it (episode 2, first-index argmax of the masked probabilities). Counted: the
picks, and those whose top two masked probabilities lie within DELTA = 2e-4 -- the picks the GPU checker would accept
as near ties. A (case, mask) runs the greedy check on the GPU only if that share is at most 1 % (the GPU checker caps
the accepted share at 2 %); the line says whether the case table lists it.

    python scripts/coma_near_ties.py [case id ...] [--scale S] [--lengths]

--scale tries another factor on fc2.weight than the case's own; --lengths also prints the episode lengths.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ma-league_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import coma_shapes as CS  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", help="case ids (default: all)")
    ap.add_argument("--scale", type=float, default=None, help="try this fc2.weight factor instead of the case's own")
    ap.add_argument("--lengths", action="store_true")
    a = ap.parse_args()
    bad = 0
    for c in CS.POLICY_CASES:
        if a.cases and c.id not in a.cases:
            continue
        spec = CS.policy_spec(c)
        scale = c.scale if a.scale is None else a.scale
        for mask in (True, False):
            _, ep_len, picks, near = CS.oracle_policy_run(spec, c.H, c.seed, scale, mask, CS.EP_GREEDY, "greedy")
            share = near / picks
            listed = mask in c.greedy
            verdict = "runs the greedy check" if listed else "no greedy check"
            if listed and share > CS.ORACLE_NEAR_TIE_CAP:
                verdict += "   > 1 %: REJECT"
                bad += 1
            print(f"{c.id:20s} H={c.H:<3d} {c.plan:13s} A={spec.n_actions:<2d} x{scale:<4g} mask={int(mask)}: {near} near "
                  f"ties of {picks} picks = {100 * share:.3f} %   {verdict}"
                  + (f"   lengths {ep_len.tolist()}" if a.lengths else ""), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
