#!/usr/bin/env python
"""CPU only: the float64 oracle's own self-play over the REFIL self-play cases (tests/refil_selfplay_shapes.py).

For every case both sides are played by the float64 oracle agent (oracle/refil_ref.py entity_agent, hidden state
carried per side) over the oracle two-policy entity env (tests/refil_selfplay_ref.py), the away side through the
canonical view: the test-mode run of episode 0 and the train-mode run of episode 1 (eps_home 0.525, eps_away 0.3, draws
from the counter RNG by global agent index, as the kernel makes them). Counted per side: the decisions (greedy picks
with at least two available actions) and those whose top-two masked Q lie within Q_TOL = 1e-4. A case's seeds are kept
only if the share is at most 0.5 % on both sides (the GPU tests cap the accepted share at 1 %). Also printed: what the
play did -- away wins, away move and target actions, the k values seen -- the GPU test asserts the same of the kernel's
runs.

    python scripts/refil_selfplay_near_ties.py [case id ...] [--seed-away S]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ma-league_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import refil_selfplay_ref as SR  # noqa: E402
import refil_selfplay_shapes as SS  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", help="case ids (default: all)")
    ap.add_argument("--seed-away", type=int, default=None, help="try this away weight seed instead of the case's own")
    a = ap.parse_args()
    for c in SS.SP_CASES:
        if a.cases and c.id not in a.cases:
            continue
        if a.seed_away is not None:
            c = c._replace(seed_away=a.seed_away)
        spec = SS.spec_for(c)
        n, out = SR.oracle_selfplay(spec, SR.case_params(c), c.la, SS.B, c.seed, SS.RUNS)
        shares = []
        for side in SR.SIDES:
            d = n[side]
            shares.append(100.0 * d["near_ties"] / d["decisions"])
            print(f"{c.id:8s} {side}: {d['near_ties']} near ties of {d['decisions']} decisions = {shares[-1]:.3f} % "
                  f"({d['greedy']} greedy picks, {d['epsilon_draws']} epsilon draws)")
        print(f"{c.id:8s} play: away wins {out['away_wins']}, home wins {out['home_wins']}, away moves "
              f"{out['away_moves']}, away targets {out['away_targets']}, env steps {out['steps']}, k seen "
              f"{sorted(out['ks'])}{'' if max(shares) <= 0.5 else '   > 0.5 %: REJECT'}", flush=True)


if __name__ == "__main__":
    main()
