#!/usr/bin/env python
"""CPU only: what the float64 oracle alone sees on the eventful rollout cases (tests/rollout_event_shapes.py).

scripts/rollout_near_ties.py generalised to every rollout family (DRQN, feed-forward, distinct, each against the
scripted AI and in self-play, and the COMA policy) and to the events of a run. For every case the plan, seed and
weights of the GPU test are rolled out with the oracle env (oracle/env_ref.c) and the float64 oracle agent: the
test-mode run of episode 0 and the train-mode run of episode 1 at the case's epsilons. Printed per case: the greedy
picks and the near ties among them (top-two masked Q within Q_TOL = 1e-4), the envs ending before the limit, the ragged
16-env workgroups (one env ends at least 2 steps before another), the wins per side, the draws and the unit deaths, and
the conditions of the case table the counts violate (none for a kept case).

    python scripts/rollout_event_counts.py [case id ...] [--seed S] [--grid G] [--limit L] [-j JOBS]
"""
import argparse
import os
import sys
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ma-league_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import rollout_event_shapes as ES  # noqa: E402


def count(c):
    import torch
    torch.set_num_threads(1)
    n = ES.oracle_counts(c)
    bad = ES.conditions(c, n)
    if c == ES.case(c.id) and {k: n[k] for k in ES.ORACLE_KEYS} != c.oracle:
        bad.append(f"the table says {c.oracle}")
    return ES.count_line(c, n) + ("" if not bad else "   REJECT: " + "; ".join(bad))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", help="case ids (default: all)")
    ap.add_argument("--seed", type=int, default=None, help="try this seed instead of the case's own")
    ap.add_argument("--grid", type=int, default=None, help="try this grid_size")
    ap.add_argument("--limit", type=int, default=None, help="try this episode_limit")
    ap.add_argument("-j", type=int, default=1, help="worker processes")
    a = ap.parse_args()
    cases = [c for c in ES.CASES if not a.cases or c.id in a.cases]
    over = {k: v for k, v in (("seed", a.seed), ("grid", a.grid), ("limit", a.limit)) if v is not None}
    cases = [c._replace(**over) for c in cases]
    if a.j > 1:
        with ProcessPoolExecutor(a.j) as pool:
            for line in pool.map(count, cases):
                print(line, flush=True)
    else:
        for c in cases:
            print(count(c), flush=True)


if __name__ == "__main__":
    main()
