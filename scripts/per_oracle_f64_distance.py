"""How far is the fp32 weighted learner oracle (tests/per_ref.py) from a float64 run of itself? Runs on the CPU.

For the cases of tests/per_shapes.py that have no figure in learner_arm_shapes.ORACLE_F64 -- the feed-forward and the
distinct-network arm tables with per = 1 and the long cases of the per-episode reduce -- the first call of the weighted
oracle in fp32 against the same call in float64. Prints the rows of per_shapes.ORACLE_F64: the largest relative
distance of a statistic left after the absolute allowance STAT_ATOL, the largest distance of a gradient tensor before the
clip relative to max(1, max|g|) of the float64 tensor, the largest distance of td_abs relative to max(1, max|td_abs|);
then the float64 grad_norm. With ``all``: every arm and reduce case."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ma-league_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import torch

import learner_arm_shapes as LA
import per_shapes as PS

STATS = ("loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean")


def distance(kind, args, agent0, mixer0, tb, w):
    g32, t32, s32 = PS.oracle_first_call(kind, args, agent0, mixer0, tb, w, torch.float32)
    g64, t64, s64 = PS.oracle_first_call(kind, args, agent0, mixer0, tb, w, torch.float64)
    ds = max(max(0.0, abs(s32[k] - s64[k]) - LA.STAT_ATOL) / max(abs(s64[k]), 1e-12) for k in STATS)
    dg = max(float((a.double() - b).abs().max()) / max(1.0, float(b.abs().max())) for a, b in zip(g32, g64))
    dt = float((t32.double() - t64).abs().max()) / max(1.0, float(t64.abs().max()))
    return ds, dg, dt, s64["grad_norm"]


if __name__ == "__main__":
    every = sys.argv[1:] == ["all"]
    for aid in PS.ARM_IDS:
        if every or not aid.startswith("rnn:"):
            kind, _, args, agent0, mixer0, tb = PS.arm_inputs(aid)
            ds, dg, dt, norm = distance(kind, args, agent0, mixer0, tb, PS.arm_weight(aid))
            print(f'    "{aid}": ({ds:.2e}, {dg:.2e}, {dt:.2e}),  # grad_norm {norm:.4g}')
    for rid in PS.REDUCE_IDS:
        if every or rid.split("-")[0] in PS.REDUCE_LONG:
            _, _, _, args, agent0, mixer0, _, tb = PS.reduce_inputs(rid)
            ds, dg, dt, norm = distance("rnn", args, agent0, mixer0, tb, PS.reduce_weight(rid))
            print(f'    "{rid}": ({ds:.2e}, {dg:.2e}, {dt:.2e}),  # grad_norm {norm:.4g}')
