"""How far is the fp32 CPU oracle (oracle/learner_ref.py) from a float64 run of itself? Runs on the CPU.

Without arguments: the cases of tests/test_gpu_learner_shapes.py. Prints, per case, the largest relative distance of a
statistic over the case's calls and the largest absolute distance of a parameter after the last call: the figures
behind that file's ORACLE_F64 table (a bound there is ten times the distance, where that exceeds the usual bound).

With ``arms``: the cases of tests/learner_arm_shapes.py (tests/test_gpu_learner_arms.py), three calls each. Prints
rows for that file's ORACLE_F64 table: the two figures above, the largest distance of a first-call gradient tensor
before the clip relative to max(1, max|g|) of that tensor, and the first call's grad_norm."""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ma-league_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

import learner_ref as LR
import test_gpu_learner_shapes as TS
from helpers import qmix_args


def run(agent0, mixer0, args, batch, calls, dtype):
    ref = LR.QLearnerRef(agent0, mixer0, copy.copy(args), dtype=dtype)
    stats, grads = [], None
    for t_env, ep in calls:
        stats.append(ref.train({k: v.clone() for k, v in batch.items()}, t_env, ep))
        if grads is None:
            grads = [g.double().numpy() for g in ref.last_grads]
    params = dict(ref.agent_state())
    params.update({"t." + k: v for k, v in ref.tp.items()})
    if ref.mp is not None:
        params.update({"m." + k: v for k, v in ref.mixer_state().items()})
        params.update({"tm." + k: v for k, v in ref.tmp.items()})
    return stats, {k: v.detach().double().numpy() for k, v in params.items()}, grads


def distance(agent0, mixer0, args, batch, calls):
    s32, p32, g32 = run(agent0, mixer0, args, batch, calls, torch.float32)
    s64, p64, g64 = run(agent0, mixer0, args, batch, calls, torch.float64)
    ds = max(abs(a[k] - b[k]) / max(abs(b[k]), 1e-12) for a, b in zip(s32, s64) for k in TS.STAT_KEYS)
    dp = max(float(np.abs(p32[k] - p64[k]).max()) for k in p64)
    dg = max(float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max())) for a, b in zip(g32, g64))
    return ds, dp, dg, s64


def shapes_cases():
    d = np.load(os.path.join(ROOT, "tests", "golden", "qlearner_qmix_dq.npz"))
    tb = LR.batch_from_npz(d)

    def show(name, *a):
        ds, dp, _, s64 = distance(*a)
        print(f'    "{name}": ({ds:.2e}, {dp:.2e}),  # largest grad_norm {max(s["grad_norm"] for s in s64):.4g}')

    for case, kw in TS.TRAJ.items():
        args = qmix_args(device="cpu", **kw)
        show(case, TS._golden_agent(d), TS.mixer_state(args) if args.mixer == "qmix" else None, args, tb, TS.CALLS)
    wide = TS.wide_oracle_batch(TS.wide_batch())
    for case, kw in TS.WIDE_CASES.items():
        args = qmix_args(device="cpu", **kw)
        show("wide-" + case, TS.agent_state(args, wide["obs"].shape[-1]),
             TS.mixer_state(args) if args.mixer == "qmix" else None, args, wide, [(0, 0)])


def arm_cases():
    import learner_arm_shapes as LA
    for c in LA.CASES:
        args = LA.case_args(c, "cpu")
        agent0, mixer0 = LA.case_weights(c, args)
        ds, dp, dg, s64 = distance(agent0, mixer0, args, LA.oracle_batch(LA.case_batch(c)), LA.CALLS)
        print(f'    "{c.id}": ({ds:.2e}, {dp:.2e}, {dg:.2e}, {s64[0]["grad_norm"]:.4g}),')


if __name__ == "__main__":
    arm_cases() if sys.argv[1:] == ["arms"] else shapes_cases()
