"""How far is the fp32 CPU oracle (oracle/learner_ref.py) from a float64 run of itself on the cases of
tests/test_gpu_learner_shapes.py? Runs on the CPU. Prints, per case, the largest relative distance of a statistic
over the case's calls and the largest absolute distance of a parameter after the last call: the figures behind that
file's ORACLE_F64 table (a bound there is ten times the distance, where that exceeds the usual bound)."""
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
    torch.set_default_dtype(dtype)
    try:
        ref = LR.QLearnerRef(agent0, mixer0, copy.copy(args))
        if dtype == torch.float64:  # the oracle builds fp32 leaves: rebuild them, and its optimizer, in float64
            ref.p = {k: v.detach().double().requires_grad_(True) for k, v in ref.p.items()}
            ref.tp = {k: v.detach().clone() for k, v in ref.p.items()}
            if ref.mp is not None:
                ref.mp = {k: v.detach().double().requires_grad_(True) for k, v in ref.mp.items()}
                ref.tmp = {k: v.detach().clone() for k, v in ref.mp.items()}
            ref.params = list(ref.p.values()) + (list(ref.mp.values()) if ref.mp is not None else [])
            ref.opt = torch.optim.RMSprop(ref.params, lr=args.lr, alpha=args.optim_alpha, eps=args.optim_eps)
        stats = []
        for t_env, ep in calls:
            b = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in batch.items()}
            stats.append(ref.train(b, t_env, ep))
        params = dict(ref.agent_state())
        params.update({"t." + k: v for k, v in ref.tp.items()})
        if ref.mp is not None:
            params.update({"m." + k: v for k, v in ref.mixer_state().items()})
            params.update({"tm." + k: v for k, v in ref.tmp.items()})
        return stats, {k: v.detach().double().numpy() for k, v in params.items()}
    finally:
        torch.set_default_dtype(torch.float32)


def distance(name, agent0, mixer0, args, batch, calls):
    s32, p32 = run(agent0, mixer0, args, batch, calls, torch.float32)
    s64, p64 = run(agent0, mixer0, args, batch, calls, torch.float64)
    ds = max(abs(a[k] - b[k]) / max(abs(b[k]), 1e-12) for a, b in zip(s32, s64) for k in TS.STAT_KEYS)
    dp = max(float(np.abs(p32[k] - p64[k]).max()) for k in p64)
    gn = max(b["grad_norm"] for b in s64)
    print(f'    "{name}": ({ds:.2e}, {dp:.2e}),  # largest grad_norm {gn:.4g}')


if __name__ == "__main__":
    d = np.load(os.path.join(ROOT, "tests", "golden", "qlearner_qmix_dq.npz"))
    tb = LR.batch_from_npz(d)
    for case, kw in TS.TRAJ.items():
        args = qmix_args(device="cpu", **kw)
        distance(case, TS._golden_agent(d), TS.mixer_state(args) if args.mixer == "qmix" else None, args, tb, TS.CALLS)
    wide = TS.wide_oracle_batch(TS.wide_batch())
    for case, kw in TS.WIDE_CASES.items():
        args = qmix_args(device="cpu", **kw)
        distance("wide-" + case, TS.agent_state(args, wide["obs"].shape[-1]),
                 TS.mixer_state(args) if args.mixer == "qmix" else None, args, wide, [(0, 0)])
