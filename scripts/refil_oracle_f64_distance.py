"""How far is the fp32 CPU oracle of the REFIL learner (oracle/refil_ref.py, tests/refil_baseline_ref.py) from a
float64 run of itself, on the cases of tests/refil_learner_shapes.py? Runs on the CPU.

Prints, per case, the rows of that module's two tables. ORACLE_F64: the largest distance of a statistic over the three
calls (as the rtol at which the statistics' rtol / atol pair, scaled together, would just hold), the largest absolute
distance of a parameter (online or target) after them, the float64 oracle's smallest top-two gap of the masked online
Q over the three calls (a seed is kept at >= 1e-4) and its first-call grad_norm (> 20 for the -clip cases, < 5
elsewhere). GRAD_D32: per tensor, in flat parameter order, max|g32 - g64| of the first call's gradients before the
clip. With ``-v`` also each tensor's max|g64| and d32 / max|g64|.

With case ids as arguments: those cases only. With ``seeds=1,2,3`` as an argument: the gap and grad_norm columns for
those seeds instead of the case's own (to choose a seed)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ma-league_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np
import torch

import refil_learner_shapes as RS


def params_of(ref):
    out = {}
    for tag, d in (("agent.", ref.agent), ("mixer.", ref.mixer), ("t_agent.", ref.t_agent), ("t_mixer.", ref.t_mixer)):
        out.update({tag + k: v.detach().double().numpy() for k, v in d.items()})
    return out


def distance(c):
    s32, r32, g32, _ = RS.run_oracle(c, torch.float32)
    s64, r64, g64, gap = RS.run_oracle(c, torch.float64)
    floor = RS.STAT_ATOL / RS.STAT_RTOL
    ds = max(abs(a[k] - b[k]) / (floor + abs(b[k])) for a, b in zip(s32, s64) for k in b)
    p32, p64 = params_of(r32), params_of(r64)
    dp = max(float(np.abs(p32[k] - p64[k]).max()) for k in p64)
    dg = [float((a.double() - b).abs().max()) for a, b in zip(g32, g64)]
    return ds, dp, dg, [float(g.abs().max()) for g in g64], gap, s64[0]["grad_norm"]


def main(argv):
    verbose = "-v" in argv
    seeds = next((a[6:].split(",") for a in argv if a.startswith("seeds=")), None)
    ids = [a for a in argv if a in RS.IDS] or RS.IDS
    if seeds:
        for cid in ids:
            for s in seeds:
                c = RS.case(cid)._replace(seed=int(s))
                st, _, _, gap = RS.run_oracle(c, torch.float64)
                print(f"{cid} seed {s}: gap {gap:.2e}, grad_norm {st[0]['grad_norm']:.4g}", flush=True)
        return
    rows = []
    for cid in ids:
        ds, dp, dg, mg, gap, gn = distance(RS.case(cid))
        print(f'    "{cid}": ({ds:.2e}, {dp:.2e}, {gap:.2e}, {gn:.4g}),'
              f'  # largest d32 / max|g64| {max(d / m for d, m in zip(dg, mg) if m > 0):.1e}', flush=True)
        rows.append(f'    "{cid}": (' + ", ".join(f"{d:.2e}" for d in dg) + "),")
        if verbose:
            for i, (d, m) in enumerate(zip(dg, mg)):
                print(f"        tensor {i}: max|g64| {m:.3e}, d32 {d:.2e}, ratio {d / max(m, 1e-300):.1e}")
    print("GRAD_D32")
    print("\n".join(rows))


if __name__ == "__main__":
    main(sys.argv[1:])
