"""Generate the average-proportional-loss golden fixture (tests/golden/jpc.npz) from the reference's own
src/eval/methods.py (avg_proportional_loss, :8-18).

TEST INFRASTRUCTURE ONLY. Loads the reference's eval/methods.py as a standalone module at run time (it needs torch
and numpy only) and records DATA: a few joint-policy-correlation matrices and, per matrix, what the reference returns
for it (or the flag that it raised NotImplementedError: a negative diagonal mean). No reference source text.

Cases: a plain 2x2, a 3x3, an off-diagonal-greater matrix (negative loss; the reference prints a note), a 4x4 with
negative entries but a positive diagonal mean, and a negative-diagonal matrix (raises).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jpc_golden.py <reference checkout>
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpc.npz")


def load_reference(ref_root):
    path = os.path.join(ref_root, "src", "eval", "methods.py")
    spec = importlib.util.spec_from_file_location("ref_eval_methods", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref_root):
    ref = load_reference(ref_root)
    rng = np.random.RandomState(7)
    cases = [
        np.array([[30.0, 12.0], [10.0, 26.0]], dtype=np.float32),
        (rng.rand(3, 3) * 20 + np.eye(3) * 25).astype(np.float32),
        np.array([[5.0, 9.0, 8.0], [7.5, 4.0, 9.5], [8.0, 10.0, 6.0]], dtype=np.float32),  # off-diagonal greater
        (rng.randn(4, 4) * 6 + np.eye(4) * 12).astype(np.float32),
        np.array([[-3.0, 2.0], [1.0, -5.0]], dtype=np.float32),  # negative diagonal mean
    ]
    out = {"n": np.int64(len(cases))}
    for k, m in enumerate(cases):
        out[f"jpc_{k}"] = m
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                v = ref.avg_proportional_loss(torch.from_numpy(m.copy()))
            out[f"apl_{k}"] = np.float32(float(v))
            out[f"raises_{k}"] = np.bool_(False)
        except NotImplementedError:
            out[f"apl_{k}"] = np.float32(np.nan)
            out[f"raises_{k}"] = np.bool_(True)
    np.savez(OUT, **out)
    print(f"wrote {OUT}: " + ", ".join(f"{float(out[f'apl_{k}']):.6f}" for k in range(len(cases))))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
