"""Seeds of the sampling cases of tests/per_shapes.py. Runs on the CPU, the float64 oracle (tests/per_ref.py) alone.

Per case: the first seed from the case's base (per_shapes.sample_base_seed) at which no draw lies within
per_cases.NEAR_TIE (1e-9 of the total) of a cumulative boundary, so that the device's fp64 scan, which adds in another
order, must pick the same slot for every draw. Prints the rows of per_shapes.SAMPLE_SEEDS with the margin found and the
seeds tried."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ma-league_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import per_cases as PC
import per_ref as PR
import per_shapes as PS

if __name__ == "__main__":
    for sid in PS.SAMPLE_IDS:
        base = PS.sample_base_seed(sid)
        for seed in range(base, base + 64):
            p, n, B, _, draw, beta = PS.sample_case(sid, seed=seed)
            margin = PR.sample(p, n, B, seed, draw, beta)[2]
            if margin > PC.NEAR_TIE:
                print(f'    "{sid}": {seed},  # margin {margin:.2e}, {seed - base + 1} tried')
                break
        else:
            sys.exit(f"{sid}: no seed in {base} .. {base + 63}")
