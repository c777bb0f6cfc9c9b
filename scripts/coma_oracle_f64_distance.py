#!/usr/bin/env python
"""CPU only: how far is an fp32 run of the COMA restatement (tests/coma_ref.py with dtype=float32, numpy's summation
order) from its float64 run, on the critic cases and the learner case of tests/coma_shapes.py?

Prints, per critic case, the largest |fp32 - float64| per quantity over the two calls (q_vals, TD(lambda) targets, the
five stat means, the parameters), the largest magnitude of each quantity, the steps taken and the range of the
gradient norms; for the learner case the same over three calls on the batch the float64 oracle alone rolls out (with
the actor stats and the agent parameters). These floors stand beside the cases in tests/coma_shapes.py; the GPU
tolerances are 4x them.

    python scripts/coma_oracle_f64_distance.py [case id ...] [--ascending]      (the learner case: learner)

--ascending also prints, per critic case, the distance of an fp32 run whose matrix products add their terms one at a
time in ascending order, as the kernels do (coma_ref.mm_ascending: fused multiply-adds in the layers, 32 inputs
per chain and then the chains, as coma.hip's dense16; the product rounded first in the gradient sums); numpy adds them in blocks and lands closer to float64. This figure is not a floor: it says how much of the 4x margin the order of summation alone takes.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ma-league_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import coma_shapes as CS  # noqa: E402


def fmt(d):
    return ", ".join(f"{k} {v:.2e}" for k, v in d.items())


def main(argv):
    named = [a for a in argv if not a.startswith("--")]
    ids = [a for a in named if a in CS.CRITIC_IDS] or ([] if named else CS.CRITIC_IDS)
    for cid in ids:
        c = CS.critic_case(cid)
        r64, r32 = CS.run_critic_ref(c, np.float64), CS.run_critic_ref(c, np.float32)
        d = CS.distance(r32, r64, CS.CRITIC_KEYS)
        mag = {k: max(float(np.abs(r[k]).max()) for r in r64) for k in CS.CRITIC_KEYS}
        norms = [n for r in r64 for n in r["norms"]]
        print(f"{cid:7s} floors: {fmt(d)}\n        max |.|: {fmt(mag)}; steps {[r['taken'] for r in r64]}, grad norms "
              f"{min(norms):.3g}..{max(norms):.3g}, blocks {CS.critic_blocks(c)}", flush=True)
        print(f"        ({', '.join(f'{d[k]:.2e}' for k in CS.CRITIC_KEYS)})", flush=True)
        if "--ascending" in argv:
            da = CS.distance(CS.run_critic_ref(c, np.float32, ascending=True), r64, CS.CRITIC_KEYS)
            print(f"        fp32 in the kernels' order of summation: {fmt(da)}", flush=True)
    if not named or "learner" in named:
        spec, batch, ep_len = CS.learner_oracle_batch()
        r64, r32 = CS.run_learner_ref(batch, spec, np.float64), CS.run_learner_ref(batch, spec, np.float32)
        d = CS.distance(r32, r64, CS.LEARNER_KEYS)
        mag = {k: max(float(np.abs(r[k]).max()) for r in r64) for k in CS.LEARNER_KEYS}
        print(f"learner ({CS.LEARNER_CASE.id}, episode lengths {ep_len.tolist()} of {CS.LEARNER_LIMIT}) floors: {fmt(d)}\n"
              f"        max |.|: {fmt(mag)}", flush=True)
        print(f"        ({', '.join(f'{d[k]:.2e}' for k in CS.LEARNER_KEYS)})", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
