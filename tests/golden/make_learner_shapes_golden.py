"""Golden vectors of the reference QLearner for the mixer shapes beyond the default one (run where the reference
checkout that make_golden.py names is present):

  qlearner_qmix_h1.npz         hypernet_layers 1 (the reference QMixer's fallback, qmix.py:17), mixing_embed_dim 32
  qlearner_qmix_e64_he128.npz  hypernet_layers 2, mixing_embed_dim 64, hypernet_embed 128

Both reuse make_golden.qlearner_fixture unchanged (same batch, agent seed and three calls as qlearner_qmix_dq.npz),
in its non-"full" form: initial parameters, the statistics of every call, the parameters after the last call.

There is no IQL golden: with `mixer: None` the reference's QLearner.parameters() returns [] (the precedence slip at
q_learner.py:30-32) and torch.optim.RMSprop refuses an empty parameter list, so the reference cannot train IQL at
all. IQL is checked against oracle/learner_ref.py only (tests/test_gpu_learner_shapes.py).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as G  # noqa: E402

if __name__ == "__main__":
    G.qlearner_fixture("qmix_h1", False, hypernet_layers=1)
    G.qlearner_fixture("qmix_e64_he128", False, mixing_embed_dim=64, hypernet_embed=128)
    print("golden fixtures written to", G.OUT)
