"""COMA critic: fc1 -> ReLU -> fc2 -> ReLU -> fc3 over [state | obs | masked joint actions | last joint actions |
agent id] (API + state_dict keys of src/marl/modules/critics/coma.py:6-73).

The parameters are ordinary nn.Linear tensors (``critic.th`` checkpoints interoperate with the reference). The
critic runs only inside ``mlg_coma_critic_train`` (COMALearner), which builds the input rows from the batch in the
kernel: the [B, T, N, D] input tensor is never materialised, and there is no Python forward.
"""
from __future__ import annotations

import torch.nn as nn

from ... import _native

CRITIC_ORDER = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias"]
HIDDEN = 128  # critics/coma.py:18-20


class COMACritic(nn.Module):
    def __init__(self, scheme, args):
        super().__init__()
        self.args = args
        self.n_actions = args.n_actions
        self.n_agents = args.n_agents
        self.input_shape = self._get_input_shape(scheme)
        self.output_type = "q"
        dev = getattr(args, "device", "cpu")
        self.fc1 = nn.Linear(self.input_shape, HIDDEN, device=dev)
        self.fc2 = nn.Linear(HIDDEN, HIDDEN, device=dev)
        self.fc3 = nn.Linear(HIDDEN, self.n_actions, device=dev)

    def forward(self, batch, t=None):
        raise _native.NativeError("COMACritic runs inside mlg_coma_critic_train (COMALearner.train); it has no "
                                  "stand-alone forward")

    def _get_input_shape(self, scheme):
        vs = scheme["state"]["vshape"]
        state = int(vs[0] if isinstance(vs, (tuple, list)) else vs)
        vo = scheme["obs"]["vshape"]
        obs = int(vo[0] if isinstance(vo, (tuple, list)) else vo)
        return state + obs + 2 * scheme["actions_onehot"]["vshape"][0] * self.n_agents + self.n_agents
