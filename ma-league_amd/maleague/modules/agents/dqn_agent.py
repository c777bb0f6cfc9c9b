"""Feed-forward agent: fc1 -> ReLU -> fc2 (API + state_dict keys of src/marl/modules/agents/dqn_agent.py:9-37).

Parameters are ordinary nn.Linear tensors (so ``{name}agent.th`` checkpoints interoperate with the reference); the
forward pass runs in the gfx950 kernel (mlg_ff_forward) from a packed copy of the weights that is refreshed whenever
the parameters change. The hidden state is handed back untouched: the agent has none (DESIGN.md §7 records the
reference's ``init_hidden`` defect and the shape used here).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ... import _native
from .drqn_agent import AgentNetwork


class DQNAgentNetwork(AgentNetwork):
    # named_parameters() order = the flat order of mlg_ff_backward's dparams
    PARAM_ORDER = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
    recurrent = False

    def __init__(self, input_shape, args):
        super().__init__(input_shape, args)
        dev = getattr(args, "device", "cpu")
        self.fc1 = nn.Linear(input_shape, args.rnn_hidden_dim, device=dev)
        self.fc2 = nn.Linear(args.rnn_hidden_dim, args.n_actions, device=dev)
        self._packed = None
        self._packed_key = None
        self._dirty = 0
        self._h0 = None
        self._autograd = bool(getattr(args, "native_autograd", False))

    # ---- kernel plumbing --------------------------------------------------------------------
    def dims(self) -> _native.MlgAgentDims:
        a = self.args
        return _native.MlgAgentDims(d_obs=self.input_shape - (a.n_actions if a.obs_last_action else 0)
                                    - (a.n_agents if a.obs_agent_id else 0),
                                    n_actions=a.n_actions, n_agents=a.n_agents, hidden=a.rnn_hidden_dim,
                                    d_in=self.input_shape, obs_last_action=int(bool(a.obs_last_action)),
                                    obs_agent_id=int(bool(a.obs_agent_id)))

    def mark_dirty(self):
        """Call after parameters were modified outside torch."""
        self._dirty += 1

    def packed(self) -> torch.Tensor:
        """Packed weight block (agent_ff_device.h layout); rebuilt when any parameter changed."""
        params = self._live_params()
        key = (self._dirty,) + tuple((p.data_ptr(), p._version) for p in params)
        if self._packed is None or key != self._packed_key:
            d = self.dims()
            n = _native.load().mlg_ff_packed_size(_native.byref(d))
            if n < 0:
                raise _native.NativeError(_native.load().mlg_last_error().decode())
            dev = self.fc1.weight.device
            if self._packed is None or self._packed.numel() != n or self._packed.device != dev:
                self._packed = torch.empty(n, dtype=torch.float32, device=dev)
            with torch.no_grad():
                cp = [p.detach().float().contiguous() for p in params]
            cparams = _native.MlgFFParams(*[_native.ptr(p) for p in cp])
            _native.call("mlg_ff_pack", _native.byref(d), _native.byref(cparams), _native.ptr(self._packed),
                         _native.stream_ptr())
            self._packed_key = key
        return self._packed

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self.mark_dirty()

    # ---- reference API -------------------------------------------------------------------------
    def init_hidden(self):
        """A zero [1, 1] placeholder; one cached tensor per device, so BasicMAC.init_hidden yields [B, N, 1] with no
        fill launch. (The reference returns zeros(batch_size, 1, 1), which BasicMAC.init_hidden cannot expand.)"""
        w = self.fc1.weight
        if self._h0 is None or self._h0.device != w.device or self._h0.dtype != w.dtype:
            self._h0 = w.new_zeros(1, 1)
        return self._h0

    def enable_autograd(self, flag: bool = True):
        """Opt in to a differentiable forward (also from ``args.native_autograd``): in grad mode, with a parameter
        or the input requiring grad, forward goes through ``maleague::dqn_forward`` with the live parameters and
        ``loss.backward()`` reaches them (HIP backward, ``mlg_ff_backward``). Off by default. Values are
        bit-identical either way."""
        self._autograd = bool(flag)
        return self

    def _live_params(self):
        """The parameters in named_parameters() order (PARAM_ORDER)."""
        return [self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias]

    def wants_grad(self, *tensors) -> bool:
        """The routing condition of the differentiable path."""
        return (self._autograd and torch.is_grad_enabled()
                and (any(p.requires_grad for p in self._live_params())
                     or any(t is not None and t.requires_grad for t in tensors)))

    def forward(self, inputs, hidden_state):
        x = inputs.float().contiguous()
        from ...ops import struct_fields
        if self.wants_grad(inputs):
            params = [p.float().contiguous() for p in self._live_params()]
            q = torch.ops.maleague.dqn_forward(params, self.packed(), x, struct_fields(self.dims()))
        else:
            q = torch.ops.maleague.ff_forward(self.packed(), x, struct_fields(self.dims()))
        return q, hidden_state
