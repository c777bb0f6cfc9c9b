"""Multi-agent controller without parameter sharing (API of src/marl/controllers/distinct_agents_controller.py:12-95):
agent slot i acts with network i.

forward(ep_batch, t) builds the agent inputs [obs_t | onehot(a_{t-1})] and runs the N DRQN cells in one fused gfx950
kernel (mlg_mac_forward_distinct) from a packed pool [N][mlg_packed_agent_size]: a 16-row MFMA tile is one agent across
16 batch rows, its weight block selected by the tile's agent. Differences from the reference, on purpose:
the mapping slot i <-> network i holds at every batch size (the reference concatenates per-agent outputs agent-major
and views them batch-major, which is right at batch_size 1 only), and parameters() yields every network's parameters
(the reference's returns []).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import _native
from ..components.action_selectors import REGISTRY as action_REGISTRY
from ..components.batch_view import mlg_batch
from ..exceptions import HiddenStateNotInitialized
from ..modules.agents import DRQNAgentNetwork
from ..utils.checkpoint import save_module
from ..utils.flat import flat_view
from .basic_controller import BasicMAC


def refuse_distinct(mac, who: str):
    """The refusal of every path that holds ``mac.agent``: a DistinctMAC has ``mac.agents`` and no ``agent``."""
    if isinstance(mac, DistinctMAC):
        raise NotImplementedError(f"{who} does not support mac='distinct' (one network per agent slot): it drives "
                                  "parameter-shared MACs (mac='basic') only")


class DistinctMAC(BasicMAC):
    def __init__(self, scheme, groups, args):
        if getattr(args, "obs_agent_id", False):
            # the reference raises this from _build_inputs (distinct_agents_controller.py:91)
            raise NotImplementedError("Please deactivate agent id observation for distinct agents networks.")
        if args.agent != "rnn":
            raise NotImplementedError(f"mac='distinct' runs the recurrent agent (agent='rnn') only, got "
                                      f"agent={args.agent!r}")
        if getattr(args, "agent_output_type", "q") != "q":
            raise NotImplementedError(f"mac='distinct' supports agent_output_type='q' only, got "
                                      f"agent_output_type={args.agent_output_type!r}")
        # MultiAgentController.__init__ with `agents` (an nn.ModuleList) in place of `agent`
        self.n_agents = args.n_agents
        self.n_actions = args.n_actions
        self.args = args
        self.input_shape = self._get_input_shape(scheme)
        self.agents = self._build_agent(self.input_shape)
        self.agent_output_type = args.agent_output_type
        self.action_selector = action_REGISTRY[args.action_selector](args)
        self.hidden_states = None
        if getattr(args, "freeze_native", False):
            for p in self.agents.parameters():
                p.requires_grad = False
        self._pool = None
        self._pool_key = None

    def _build_agent(self, input_shape):
        return nn.ModuleList([DRQNAgentNetwork(input_shape, self.args) for _ in range(self.n_agents)])

    # ---- kernel plumbing ------------------------------------------------------------------------------------------
    def dims(self) -> _native.MlgAgentDims:
        return self.agents[0].dims()

    def mark_dirty(self):
        for a in self.agents:
            a.mark_dirty()

    def packed(self) -> torch.Tensor:
        """The packed pool [N][mlg_packed_agent_size] (row i = network i's mlg_pack_agent block); rebuilt when any
        network's parameters changed (the key scheme of DRQNAgentNetwork.packed). One mlg_pack_agent_pool launch when
        the parameters sit back to back in named_parameters() order with equal row strides (a learner's flat buffer),
        else one mlg_pack_agent per row."""
        per_agent = [a._live_params() for a in self.agents]
        key = tuple((a._dirty,) + tuple((p.data_ptr(), p._version) for p in ps)
                    for a, ps in zip(self.agents, per_agent))
        if self._pool is not None and key == self._pool_key:
            return self._pool
        d = self.dims()
        n = _native.load().mlg_packed_agent_size(_native.byref(d))
        if n < 0:
            raise _native.NativeError(_native.load().mlg_last_error().decode())
        dev = per_agent[0][0].device
        N = self.n_agents
        if self._pool is None or tuple(self._pool.shape) != (N, n) or self._pool.device != dev:
            self._pool = torch.empty(N, n, dtype=torch.float32, device=dev)
        flat = flat_view([p for ps in per_agent for p in ps])
        if flat is not None:
            _native.call("mlg_pack_agent_pool", _native.byref(d), flat.data_ptr(), flat.numel() // N, N,
                         _native.ptr(self._pool), _native.stream_ptr())
        else:
            for i, a in enumerate(self.agents):
                with torch.no_grad():
                    cp = [p.detach().float().contiguous() for p in
                          (a.fc1.weight, a.fc1.bias, a.gru.weight_ih, a.gru.bias_ih, a.gru.weight_hh, a.gru.bias_hh,
                           a.fc2.weight, a.fc2.bias)]
                cparams = _native.MlgAgentParams(*[_native.ptr(p) for p in cp])
                _native.call("mlg_pack_agent", _native.byref(d), _native.byref(cparams), _native.ptr(self._pool[i]),
                             _native.stream_ptr())
        self._pool_key = key
        return self._pool

    # ---- forward ----------------------------------------------------------------------------------------------------
    def forward(self, ep_batch, t, test_mode=False):
        if self.hidden_states is None:
            raise HiddenStateNotInitialized()
        if self._wants_grad():
            return self._grad_forward(ep_batch, t)
        return self._fused_forward(ep_batch, t)

    def _fused_forward(self, ep_batch, t):
        B, N, H = ep_batch.batch_size, self.n_agents, self.args.rnn_hidden_dim
        mb, keep = mlg_batch(ep_batch, required=("obs", "actions_onehot"))
        pool = self.packed()
        h_in = self.hidden_states.reshape(B * N, H).float().contiguous()
        q = torch.empty(B, N, self.n_actions, device=h_in.device)
        h_out = torch.empty(B, N, H, device=h_in.device)
        _native.call("mlg_mac_forward_distinct", _native.byref(self.dims()), _native.ptr(pool), _native.byref(mb),
                     int(t), _native.ptr(h_in), _native.ptr(q), _native.ptr(h_out), _native.stream_ptr())
        del keep
        self.hidden_states = h_out
        return q

    def _grad_forward(self, ep_batch, t):
        """Differentiable path: agent-major inputs [N][B][d_in], network i on its contiguous slice
        (maleague::drqn_forward), outputs back as [B, N, A]; hidden_states carries the graph across steps."""
        B, N, H = ep_batch.batch_size, self.n_agents, self.args.rnn_hidden_dim
        x = self._build_inputs(ep_batch, t).float().transpose(0, 1).contiguous()  # [N, B, d_in]
        h = self.hidden_states.reshape(B, N, H)
        qs, hs = [], []
        for i, agent in enumerate(self.agents):
            q_i, h_i = agent(x[i], h[:, i])
            qs.append(q_i)
            hs.append(h_i)
        self.hidden_states = torch.stack(hs, dim=1)
        return torch.stack(qs, dim=1)

    def _build_inputs(self, batch, t):
        """[obs_t | onehot(a_{t-1})] as [B, N, d_in] (distinct_agents_controller.py:82-95)."""
        inputs = [batch["obs"][:, t]]
        if self.args.obs_last_action:
            oh = batch["actions_onehot"]
            inputs.append(torch.zeros_like(oh[:, t]) if t == 0 else oh[:, t - 1])
        return torch.cat([x.float() for x in inputs], dim=2)

    def enable_autograd(self, flag: bool = True):
        """Every network on maleague::drqn_forward: in grad mode forward(ep_batch, t) calls network i on agent i's
        rows, so a loss over the unrolled outputs backpropagates through time into each network. Under no_grad, or
        when not enabled, forward stays the fused mlg_mac_forward_distinct call."""
        for a in self.agents:
            a.enable_autograd(flag)
        return self

    def _wants_grad(self) -> bool:
        return any(a.wants_grad(self.hidden_states) for a in self.agents)

    # ---- reference API ----------------------------------------------------------------------------------------------
    def init_hidden(self, batch_size):
        self.hidden_states = self.agents[0].init_hidden().unsqueeze(0).expand(batch_size, self.n_agents, -1)

    def update_trained_steps(self, trained_steps):
        """Sets every network's counter (distinct_agents_controller.py:46-51; BasicMAC's adds)."""
        for a in self.agents:
            a.trained_steps = trained_steps

    def parameters(self):
        """Every network's parameters, agent 0 first, in named_parameters() order (the reference's returns []: its
        `params + list(...)` is discarded, distinct_agents_controller.py:53-56)."""
        return [p for a in self.agents for p in a.parameters()]

    def load_state(self, other_mac, agents=None):
        src = agents if agents is not None else other_mac.agents
        for a, o in zip(self.agents, src):
            a.load_state_dict(o.state_dict())

    def load_state_dict(self, agents):
        for a, sd in zip(self.agents, agents):
            a.load_state_dict(sd)

    def cuda(self):
        self.agents.cuda()

    def save_models(self, path, name):
        for i, a in enumerate(self.agents):
            save_module(a, f"{path}/{name}agent_{i}.th")

    def load_models(self, path, name):
        for i, a in enumerate(self.agents):
            a.load_state_dict(torch.load(f"{path}/{name}agent_{i}.th", map_location=lambda s, loc: s,
                                         weights_only=True))
