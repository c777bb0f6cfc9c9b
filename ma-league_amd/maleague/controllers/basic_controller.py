"""Parameter-shared multi-agent controller (API of src/marl/controllers/basic_controller.py:12-101).

forward(ep_batch, t) builds the agent inputs [obs_t | onehot(a_{t-1}) | agent id] and runs the DRQN
cell in one fused gfx950 kernel (mlg_mac_forward); the input concatenation is never materialised.
"""
from __future__ import annotations

from typing import OrderedDict

import torch

from .. import _native
from ..components.action_selectors import REGISTRY as action_REGISTRY
from ..components.batch_view import mlg_batch
from ..exceptions import HiddenStateNotInitialized
from ..modules.agents import REGISTRY as agent_REGISTRY
from ..utils.checkpoint import save_module


class MultiAgentController:
    def __init__(self, scheme, groups, args):
        self.n_agents = args.n_agents
        self.n_actions = args.n_actions
        self.args = args
        self.input_shape = self._get_input_shape(scheme)
        self.agent = self._build_agent(self.input_shape)
        self.agent_output_type = args.agent_output_type
        self.action_selector = action_REGISTRY[args.action_selector](args)
        self.hidden_states = None
        self.agent.trained_steps = 0
        if getattr(args, "freeze_native", False):
            for p in self.agent.parameters():
                p.requires_grad = False

    def _build_agent(self, input_shape):
        raise NotImplementedError()

    def _get_input_shape(self, scheme):
        raise NotImplementedError()


class BasicMAC(MultiAgentController):
    def select_actions(self, ep_batch, t_ep, t_env, bs=slice(None), test_mode=False):
        avail_actions = ep_batch["avail_actions"][:, t_ep]
        agent_outs = self.forward(ep_batch, t_ep, test_mode=test_mode)
        return self.action_selector.select(agent_outs[bs], avail_actions[bs], t_env, test_mode)

    def forward(self, ep_batch, t, test_mode=False):
        if self.agent_output_type not in ("q", "pi_logits"):
            raise NotImplementedError(f"agent_output_type={self.agent_output_type!r} is not supported (q, pi_logits)")
        if self.hidden_states is None:
            raise HiddenStateNotInitialized()
        B, N, H = ep_batch.batch_size, self.n_agents, self.args.rnn_hidden_dim
        if self._wants_grad():
            # differentiable path: hidden_states carries the graph across steps
            q, h = self.agent(self._build_inputs(ep_batch, t), self.hidden_states)
            self.hidden_states = h
            q = q.view(B, N, self.n_actions)
            return self._softmax(q, ep_batch, t, test_mode) if self.agent_output_type == "pi_logits" else q
        if self.agent_output_type == "pi_logits":
            with torch.no_grad():
                return self._softmax(self._fused_forward(ep_batch, t), ep_batch, t, test_mode)
        return self._fused_forward(ep_batch, t)

    def _softmax(self, logits, ep_batch, t, test_mode):
        """MultiAgentController._softmax (multi_agent_controller.py:78-99) as one HIP op: probabilities [B, N, A];
        epsilon is the action selector's, as in the reference."""
        avail = ep_batch["avail_actions"][:, t].to(torch.int32)
        return torch.ops.maleague.policy_probs(logits, avail, float(self.action_selector.epsilon),
                                               int(bool(getattr(self.args, "mask_before_softmax", True))),
                                               int(bool(test_mode)))

    def _fused_forward(self, ep_batch, t):
        B, N, H = ep_batch.batch_size, self.n_agents, self.args.rnn_hidden_dim
        mb, keep = mlg_batch(ep_batch, required=("obs", "actions_onehot"))
        if not getattr(self.agent, "recurrent", True):
            # feed-forward agent (agent: dqn): no hidden state to read or to carry, hidden_states stays as it is
            packed = self.agent.packed()
            q = torch.empty(B, N, self.n_actions, device=packed.device)
            _native.call("mlg_ff_mac_forward", _native.byref(self.agent.dims()), _native.ptr(packed),
                         _native.byref(mb), int(t), _native.ptr(q), _native.stream_ptr())
            del keep
            return q
        h_in = self.hidden_states.reshape(B * N, H).float().contiguous()
        q = torch.empty(B, N, self.n_actions, device=h_in.device)
        h_out = torch.empty(B * N, H, device=h_in.device)
        d = self.agent.dims()
        _native.call("mlg_mac_forward", _native.byref(d), _native.ptr(self.agent.packed()), _native.byref(mb), int(t),
                     _native.ptr(h_in), _native.ptr(q), _native.ptr(h_out), _native.stream_ptr())
        del keep
        self.hidden_states = h_out
        return q

    def enable_autograd(self, flag: bool = True):
        """Opt in to a differentiable forward (DRQNAgentNetwork.enable_autograd): in grad mode forward(ep_batch, t)
        then builds the agent inputs with torch ops and calls the agent module, so a loss over the unrolled
        outputs backpropagates through time. Under no_grad, or when not enabled, forward stays the fused
        mlg_mac_forward call."""
        self.agent.enable_autograd(flag)
        return self

    def _wants_grad(self) -> bool:
        wants = getattr(self.agent, "wants_grad", None)
        return wants is not None and wants(self.hidden_states)

    def _build_inputs(self, batch, t):
        """[obs_t | onehot(a_{t-1}) | eye(N)] as [B * N, d_in] (basic_controller.py:80-92)."""
        B, N = batch.batch_size, self.n_agents
        inputs = [batch["obs"][:, t]]
        if self.args.obs_last_action:
            oh = batch["actions_onehot"]
            inputs.append(torch.zeros_like(oh[:, t]) if t == 0 else oh[:, t - 1])
        if self.args.obs_agent_id:
            inputs.append(torch.eye(N, device=inputs[0].device).unsqueeze(0).expand(B, -1, -1))
        return torch.cat([x.reshape(B * N, -1).float() for x in inputs], dim=1)

    def update_trained_steps(self, update):
        self.agent.add_trained_steps(update)

    def init_hidden(self, batch_size):
        self.hidden_states = self.agent.init_hidden().unsqueeze(0).expand(batch_size, self.n_agents, -1)

    def parameters(self):
        return self.agent.parameters()

    def load_state(self, other_mac):
        self.agent.load_state_dict(other_mac.agent.state_dict())

    def load_state_dict(self, agent: OrderedDict):
        self.agent.load_state_dict(agent)

    def cuda(self):
        self.agent.cuda()

    def save_models(self, path, name):
        save_module(self.agent, f"{path}/{name}agent.th")

    def load_models(self, path, name):
        self.agent.load_state_dict(torch.load(f"{path}/{name}agent.th", map_location=lambda s, loc: s,
                                              weights_only=True))

    def _build_agent(self, input_shape):
        return agent_REGISTRY[self.args.agent](input_shape, self.args)

    def _get_input_shape(self, scheme):
        shape = scheme["obs"]["vshape"]
        if self.args.obs_last_action:
            shape += scheme["actions_onehot"]["vshape"][0]
        if self.args.obs_agent_id:
            shape += self.n_agents
        return shape
