"""COMA learner (API, stat keys and checkpoint files of src/marl/learners/coma_learner.py:24-189).

train() queues, without a host wait: the critic pipeline (``mlg_coma_critic_train``: target critic, TD(lambda)
targets, one clipped RMSprop step per timestep from the last to the first), the MAC's differentiable unroll
(``maleague::drqn_forward`` + ``maleague::policy_probs`` per step, HIP backward), the actor loss
(``maleague::coma_policy_loss``, forward and d pi in one launch) and the device-side target-critic update
(``mlg_coma_target_update``). Gradient clipping and RMSprop of the agent are torch's. The critic's
parameters, gradients and RMSprop state live in flat fp32 buffers like the Q learners'; the nn.Module parameters are
views into them, so ``critic.th`` / ``critic_opt.th`` load in the reference and the reverse.
"""
from __future__ import annotations

import copy

import torch

from .. import _native
from ..components.batch_view import mlg_batch
from ..controllers.distinct_controller import refuse_distinct
from ..modules.agents import DQNAgentNetwork
from ..modules.critics import COMACritic
from ..modules.critics.coma import CRITIC_ORDER, HIDDEN
from ..utils.checkpoint import save_module, save_optimizer
from .q_learner import FlatParams, Learner

CRITIC_STATS = ("critic_loss", "critic_grad_norm", "td_error_abs", "q_taken_mean", "target_mean")


def build_td_lambda_targets(rewards, terminated, mask, target_qs, n_agents, gamma, td_lambda):
    """coma_learner.py:10-21: target_qs [B, T, N]; rewards, terminated, mask [B, T-1, 1] -> the lambda-returns
    [B, T-1, N]. Plain tensor code on whatever device the inputs are on (``mlg_coma_critic_train`` runs the same
    recursion in its TD(lambda) launch; this function is the public counterpart)."""
    ret = target_qs.new_zeros(*target_qs.shape)
    ret[:, -1] = target_qs[:, -1] * (1 - torch.sum(terminated, dim=1))
    for t in reversed(range(ret.shape[1] - 1)):
        ret[:, t] = td_lambda * gamma * ret[:, t + 1] + mask[:, t] * (
            rewards[:, t] + (1 - td_lambda) * gamma * target_qs[:, t + 1] * (1 - terminated[:, t]))
    return ret[:, 0:-1]


class COMALearner(Learner):
    def __init__(self, mac, scheme, logger, args, name=None):
        super().__init__(mac, scheme, logger, args, name)
        if getattr(args, "prioritized_replay", False):
            raise ValueError(f"COMALearner: prioritized_replay=True is not supported (its kernels take no importance weights "
                             f"and report no per-episode errors); QLearner does")
        self.n_agents = args.n_agents
        self.n_actions = args.n_actions
        for key, want in (("critic_train_mode", "seq"), ("q_nstep", 0)):
            got = getattr(args, key, want)
            if got != want:
                raise NotImplementedError(f"COMALearner supports {key}={want!r} only, got {key}={got!r}")
        refuse_distinct(mac, "COMALearner")
        if getattr(mac, "agent_output_type", "pi_logits") != "pi_logits":
            raise ValueError(f"COMALearner needs agent_output_type='pi_logits', got {mac.agent_output_type!r}")
        if isinstance(getattr(mac, "agent", None), DQNAgentNetwork):
            raise NotImplementedError("COMALearner trains the recurrent agent (agent='rnn') only: agent='dqn' with "
                                      "agent_output_type='pi_logits' is not supported")
        self.critic = COMACritic(scheme, args)
        self.target_critic = copy.deepcopy(self.critic)
        self.device = torch.device(getattr(args, "device", "cuda"))
        self.agent_params = list(mac.parameters())
        self.critic_params = list(self.critic.parameters())
        self.params = self.agent_params + self.critic_params
        self.agent_optimiser = None
        self.critic_optimiser = None
        self._ws = None
        self._cstats = None
        self._astats = None
        self._grad_norm = None
        self._counters = None
        self._step_base = 0.0
        self.q_vals = None
        self.targets = None
        self.train_calls = 0
        mac.enable_autograd()

    # ---- reference attributes resolved from the device counters (reading them syncs the stream) -------------------
    @property
    def critic_training_steps(self) -> int:
        return 0 if self._counters is None else int(self._counters[0].item())

    @property
    def last_target_update_step(self) -> int:
        return 0 if self._counters is None else int(self._counters[1].item())

    def parameters(self):
        return self.params

    def build_optimizer(self):
        names = [n for n, _ in self.critic.named_parameters()]
        if names != CRITIC_ORDER:
            raise RuntimeError(f"critic parameter order {names} != kernel layout {CRITIC_ORDER}")
        for m in (self.mac.agent, self.critic, self.target_critic):
            m.to(self.device)
        a = self.args
        self._flat = FlatParams(self.critic_params, self.device)
        self._tflat = FlatParams(self.target_critic.parameters(), self.device)
        self._grads = torch.zeros_like(self._flat.flat)
        self._sq = torch.zeros_like(self._flat.flat)
        self._flat.attach_grads(self._grads)
        self.agent_optimiser = torch.optim.RMSprop(params=self.agent_params, lr=a.lr, alpha=a.optim_alpha,
                                                   eps=a.optim_eps)
        self.critic_optimiser = torch.optim.RMSprop(params=self.critic_params, lr=a.critic_lr, alpha=a.optim_alpha,
                                                    eps=a.optim_eps)
        self.optimiser = self.agent_optimiser
        self._step = torch.zeros((), dtype=torch.float32)
        self._bind_critic_state()
        self._cstats = torch.zeros(6, dtype=torch.float32, device=self.device)
        self._counters = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.mac.agent.mark_dirty()

    def _bind_critic_state(self):
        for p, off, k in self._flat.views:
            self.critic_optimiser.state[p] = {"step": self._step, "square_avg": self._sq[off:off + k].view_as(p)}

    def _cfg(self, B, T):
        a = self.args
        d = self.mac.agent.dims()
        return _native.MlgComaCfg(B=B, T=T, N=a.n_agents, A=a.n_actions, d_obs=d.d_obs, S=int(a.state_shape),
                                  hidden=HIDDEN, lr=float(a.critic_lr), optim_alpha=float(a.optim_alpha),
                                  optim_eps=float(a.optim_eps), grad_norm_clip=float(a.grad_norm_clip),
                                  gamma=float(a.gamma), td_lambda=float(a.td_lambda))

    def _train_critic(self, batch):
        """coma_learner.py:121-169 as one call; returns q_vals [B, T-1, N, A] (zeros at skipped steps)."""
        lib = _native.load(require_gpu=True)
        B, T = batch.batch_size, batch.max_seq_length
        cfg = self._cfg(B, T)
        need = lib.mlg_coma_workspace_floats(_native.byref(cfg))
        if need < 0:
            raise _native.NativeError(lib.mlg_last_error().decode())
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(int(need * 1.25) + 1024, dtype=torch.float32, device=self.device)
        mb, keep = mlg_batch(batch)
        self.q_vals = torch.empty(B, T - 1, self.n_agents, self.n_actions, dtype=torch.float32, device=self.device)
        self.targets = torch.empty(B, T - 1, self.n_agents, dtype=torch.float32, device=self.device)
        bufs = _native.MlgComaBufs(mb, self._flat.flat.data_ptr(), self._grads.data_ptr(), self._sq.data_ptr(),
                                   self._tflat.flat.data_ptr(), self._ws.data_ptr(), self.q_vals.data_ptr(),
                                   self.targets.data_ptr(), self._cstats.data_ptr(), self._counters.data_ptr())
        _native.call("mlg_coma_critic_train", _native.byref(cfg), _native.byref(bufs), _native.stream_ptr(self.device))
        del keep
        return self.q_vals

    def train(self, batch, t_env, episode_num: int):
        """coma_learner.py:49-119. `t_env` may also be a zero-argument callable, resolved after the device work is
        queued (as QLearner.train)."""
        if self.critic_optimiser is None:
            raise RuntimeError("call build_optimizer() before train()")
        if batch.max_seq_length < 2:
            raise ValueError("COMALearner.train needs at least two timesteps")
        q_vals = self._train_critic(batch)  # first: a sampled view is still read in place through its slot map
        T = batch.max_seq_length
        terminated = batch["terminated"][:, :-1].float()
        mask = batch["filled"][:, :-1].float()
        mask[:, 1:] = mask[:, 1:] * (1 - terminated[:, :-1])
        avail = batch["avail_actions"][:, :-1].to(torch.int32)
        actions = batch["actions"][:, :-1]

        self.mac.init_hidden(batch.batch_size)
        mac_out = torch.stack([self.mac.forward(batch, t=t) for t in range(T - 1)], dim=1)
        stats, _ = torch.ops.maleague.coma_policy_loss(mac_out, avail, actions, q_vals, mask)
        self.agent_optimiser.zero_grad()
        stats[0].backward()
        self._grad_norm = torch.nn.utils.clip_grad_norm_(self.agent_params, self.args.grad_norm_clip)
        self.agent_optimiser.step()
        self.mac.agent.mark_dirty()
        # trained steps accumulate on the agent's device counter, no host wait (the reference's COMA learner never
        # calls update_trained_steps; the league's checkpoint thresholds need the count: DESIGN.md §7)
        self.mac.agent.add_trained_steps(torch.count_nonzero(mask))
        self._astats = stats.detach()
        self.train_calls += 1

        _native.call("mlg_coma_target_update", self._flat.flat.data_ptr(), self._tflat.flat.data_ptr(),
                     self._flat.flat.numel(), self._counters.data_ptr(), int(self.args.target_update_interval),
                     _native.stream_ptr(self.device))

        if callable(t_env):
            up = getattr(t_env, "upper", None)
            if up is not None and up() - self.log_stats_t < self.args.learner_log_interval:
                return
            t_env = t_env()
        if t_env - self.log_stats_t >= self.args.learner_log_interval:
            for k, v in self.last_stats.items():
                self.logger.log_stat(k, v, t_env)
            self.log_stats_t = t_env

    @property
    def last_stats(self):
        """The stats of the latest train() under the reference's keys (coma_learner.py:108-119): the critic's
        unprefixed means over the taken steps (left out when no step was taken), the actor's with the learner's
        name. Reading them syncs the stream."""
        if self._astats is None:
            return {}
        cs, st = self._cstats.cpu(), self._astats.cpu()
        out = {}
        taken = float(cs[5])
        if taken > 0:
            for i, k in enumerate(CRITIC_STATS):
                out[k] = float(cs[i]) / taken
        out[self.name + "advantage_mean"] = float(st[1])
        out[self.name + "coma_loss"] = float(st[0])
        out[self.name + "agent_grad_norm"] = float(self._grad_norm)
        out[self.name + "pi_max"] = float(st[2])
        return out

    def update_targets(self):
        self._tflat.flat.copy_(self._flat.flat)
        self.logger.info("Updated target network")

    def cuda(self):
        pass

    def save_models(self, path, name=None):
        """coma_learner.py:175-179: {name}agent.th, critic.th, agent_opt.th, critic_opt.th."""
        self.mac.save_models(path, name=self.name)
        save_module(self.critic, f"{path}/critic.th")
        save_optimizer(self.agent_optimiser, f"{path}/agent_opt.th")
        self._step.fill_(self._step_base + float(self.critic_training_steps))
        save_optimizer(self.critic_optimiser, f"{path}/critic_opt.th")

    def load_models(self, path):
        """coma_learner.py:181-189 (the target critic is not saved: it restarts from the critic)."""
        self.mac.load_models(path, self.name)
        loc = lambda s, _loc: s  # noqa: E731
        self.critic.load_state_dict(torch.load(f"{path}/critic.th", map_location=loc, weights_only=True))
        self._tflat.flat.copy_(self._flat.flat)
        self.agent_optimiser.load_state_dict(torch.load(f"{path}/agent_opt.th", map_location=loc, weights_only=True))
        self.critic_optimiser.load_state_dict(torch.load(f"{path}/critic_opt.th", map_location=loc,
                                                         weights_only=True))
        for p, off, k in self._flat.views:  # re-home the loaded RMSprop state into the flat buffer
            st = self.critic_optimiser.state.get(p, {})
            if "square_avg" in st:
                self._sq[off:off + k].copy_(st["square_avg"].reshape(-1))
            if "step" in st:
                self._step_base = float(st["step"]) - float(self.critic_training_steps)
        self._bind_critic_state()
        self.mac.agent.mark_dirty()
