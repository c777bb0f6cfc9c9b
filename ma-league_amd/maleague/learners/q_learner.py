"""QMIX/VDN/IQL Q-learner (API of src/marl/learners/learner.py:6-79 and q_learner.py:15-147).

train() is one call into the fused gfx950 pipeline (mlg_qlearner_train): online + target BPTT unrolls,
double-Q targets, mixer forward/backward, masked TD loss, all weight gradients, clip_grad_norm_ and the
RMSprop step. To make that possible the parameters of the MAC and mixer (and of their target copies)
are re-homed into flat fp32 buffers; the nn.Module parameters become views into them, so state_dict()
keys, checkpoint files and torch.optim.RMSprop.state_dict() stay compatible with the reference.

With a DistinctMAC (mac: distinct, one network per agent slot) train() is the same call with cfg.distinct = 1: the flat
vectors are [agent 0 | ... | agent N-1 | mixer] and the agent kernels run the N networks by a grid coordinate
(DESIGN.md §4j). MLG_DISTINCT_LEARNER=unrolled in the environment (read per call) takes the unrolled branch instead
(_train_distinct): the MAC's differentiable forward per step, the mixer op with its HIP backward,
torch's clip_grad_norm_ and RMSprop. Both work on the same flat parameters, gradients and RMSprop state, so a learner
may switch between them from one call to the next.
"""
from __future__ import annotations

import copy
import os

import torch

from .. import _native
from ..components.batch_view import mlg_batch
from ..controllers.distinct_controller import DistinctMAC
from ..modules.agents import DQNAgentNetwork
from ..modules.mixers import QMixer, VDNMixer
from ..utils.checkpoint import save_module, save_optimizer

AGENT_ORDER = ["fc1.weight", "fc1.bias", "gru.weight_ih", "gru.weight_hh", "gru.bias_ih", "gru.bias_hh",
               "fc2.weight", "fc2.bias"]
QMIX_ORDER = ["hyper_w_1.0.weight", "hyper_w_1.0.bias", "hyper_w_1.2.weight", "hyper_w_1.2.bias",
              "hyper_w_final.0.weight", "hyper_w_final.0.bias", "hyper_w_final.2.weight", "hyper_w_final.2.bias",
              "hyper_b_1.weight", "hyper_b_1.bias", "V.0.weight", "V.0.bias", "V.2.weight", "V.2.bias"]
# hypernet_layers 1 (the reference QMixer's fallback, qmix.py:17): the hypernets are single Linear layers
QMIX1_ORDER = ["hyper_w_1.weight", "hyper_w_1.bias", "hyper_w_final.weight", "hyper_w_final.bias",
               "hyper_b_1.weight", "hyper_b_1.bias", "V.0.weight", "V.0.bias", "V.2.weight", "V.2.bias"]


class FlatParams:
    """Moves `params` into one contiguous fp32 device buffer; each Parameter becomes a view of it."""

    def __init__(self, params, device):
        params = list(params)
        n = sum(p.numel() for p in params)
        self.flat = torch.empty(n, dtype=torch.float32, device=device)
        self.views = []
        off = 0
        for p in params:
            k = p.numel()
            self.flat[off:off + k].copy_(p.detach().reshape(-1))
            p.data = self.flat[off:off + k].view_as(p)
            self.views.append((p, off, k))
            off += k

    def attach_grads(self, gflat):
        for p, off, k in self.views:
            p.grad = gflat[off:off + k].view_as(p)


class Learner:
    def __init__(self, mac, scheme, logger, args, name=None):
        self.mac = mac
        self.scheme = scheme
        self.logger = logger
        self.args = args
        self.name = f'{"" if name is None else name}_{self.__class__.__name__.lower()}_'
        self.log_stats_t = -self.args.learner_log_interval - 1
        self.optimiser = None

    def parameters(self):
        raise NotImplementedError()

    def train(self, batch, t_env: int, episode_num: int):
        raise NotImplementedError()

    def update_targets(self):
        pass


class QLearner(Learner):
    def __init__(self, mac, scheme, logger, args, name=None):
        super().__init__(mac, scheme, logger, args, name)
        self.last_target_update_episode = 0
        self.mixer = None
        if args.mixer is not None:
            if args.mixer == "vdn":
                self.mixer = VDNMixer()
            elif args.mixer == "qmix":
                self.mixer = QMixer(args)
            else:
                raise ValueError(f"Mixer {args.mixer} not recognised.")
            self.target_mixer = copy.deepcopy(self.mixer)
        self.target_mac = copy.deepcopy(mac)
        self.device = torch.device(getattr(args, "device", "cuda"))
        self._ws = None
        self._stats = None
        self._last_stats = None
        self._stats_fresh = False
        self.train_calls = 0
        # prioritized replay: the latest call's per-episode errors (device, [B]) when the batch carried .is_weight
        self.last_td_abs = None
        # one network per agent slot: mlg_qlearner_train with cfg.distinct = 1; autograd stays enabled for the unrolled
        # branch (MLG_DISTINCT_LEARNER=unrolled), which the fused call never enters (it runs no torch graph)
        self._distinct = isinstance(mac, DistinctMAC)
        self._tcount = None  # distinct: the N networks' trained-steps counters as one float64 vector
        self._tviews = None
        if self._distinct:
            mac.enable_autograd()
            if isinstance(self.mixer, QMixer):
                self.mixer.enable_autograd()

    def parameters(self):
        # the reference's precedence slip (q_learner.py:30-32) returns [] for IQL; VDN/QMIX are unaffected
        return list(self.mac.parameters()) + (list(self.mixer.parameters()) if self.mixer is not None else [])

    def _target_parameters(self):
        return list(self.target_mac.parameters()) + (list(self.target_mixer.parameters())
                                                     if self.mixer is not None else [])

    def _check_order(self):
        for agent in (self.mac.agents if self._distinct else [self.mac.agent]):
            names = [n for n, _ in agent.named_parameters()]
            order = list(getattr(agent, "PARAM_ORDER", AGENT_ORDER))  # the feed-forward agent carries its own
            if names != order:
                raise RuntimeError(f"agent parameter order {names} != kernel layout {order}")
        if isinstance(self.mixer, QMixer):
            names = [n for n, _ in self.mixer.named_parameters()]
            order = QMIX1_ORDER if self.mixer.hypernet_layers == 1 else QMIX_ORDER
            if names != order:
                raise RuntimeError(f"mixer parameter order {names} != kernel layout {order}")

    def build_optimizer(self):
        """Parameters re-homed into one flat buffer (a DistinctMAC's N networks back to back, then the mixer: the MAC's
        pool then packs in one mlg_pack_agent_pool launch and the target update is one copy), the gradient and RMSprop
        square_avg vectors beside it; torch.optim.RMSprop carries the state dict."""
        self._check_order()
        nets = [self.mac.agents, self.target_mac.agents] if self._distinct else [self.mac.agent, self.target_mac.agent]
        for m in nets + ([self.mixer, self.target_mixer] if self.mixer else []):
            m.to(self.device)
        params = self.parameters()
        self._flat = FlatParams(params, self.device)
        self._tflat = FlatParams(self._target_parameters(), self.device)
        self._grads = torch.zeros_like(self._flat.flat)
        self._sq = torch.zeros_like(self._flat.flat)
        self._flat.attach_grads(self._grads)
        a = self.args
        self.optimiser = torch.optim.RMSprop(params=params, lr=a.lr, alpha=a.optim_alpha, eps=a.optim_eps)
        self._step = torch.zeros((), dtype=torch.float32)
        for p, off, k in self._flat.views:
            self.optimiser.state[p] = {"step": self._step, "square_avg": self._sq[off:off + k].view_as(p)}
        self._stats = torch.zeros(8, dtype=torch.float32, device=self.device)
        self._online().mark_dirty()
        self._target().mark_dirty()

    def _online(self):
        """What holds the online networks' packed weights: the DistinctMAC itself (a pool), else the shared agent."""
        return self.mac if self._distinct else self.mac.agent

    def _target(self):
        return self.target_mac if self._distinct else self.target_mac.agent

    def _trained_counters(self):
        """distinct: the networks' device-side trained-steps counts as one float64 vector [N] (element i seated as
        network i's count), so the optimizer launch adds to all of them. Re-seated when a count was set from outside."""
        agents = self.mac.agents
        if self._tcount is None or not all(a.trained_counter_is(v) for a, v in zip(agents, self._tviews)):
            self._tcount = torch.stack([a.trained_counter(self.device) for a in agents])
            self._tviews = [a.seat_trained_counter(self._tcount[i]) for i, a in enumerate(agents)]
        return self._tcount

    def _is_weight(self, batch):
        """The batch's importance weights (a PrioritizedReplayBuffer sample) as fp32 [B] on the device, else None."""
        w = getattr(batch, "is_weight", None)
        if w is None:
            return None
        w = torch.as_tensor(w, dtype=torch.float32).to(self.device).contiguous().reshape(-1)
        if w.numel() != batch.batch_size:
            raise ValueError(f"is_weight has {w.numel()} entries for {batch.batch_size} episodes")
        return w

    def _cfg(self, B, T, per=False):
        a = self.args
        d = self._online().dims()
        mixer = 2 if isinstance(self.mixer, QMixer) else (1 if isinstance(self.mixer, VDNMixer) else 0)
        return _native.MlgLearnerCfg(B=B, T=T, N=a.n_agents, A=a.n_actions, d_obs=d.d_obs, H=a.rnn_hidden_dim,
                             S=int(a.state_shape), E=int(getattr(a, "mixing_embed_dim", 32)),
                             HE=int(getattr(a, "hypernet_embed", 64)), hypernet_layers=int(getattr(a, "hypernet_layers", 1)),
                             mixer=mixer, double_q=int(bool(a.double_q)), obs_last_action=int(bool(a.obs_last_action)),
                             obs_agent_id=int(bool(a.obs_agent_id)), gamma=float(a.gamma), lr=float(a.lr),
                             optim_alpha=float(a.optim_alpha), optim_eps=float(a.optim_eps),
                             grad_norm_clip=float(a.grad_norm_clip),
                             agent=int(not self._distinct and isinstance(self.mac.agent, DQNAgentNetwork)),
                             distinct=int(self._distinct), per=int(per))

    def train(self, batch, t_env, episode_num: int):
        """q_learner.py:34-131. `t_env` may also be a zero-argument callable, resolved after the device work
        is queued (lets the caller avoid a host sync before the launch)."""
        if self.optimiser is None:
            raise RuntimeError("call build_optimizer() before train()")
        if self._distinct:
            which = os.environ.get("MLG_DISTINCT_LEARNER", "fused")  # read per call, as MLG_LEARNER_FULL
            if which == "unrolled":
                return self._train_distinct(batch, t_env, episode_num)
            if which != "fused":
                raise ValueError(f"MLG_DISTINCT_LEARNER={which!r} not recognised (fused, unrolled)")
        lib = _native.load(require_gpu=True)
        weights = self._is_weight(batch)
        cfg = self._cfg(batch.batch_size, batch.max_seq_length, per=weights is not None)
        td_abs = None if weights is None else torch.empty(batch.batch_size, dtype=torch.float32, device=self.device)
        need = lib.mlg_qlearner_workspace_floats(_native.byref(cfg))
        if need < 0:
            raise _native.NativeError(lib.mlg_last_error().decode())
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.zeros(int(need * 1.25) + 1024, dtype=torch.float32, device=self.device)
        # a sampled view of the device buffer hands its slot map over as a kernel argument (no H2D copy)
        host_rows = getattr(batch, "host_rows", None)
        if host_rows is not None and (batch.batch_size > lib.mlg_qlearner_inline_rows()
                                      or getattr(batch, "_data", None) is not None):
            host_rows = None
        mb, keep = mlg_batch(batch, device_rows=host_rows is None)
        # the target update due after this step (q_learner.py:127-128) is written by the optimizer launch itself
        sync = (episode_num - self.last_target_update_episode) / self.args.target_update_interval >= 1.0
        # no host sync per train step: trained steps accumulate on the device (Agent.trained_steps)
        counter = self._trained_counters() if self._distinct else self.mac.agent.trained_counter(self.device)
        bufs = _native.MlgLearnerBufs(mb, self._flat.flat.data_ptr(), self._grads.data_ptr(), self._sq.data_ptr(),
                                      self._tflat.flat.data_ptr(), self._ws.data_ptr(), self._stats.data_ptr(),
                                      self._tflat.flat.data_ptr() if sync else None, counter.data_ptr(),
                                      None if host_rows is None else host_rows.ctypes.data,
                                      None if weights is None else weights.data_ptr(),
                                      None if td_abs is None else td_abs.data_ptr())
        _native.call("mlg_qlearner_train", _native.byref(cfg), _native.byref(bufs), _native.stream_ptr(self.device))
        del keep
        self.last_td_abs = td_abs
        self._step += 1
        self._online().mark_dirty()
        self.train_calls += 1
        if sync:
            self._target().mark_dirty()
            self.logger.info(f"Updated {self.name}target network.")
            self.last_target_update_episode = episode_num
        self._stats_fresh = True
        if callable(t_env):  # lazily resolved t_env: the kernels above are already queued
            up = getattr(t_env, "upper", None)
            if up is not None and up() - self.log_stats_t < self.args.learner_log_interval:
                return  # no log due for any t_env still possible: no wait for the runs in flight
            t_env = t_env()
        if t_env - self.log_stats_t >= self.args.learner_log_interval:
            for k, v in self.last_stats.items():
                self.logger.log_stat(self.name + k, v, t_env)
            self.log_stats_t = t_env

    # ---- mac: distinct -- the unrolled branch (MLG_DISTINCT_LEARNER=unrolled; the pattern COMALearner uses for its
    # actor), the same-commit comparator of the fused call ------------------------------------------------------------
    def _train_distinct(self, batch, t_env, episode_num):
        """q_learner.py:34-131 with torch ops over the MAC unrolls: the online MAC differentiably
        (maleague::drqn_forward per network and step, HIP backward), the target MAC under no_grad through the fused
        mlg_mac_forward_distinct; QMIX through maleague::qmix_forward (HIP backward), VDN's sum, or none. Gradients
        are autograd's, accumulated into the fused learner's gradient vector (every .grad is a view of it); the step is
        torch.optim.RMSprop's on the fused learner's square_avg vector, so the next call may be either branch's."""
        a = self.args
        rewards = batch["reward"][:, :-1]
        actions = batch["actions"][:, :-1]
        terminated = batch["terminated"][:, :-1].float()
        mask = batch["filled"][:, :-1].float()
        mask[:, 1:] = mask[:, 1:] * (1 - terminated[:, :-1])
        avail = batch["avail_actions"]
        T = batch.max_seq_length
        # the reference trains on the sample truncated to max_t_filled (ma_experiment.py:235-239): transitions from
        # max_t_filled - 1 on are masked out, on the device (no host sync), as the fused learner does
        te = batch["filled"][:, :, 0].sum(dim=1).max().clamp(min=2)
        mask = mask * (torch.arange(T - 1, device=mask.device) < te - 1).view(1, T - 1, 1).float()
        self.mac.init_hidden(batch.batch_size)
        mac_out = torch.stack([self.mac.forward(batch, t=t) for t in range(T)], dim=1)
        chosen = torch.gather(mac_out[:, :-1], dim=3, index=actions).squeeze(3)
        # A slot that is dead in every stored step (nothing but the no-op, action 0, was ever available to it) took no
        # decision in this batch. Its chosen Q keeps its value in the mix, the loss and the statistics, but passes no
        # gradient: the slot's own network gets exactly zero and is not moved (with shared parameters
        # the question does not arise). The other slots' gradients do not change.
        stored = (batch["filled"][:, :, 0] != 0).unsqueeze(2)
        alive = ((avail[..., 1:] != 0).any(dim=3) & stored).flatten(0, 1).any(dim=0)  # [N]
        chosen = torch.where(alive.view(1, 1, -1), chosen, chosen.detach())
        with torch.no_grad():
            self.target_mac.init_hidden(batch.batch_size)
            tmac = torch.stack([self.target_mac.forward(batch, t=t) for t in range(T)][1:], dim=1)
            tmac[avail[:, 1:] == 0] = -9999999
            if a.double_q:
                md = mac_out.detach().clone()
                md[avail == 0] = -9999999
                cur_max = md[:, 1:].max(dim=3, keepdim=True)[1]
                target_max = torch.gather(tmac, 3, cur_max).squeeze(3)
            else:
                target_max = tmac.max(dim=3)[0]
        if self.mixer is not None:
            chosen = self.mixer(chosen, batch["state"][:, :-1])
            with torch.no_grad():
                target_max = self.target_mixer(target_max, batch["state"][:, 1:])
        targets = rewards + a.gamma * (1 - terminated) * target_max
        td = chosen - targets.detach()
        mask = mask.expand_as(td)
        mtd = td * mask
        n = mask.sum()
        weights = self._is_weight(batch)  # prioritized replay: the weighted loss, the per-episode errors
        if weights is None:
            loss = (mtd ** 2).sum() / n
            self.last_td_abs = None
        else:
            loss = ((mtd ** 2).sum(dim=(1, 2)) * weights).sum() / n
            with torch.no_grad():
                ms = mask.sum(dim=(1, 2))
                self.last_td_abs = torch.where(ms > 0, mtd.abs().sum(dim=(1, 2)) / ms.clamp(min=1), torch.zeros_like(ms))
        self._grads.zero_()
        self._flat.attach_grads(self._grads)  # autograd then accumulates in place
        loss.backward()
        params = self.parameters()
        grad_norm = torch.nn.utils.clip_grad_norm_(params, a.grad_norm_clip)
        steps_done = float(self._step)
        self.optimiser.step()
        self._step.fill_(steps_done + 1)  # the one step tensor is every parameter's: torch counted it once for each
        self.mac.mark_dirty()
        self.train_calls += 1
        if (episode_num - self.last_target_update_episode) / a.target_update_interval >= 1.0:
            self.update_targets()
            self.last_target_update_episode = episode_num
        with torch.no_grad():
            steps = torch.count_nonzero(mask)
            for ag in self.mac.agents:  # no host sync: trained steps accumulate on the device (Agent.trained_steps)
                ag.add_trained_steps(steps)
            self._stats[:7] = torch.stack([loss.detach(), grad_norm.detach().reshape(()), mtd.abs().sum() / n,
                                           (chosen * mask).sum() / (n * a.n_agents),
                                           (targets * mask).sum() / (n * a.n_agents), n, steps.float()])
        self._stats_fresh = True
        if callable(t_env):
            up = getattr(t_env, "upper", None)
            if up is not None and up() - self.log_stats_t < a.learner_log_interval:
                return
            t_env = t_env()
        if t_env - self.log_stats_t >= a.learner_log_interval:
            for k, v in self.last_stats.items():
                self.logger.log_stat(self.name + k, v, t_env)
            self.log_stats_t = t_env

    @property
    def last_stats(self):
        """Stats of the latest train() (q_learner.py:115-124 values); reading them syncs the stream."""
        if self._stats is None or not self._stats_fresh:
            return self._last_stats
        st = self._stats.cpu()
        self._last_stats = {"loss": float(st[0]), "grad_norm": float(st[1]), "td_error_abs": float(st[2]),
                            "q_taken_mean": float(st[3]), "target_mean": float(st[4])}
        self._stats_fresh = False
        return self._last_stats

    def update_targets(self):
        self._tflat.flat.copy_(self._flat.flat)
        (self.target_mac if self._distinct else self.target_mac.agent).mark_dirty()
        self.logger.info(f"Updated {self.name}target network.")

    def cuda(self):
        pass

    def save_models(self, path, name):
        self.mac.save_models(path, name=self.name)
        if self.mixer is not None:
            save_module(self.mixer, f"{path}/{self.name}mixer.th")
        save_optimizer(self.optimiser, f"{path}/{self.name}opt.th")

    def load_models(self, path):
        self.mac.load_models(path, self.name)
        self.target_mac.load_models(path, self.name)  # target nets are not saved (q_learner.py:141-142)
        if self.mixer is not None:
            sd = torch.load(f"{path}/{self.name}mixer.th", map_location=lambda s, loc: s, weights_only=True)
            self.mixer.load_state_dict(sd)
        opt = torch.load(f"{path}/{self.name}opt.th", map_location=lambda s, loc: s, weights_only=True)
        self.optimiser.load_state_dict(opt)
        if self._distinct:
            # the target networks and mixer restart as copies of the online ones (as the branch did before it had a
            # fused form; an opt.th it wrote then holds torch's own per-parameter state and re-homes like any other)
            self._tflat.flat.copy_(self._flat.flat)
        for p, off, k in self._flat.views:  # re-home the loaded RMSprop state into the flat buffer
            st = self.optimiser.state.get(p, {})
            if "square_avg" in st:
                self._sq[off:off + k].copy_(st["square_avg"].reshape(-1))
            if "step" in st:  # one shared step counter (RMSprop steps every parameter together)
                self._step.fill_(float(st["step"]))
            self.optimiser.state[p] = {"step": self._step, "square_avg": self._sq[off:off + k].view_as(p)}
        self._online().mark_dirty()
        self._target().mark_dirty()
