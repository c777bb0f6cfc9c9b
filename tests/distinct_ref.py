"""CPU restatement of distinct per-agent networks (mac: distinct): agent slot i acts with DRQN i at every batch size
(the intent of src/marl/controllers/distinct_agents_controller.py; at batch_size 1 also what the reference computes,
pinned to its golden by tests/test_distinct.py). The oracle of tests/test_gpu_distinct.py and
tests/test_gpu_distinct_learner.py. Plain torch ops, fp32 by default, float64 when parameters and inputs are cast
(strictly more precise than the kernels). The cell is oracle/learner_ref.py's drqn_forward.

QLearner.train over N networks is oracle/learner_ref.py's QLearnerRef with the MAC unroll swapped for the per-agent
one (DistinctLearnerRef): masks, double-Q targets, mixers, loss, clip and RMSprop are the pinned restatement's, and
every network's parameters are in the optimiser (the reference's parameters() returns []).
"""
import numpy as np
import torch

import learner_ref as LR

AGENT_KEYS = LR.AGENT_KEYS


def agent_params(i, d_in, hidden, n_actions, seed, fc2_scale=1.0):
    """DRQN parameters of network ``i`` drawn with numpy (the same on every host and torch build) in torch's default
    ranges U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)), from a stream of its own per (seed, i): different weights per
    agent. fc2 times ``fc2_scale``. state_dict keys in order, float32 arrays."""
    rng = np.random.RandomState(1000 * seed + 7 * i + 1)
    u = lambda bound, *shape: rng.uniform(-bound, bound, size=shape).astype(np.float32)  # noqa: E731
    k1, kh = 1.0 / np.sqrt(d_in), 1.0 / np.sqrt(hidden)
    s = np.float32(fc2_scale)
    H = hidden
    return {"fc1.weight": u(k1, H, d_in), "fc1.bias": u(k1, H), "gru.weight_ih": u(kh, 3 * H, H),
            "gru.weight_hh": u(kh, 3 * H, H), "gru.bias_ih": u(kh, 3 * H), "gru.bias_hh": u(kh, 3 * H),
            "fc2.weight": u(kh, n_actions, H) * s, "fc2.bias": u(kh, n_actions) * s}


def all_agent_params(N, d_in, hidden, n_actions, seed, fc2_scale=1.0):
    return [agent_params(i, d_in, hidden, n_actions, seed, fc2_scale) for i in range(N)]


def load_agents(mac, params):
    """Load per-agent state dicts (arrays or tensors) into a DistinctMAC's networks."""
    for a, p in zip(mac.agents, params):
        a.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in p.items()})


def build_inputs(batch, t, last_action=True):
    """distinct_agents_controller.py:82-95: [obs_t | onehot(a_{t-1})] as [B, N, d_in] (no agent id)."""
    parts = [batch["obs"][:, t]]
    if last_action:
        oh = batch["actions_onehot"]
        parts.append(torch.zeros_like(oh[:, t]) if t == 0 else oh[:, t - 1])
    return torch.cat(parts, dim=2)


def mac_unroll(ps, batch, T=None, h0=None, last_action=True):
    """DistinctMAC.forward over t = 0..T-1 with network i for agent slot i -> (Q [B, T, N, A], h [B, N, H]).
    ``ps``: N state dicts. ``h0`` [B, N, H] (zeros by default)."""
    N = len(ps)
    B = batch["obs"].shape[0]
    T = batch["obs"].shape[1] if T is None else T
    dt = ps[0]["fc1.weight"].dtype
    H = ps[0]["gru.weight_hh"].shape[1]
    h = [torch.zeros(B, H, dtype=dt) if h0 is None else h0[:, i].to(dt) for i in range(N)]
    outs = []
    for t in range(T):
        x = build_inputs(batch, t, last_action).to(dt)
        qs = []
        for i in range(N):
            q, h[i] = LR.drqn_forward(ps[i], x[:, i], h[i])
            qs.append(q)
        outs.append(torch.stack(qs, dim=1))
    return torch.stack(outs, dim=1), torch.stack(h, dim=1)


def mac_step(ps, batch, t, h_in, last_action=True):
    """One step from ``h_in`` [B, N, H] -> (Q [B, N, A], h' [B, N, H])."""
    dt = ps[0]["fc1.weight"].dtype
    x = build_inputs(batch, t, last_action).to(dt)
    qs, hs = [], []
    for i, p in enumerate(ps):
        q, hn = LR.drqn_forward(p, x[:, i], h_in[:, i].to(dt))
        qs.append(q)
        hs.append(hn)
    return torch.stack(qs, dim=1), torch.stack(hs, dim=1)


def mac_params(mac, dtype=None):
    ps = [{k: v.detach().cpu() for k, v in a.state_dict().items()} for a in mac.agents]
    return ps if dtype is None else [{k: v.to(dtype) for k, v in p.items()} for p in ps]


def oracle_q(mac, tb, N, T, dtype=None):
    """helpers.oracle_q for a DistinctMAC: Q [B, T, N, A] along a recorded batch with the MAC's N parameter sets."""
    ps = mac_params(mac, dtype)
    assert len(ps) == N
    tb = {k: tb[k] for k in ("obs", "actions_onehot")}
    if dtype is not None:
        tb = {k: v.to(dtype) for k, v in tb.items()}
    with torch.no_grad():
        return mac_unroll(ps, tb, T=T, last_action=bool(mac.args.obs_last_action))[0].numpy()


def _split(p, N):
    return [{k: p[f"{i}.{k}"] for k in AGENT_KEYS} for i in range(N)]


class DistinctLearnerRef(LR.QLearnerRef):
    """QLearner.train (q_learner.py:34-131) over N networks: QLearnerRef with its parameter dict holding
    "<i>.<key>" for every network (agent 0 first, named_parameters() order, then the mixer: the optimiser's order) and
    LR.mac_unroll replaced, for the duration of a call, by the per-agent unroll above."""

    def __init__(self, agent_params_list, mixer_params, args, dtype=torch.float32):
        flat = {f"{i}.{k}": p[k] for i, p in enumerate(agent_params_list) for k in AGENT_KEYS}
        super().__init__(flat, mixer_params, args, dtype=dtype)
        self.N = len(agent_params_list)

    def _train(self, batch, t_env, episode_num):
        saved = LR.mac_unroll
        N = self.N

        def unroll(p, b, n_agents, T=None, h0=None, last_action=True, agent_id=True):
            assert n_agents == N and not agent_id
            return mac_unroll(_split(p, N), b, T=T, last_action=last_action)

        LR.mac_unroll = unroll
        try:
            return super()._train(batch, t_env, episode_num)
        finally:
            LR.mac_unroll = saved

    def agent_states(self):
        return [{k: v.detach().clone() for k, v in p.items()} for p in _split(self.p, self.N)]

    def target_states(self):
        return _split(self.tp, self.N)


def learner_ref(agent_params_list, mixer_params, args, dtype=torch.float32):
    return DistinctLearnerRef(agent_params_list, mixer_params, args, dtype=dtype)
