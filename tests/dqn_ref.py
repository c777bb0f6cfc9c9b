"""CPU restatement of the feed-forward agent (agent: dqn) and of its BasicMAC unroll: the oracle of tests/test_dqn.py
(pinned to the reference's goldens there) and tests/test_gpu_dqn.py. Plain torch ops, fp32 by default, float64 when
the parameters and inputs are cast (strictly more precise than the kernels). Input building comes from
oracle/learner_ref.py.

QLearner.train over the feed-forward agent is oracle/learner_ref.py's QLearnerRef with the MAC unroll swapped for the
feed-forward one (DQNLearnerRef): masks, double-Q targets, mixers, loss, clip and RMSprop are the pinned restatement's.
"""
import numpy as np
import torch
import torch.nn.functional as F

import learner_ref as LR

AGENT_KEYS = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]


def dqn_forward(p, inputs):
    """src/marl/modules/agents/dqn_agent.py:34-37: fc2(relu(fc1(inputs)))."""
    return F.linear(F.relu(F.linear(inputs, p["fc1.weight"], p["fc1.bias"])), p["fc2.weight"], p["fc2.bias"])


def mac_unroll(p, batch, n_agents, T=None, last_action=True, agent_id=True, ts=None):
    """BasicMAC.forward over t = 0..T-1 (or the steps ``ts``) with a feed-forward agent -> [B, T, N, A]."""
    B = batch["obs"].shape[0]
    ts = range(batch["obs"].shape[1] if T is None else T) if ts is None else ts
    dt = p["fc1.weight"].dtype
    outs = []
    for t in ts:
        x = LR.build_inputs(batch, t, n_agents, last_action, agent_id).to(dt)
        outs.append(dqn_forward(p, x).view(B, n_agents, -1))
    return torch.stack(outs, dim=1)


def oracle_q(mac, tb, N, T, dtype=None):
    """helpers.oracle_q for a feed-forward MAC: Q [B, T, N, A] along a recorded batch with ``mac``'s parameters."""
    params = {k: v.detach().cpu() for k, v in mac.agent.state_dict().items()}
    tb = {k: tb[k] for k in ("obs", "actions_onehot")}
    if dtype is not None:
        params = {k: v.to(dtype) for k, v in params.items()}
        tb = {k: v.to(dtype) for k, v in tb.items()}
    with torch.no_grad():
        return mac_unroll(params, tb, N, T=T).numpy()


def agent_params(d_in, hidden, n_actions, seed, fc2_scale=1.0):
    """Feed-forward agent parameters drawn with numpy (the same on every host and torch build) in torch's default
    ranges U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)); fc2 times ``fc2_scale``. state_dict keys, float32 arrays."""
    rng = np.random.RandomState(seed)
    u = lambda bound, *shape: rng.uniform(-bound, bound, size=shape).astype(np.float32)  # noqa: E731
    k1, kh = 1.0 / np.sqrt(d_in), 1.0 / np.sqrt(hidden)
    s = np.float32(fc2_scale)
    return {"fc1.weight": u(k1, hidden, d_in), "fc1.bias": u(k1, hidden),
            "fc2.weight": u(kh, n_actions, hidden) * s, "fc2.bias": u(kh, n_actions) * s}


class DQNLearnerRef(LR.QLearnerRef):
    """QLearner.train (q_learner.py:34-131) over a feed-forward MAC: QLearnerRef._train with LR.mac_unroll replaced,
    for the duration of the call, by the feed-forward unroll above (same signature, no hidden state)."""

    def _train(self, batch, t_env, episode_num):
        saved = LR.mac_unroll
        LR.mac_unroll = lambda p, b, N, T=None, h0=None, last_action=True, agent_id=True: \
            (mac_unroll(p, b, N, T=T, last_action=last_action, agent_id=agent_id), None)
        try:
            return super()._train(batch, t_env, episode_num)
        finally:
            LR.mac_unroll = saved


def agent_state(args, d_obs, seed):
    """Seeded feed-forward agent parameters for ``args`` (torch tensors, state_dict keys)."""
    d_in = d_obs + (args.n_actions if args.obs_last_action else 0) + (args.n_agents if args.obs_agent_id else 0)
    return {k: torch.from_numpy(v) for k, v in agent_params(d_in, args.rnn_hidden_dim, args.n_actions, seed).items()}
