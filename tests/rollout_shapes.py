"""The rollout shape cases shared by tests/test_rollout_dispatch.py (CPU: the dispatch table is pinned),
tests/test_gpu_rollout_shapes.py (GPU: oracle parity per dispatch arm) and scripts/rollout_near_ties.py (CPU: the
near-tie share of the float64 oracle alone, the seed selection rule below).

A case is (id, rnn_hidden_dim, plan, arm, seed): ``plan`` is a name helpers.shape_plan resolves, ``arm`` the kernel
mlg_rollout_describe reports for it under the default environment, ``seed`` the stepper seed (env keys, epsilon
stream) and the seed of the agent weights (agent_params: numpy, so the CPU script plays the same weights).

Seeds. The checkers accept a greedy pick that differs from the oracle's argmax only at a near tie (top-two masked Q
within Q_TOL = 1e-4), and the GPU tests cap the accepted share at 1 % of the greedy picks so that the escape cannot
hide a wrong kernel. That cap is a condition on the case, so a seed is kept only if the float64 oracle alone, rolled
out over the oracle env (B = 37, episode_limit 30, the test-mode run of episode 0 and the train-mode run of episode 1
at epsilon 0.525 -- self-play: 0.525 / 0.3 -- as the GPU test runs them), sees at most 0.5 % of its greedy picks at
such a gap. The share scripts/rollout_near_ties.py counted is written beside each case.
"""
import numpy as np

B, EPISODE_LIMIT = 37, 30
T_ENV = 25000
EPS_HOME = max(0.05, 1.0 - 0.95 / 50000 * T_ENV)  # 0.525, the schedule's value at T_ENV
EPS_AWAY = 0.3

# mlg_rollout: (id, H, plan, arm under the default environment, seed)       oracle near-tie share (picks)
ROLLOUT_CASES = [
    ("v7-4v4", 64, "4v4", "v7", 11),                              # 0.000 % (0 / 6790)
    ("v7-2v2", 64, "2v2", "v7", 11),                              # 0.059 % (2 / 3388)
    ("v2-default-5v7", 64, "5v7", "v2", 11),                      # 0.192 % (16 / 8318)
    ("v2-h32-5v5", 32, "medium_1h_4t", "v2", 11),                 # 0.012 % (1 / 8451)
    ("v2-h32-7v7", 32, "7v7", "v2", 11),                          # 0.008 % (1 / 11812)
    ("v1-h128-3v3", 128, "small", "v1-global/tpw1", 11),          # 0.196 % (10 / 5109)
    ("v1-h128-9v9", 128, "9v9", "v1-global/tpw2", 11),            # 0.132 % (20 / 15192)
    ("v1-h64-9v9", 64, "9v9", "v1-global/tpw2", 11),              # 0.151 % (23 / 15192)
    ("v1-h32-9v9", 32, "9v9", "v1-lds/tpw2", 11),                 # 0.105 % (16 / 15192)
    ("v1-large", 64, "large", "v1-global/tpw4", 11),              # 0.199 % (84 / 42181)
    ("policy-first-3v5", 64, "3v5", "v7", 11),                    # 0.224 % (11 / 4900)
    # the v1 arms the default environment reaches that the rows above do not
    ("v1-h64-7v7", 64, "7v7", "v1-lds/tpw1", 11),                 # 0.085 % (10 / 11812)
    ("v1-h32-17v17", 32, "17v17", "v1-lds/tpw3", 11),             # 0.073 % (21 / 28658)
    ("v1-h32-large", 32, "large", "v1-lds/tpw4", 11),             # 0.239 % (101 / 42181)
    ("v1-h64-17v17", 64, "17v17", "v1-global/tpw3", 11),          # 0.077 % (22 / 28658)
]

# mlg_rollout_selfplay (both plan teams policy-controlled)
SELFPLAY_CASES = [
    ("sp7-4v4", 64, "4v4", "sp7", 11),                            # 0.014 % (2 / 14579)
    ("sp2-h32-5v5", 32, "medium_1h_4t", "sp2", 11),               # 0.110 % (20 / 18188)
    ("sp2-h32-3v3", 32, "small", "sp2", 11),                      # 0.018 % (2 / 10966)
    ("v1sp-h128-3v3", 128, "small", "v1-global/tpw1", 11),        # 0.073 % (8 / 10966)
    ("v1sp-h64-7v7", 64, "7v7", "v1-global/tpw2", 11),            # 0.075 % (19 / 25451)
    ("v1sp-h64-9v9", 64, "9v9", "v1-global/tpw3", 11),            # 0.186 % (61 / 32741)
    ("v1sp-h32-13v13", 32, "13v13", "v1-global/tpw4", 11),        # 0.114 % (54 / 47262)
]

# arms of the default environment the earlier suites already check against the oracle at H = 64, 5v5 / 3v3
# (test_rollout_teacher_forced_parity, test_selfplay_rollout_parity)
ARMS_COVERED_ELSEWHERE = {"v7-static", "sp8"}


def case(cases, cid):
    return next(c for c in cases if c[0] == cid)


def agent_params(d_in, hidden, n_actions, seed):
    """DRQN parameters drawn with numpy (the same on every host and torch build) in torch's default ranges:
    U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for the linear layers, U(-1 / sqrt(H), 1 / sqrt(H)) for the GRU cell.
    state_dict keys of DRQNAgentNetwork, float32 arrays."""
    rng = np.random.RandomState(seed)
    u = lambda bound, *shape: rng.uniform(-bound, bound, size=shape).astype(np.float32)  # noqa: E731
    k1, kh = 1.0 / np.sqrt(d_in), 1.0 / np.sqrt(hidden)
    return {"fc1.weight": u(k1, hidden, d_in), "fc1.bias": u(k1, hidden),
            "gru.weight_ih": u(kh, 3 * hidden, hidden), "gru.weight_hh": u(kh, 3 * hidden, hidden),
            "gru.bias_ih": u(kh, 3 * hidden), "gru.bias_hh": u(kh, 3 * hidden),
            "fc2.weight": u(kh, n_actions, hidden), "fc2.bias": u(kh, n_actions)}


def side_seeds(seed, self_play):
    """Weight seeds of the policies of a case: one, or home and away."""
    return (seed, seed + 1000) if self_play else (seed,)
