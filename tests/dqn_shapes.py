"""The feed-forward rollout cases shared by tests/test_dqn.py (CPU: the dispatch table of mlg_rollout_ff is pinned
through mlg_rollout_ff_describe), tests/test_gpu_dqn.py (GPU: oracle parity per dispatch arm) and
scripts/dqn_near_ties.py (CPU: the near-tie share of the float64 oracle alone).

A case is (id, rnn_hidden_dim, plan, arm, seed, fc2_scale): ``plan`` is a name helpers.shape_plan resolves, ``arm``
what mlg_rollout_ff_describe reports for it, ``seed`` the stepper seed (env keys, epsilon stream) and the seed of the
agent weights (dqn_ref.agent_params: numpy, so the CPU script plays the same weights), ``fc2_scale`` a factor on fc2
(1.0 everywhere so far; the knob tests/coma_shapes.py uses to move a case off a tie-heavy regime).

Seeds follow the rule of tests/rollout_shapes.py: the GPU checker accepts a greedy pick that differs from the oracle's
argmax only at a near tie (top-two masked Q within Q_TOL = 1e-4) and caps the accepted share at 1 % of the greedy
picks; a (seed, fc2_scale) is kept only if the float64 oracle alone, rolled out on the CPU over the oracle env at the
same B and episode limit (test-mode run of episode 0, train-mode run of episode 1 at epsilon 0.525), sees at most
0.5 % of its greedy picks at such a gap. scripts/dqn_near_ties.py counts it; the share is written beside each case.

Arms. The weight image without the GRU blocks is small, so the LDS arm takes every shape up to 24v24 at H = 64, every
shape at H = 32 and up to 13v13 at H = 128; the global arm is reached from 14v14 on at H = 128 and from 25v25 on at
H = 64. No admitted shape reaches ff-global/tpw1: one tile per wave means at most 8 agents, whose image fits LDS at
every supported H, and the entry point has no variable that forces the global arm. It has no case.
"""
B, EPISODE_LIMIT = 37, 30
T_ENV = 25000
EPS = max(0.05, 1.0 - 0.95 / 50000 * T_ENV)  # 0.525, the schedule's value at T_ENV

# (id, H, plan, arm, seed, fc2_scale)                                        oracle near-tie share (picks)
CASES = [
    ("ff-lds-h64-3v3", 64, "small", "ff-lds/tpw1", 11, 1.0),             # 0.039 % (2 / 5109)
    ("ff-lds-h32-5v5", 32, "medium_1h_4t", "ff-lds/tpw1", 11, 1.0),      # 0.118 % (10 / 8451)
    ("ff-lds-h128-3v3", 128, "small", "ff-lds/tpw1", 11, 1.0),           # 0.254 % (13 / 5109)
    ("ff-lds-h64-9v9", 64, "9v9", "ff-lds/tpw2", 11, 1.0),               # 0.112 % (17 / 15192)
    ("ff-lds-h32-17v17", 32, "17v17", "ff-lds/tpw3", 11, 1.0),           # 0.115 % (33 / 28658)
    ("ff-lds-h32-25v25", 32, "25v25", "ff-lds/tpw4", 11, 1.0),           # 0.050 % (21 / 42181)
    ("ff-global-h128-14v14", 128, "14v14", "ff-global/tpw2", 11, 1.0),   # 0.157 % (37 / 23607)
    ("ff-global-h128-17v17", 128, "17v17", "ff-global/tpw3", 11, 1.0),   # 0.042 % (12 / 28658)
    ("ff-global-h64-25v25", 64, "25v25", "ff-global/tpw4", 11, 1.0),     # 0.114 % (48 / 42181)
]

# one case per K for the ring-mode run
RING_CASES = ["ff-lds-h64-3v3", "ff-lds-h64-9v9", "ff-lds-h32-17v17", "ff-global-h64-25v25"]


def case(cid):
    return next(c for c in CASES if c[0] == cid)


# ---- the fused learner with agent = 1 (mlg_qlearner_train's feed-forward branch) -------------------------------------
# learner_arm_shapes.Case rows: (id, rnn_hidden_dim, dims, mixer kwargs, arm, seed). ``arm`` is what
# mlg_qlearner_describe reports with agent = 1: "ff-h{H}/q{k} + <mixer part>". QMIX at the default widths runs
# qmix-generic for every shape: the split form's hypernet forward rides in the recurrence launch, which does not exist
# here. Batches are learner_arm_shapes.arm_batch's (B = 5, filled prefixes 6 / 5 / 3 / 2 / 2, two stored steps past
# max_t_filled, terminated flags on three episodes). H 32 / 64 / 128, N = 1 / 5 / 17, IQL, VDN (fast and generic),
# QMIX default, one-layer and another width.
def _learner_cases():
    from learner_arm_shapes import IQL, QMIX, VDN, Case
    return [
        Case("ff-qmix-h64-5v5", 64, "medium_1h_4t", QMIX, "ff-h64/q1 + qmix-generic", 11),
        Case("ff-qmix-h32-1v1", 32, "1v1", QMIX, "ff-h32/q1 + qmix-generic", 11),          # N = 1
        Case("ff-qmix-h128-17v17", 128, "17v17", QMIX, "ff-h128/q3 + qmix-generic", 11),   # N = 17, three action tiles
        Case("ff-vdn-h32-3v3", 32, "small", VDN, "ff-h32/q1 + vdn-fast", 11),
        Case("ff-vdn-h64-17v17", 64, "17v17", VDN, "ff-h64/q3 + vdn", 11),
        Case("ff-iql-h128-2v2", 128, "2v2", IQL, "ff-h128/q1 + iql", 11),
        Case("ff-h1-e32-h64-7v7", 64, "7v7", {"hypernet_layers": 1}, "ff-h64/q2 + qmix1-e32", 11),
        Case("ff-he32-e16-h32-5v5", 32, "medium_1h_4t", {"mixing_embed_dim": 16, "hypernet_embed": 32},
             "ff-h32/q1 + qmix-he32-e16", 11),
    ]


def learner_case(cid):
    return next(c for c in _learner_cases() if c.id == cid)


LEARNER_IDS = ["ff-qmix-h64-5v5", "ff-qmix-h32-1v1", "ff-qmix-h128-17v17", "ff-vdn-h32-3v3", "ff-vdn-h64-17v17",
               "ff-iql-h128-2v2", "ff-h1-e32-h64-7v7", "ff-he32-e16-h32-5v5"]


def learner_args(c, device="cuda"):
    import learner_arm_shapes as LA
    a = LA.case_args(c, device)
    a.agent = "dqn"
    return a


def learner_cfg(c, device="cpu"):
    import learner_arm_shapes as LA
    cfg = LA.learner_cfg(learner_args(c, device), LA.dims(c)[3])
    cfg.agent = 1
    return cfg
