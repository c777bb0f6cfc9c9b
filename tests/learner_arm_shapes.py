"""The fused learner's shape cases shared by tests/test_learner_dispatch.py (CPU: the dispatch of mlg_qlearner_train
is pinned through mlg_qlearner_describe), tests/test_gpu_learner_arms.py (GPU: oracle parity per dispatch arm) and
scripts/oracle_f64_distance.py (CPU: how far the fp32 oracle is from a float64 run of itself, the ORACLE_F64 table
below).

A case is (id, rnn_hidden_dim, dims, mixer kwargs on top of helpers.qmix_args(), arm, seed). ``dims`` is the name of a
plan that helpers.shape_plan resolves -- its (N, A, S, d_obs) then come from TeamsEnvSpec, so the table cannot drift
from the env -- or a synthetic (N, A, S, d_obs) tuple. ``arm`` is what mlg_qlearner_describe reports for the case's
cfg under the default environment: "<agent part> + <mixer part>" (include/maleague.h lists the names). ``seed`` seeds
the agent's and the mixer's CPU modules and the batch.

Every case runs with double_q on unless its kwargs say otherwise (the two ``-nodq`` cases).
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "id H dims mixer arm seed")

QMIX, VDN, IQL = {}, {"mixer": "vdn"}, {"mixer": None}
NODQ = {"double_q": False}

CASES = [
    # the split QMIX path (rec4_mixpre_kernel<H> + mix_td2_kernel<64, 32>): 1 / 2 / 4 mixer tiles per workgroup
    Case("split-h32-2v2", 32, "2v2", QMIX, "h32/bwd-split/q1 + qmix-split", 11),
    Case("split-h128-4v4", 128, "4v4", QMIX, "h128/bwd-split/q1 + qmix-split", 11),
    Case("split-h64-1v1", 64, "1v1", QMIX, "h64/bwd-fused/q1 + qmix-split", 11),       # N = 1, R = 5 agent rows
    Case("split-h64-3v3", 64, "small", QMIX, "h64/bwd-fused/q1 + qmix-split", 11),
    Case("split-at-bounds", 64, (8, 16, 64, 23), QMIX, "h64/bwd-fused/q1 + qmix-split", 11),
    # the three bounds of the fast side crossed one at a time, then real plans
    Case("generic-n9", 64, (9, 16, 64, 23), QMIX, "h64/bwd-fused/q1 + qmix-generic", 11),
    Case("generic-n9-nodq", 64, (9, 16, 64, 23), NODQ, "h64/bwd-fused/q1 + qmix-generic", 11),
    Case("generic-a17", 64, (8, 17, 64, 23), QMIX, "h64/bwd-fused/q2 + qmix-generic", 11),
    Case("generic-s65", 64, (8, 16, 65, 23), QMIX, "h64/bwd-fused/q1 + qmix-generic", 11),
    Case("generic-h64-6v6", 64, "6v6", QMIX, "h64/bwd-fused/q2 + qmix-generic", 11),
    Case("generic-h128-9v9", 128, "9v9", QMIX, "h128/bwd-split/q2 + qmix-generic", 11),
    Case("generic-h32-large", 32, "large", QMIX, "h32/bwd-split/q4 + qmix-generic", 11),
    Case("generic-h64-32v32", 64, "32v32", QMIX, "h64/bwd-fused/q5 + qmix-generic", 11),  # N = MAXN
    Case("maxa-h128", 128, (2, 96, 20, 23), QMIX, "h128/bwd-split/q6 + qmix-generic", 11),  # A = MLG_BWD_MAXA
    Case("vdn-fast-h32-3v3", 32, "small", VDN, "h32/bwd-split/q1 + vdn-fast", 11),
    Case("vdn-fast-h128-2v2", 128, "2v2", VDN, "h128/bwd-split/q1 + vdn-fast", 11),
    Case("vdn-h64-7v7", 64, "7v7", VDN, "h64/bwd-fused/q2 + vdn", 11),
    Case("vdn-h64-7v7-nodq", 64, "7v7", dict(VDN, **NODQ), "h64/bwd-fused/q2 + vdn", 11),
    Case("vdn-h128-17v17", 128, "17v17", VDN, "h128/bwd-split/q3 + vdn", 11),
    Case("vdn-h32-9v9", 32, "9v9", VDN, "h32/bwd-split/q2 + vdn", 11),
    Case("iql-h128-2v2", 128, "2v2", IQL, "h128/bwd-split/q1 + iql", 11),
    Case("iql-h64-13v13", 64, "13v13", IQL, "h64/bwd-fused/q2 + iql", 11),
    Case("h1-e32-h128-7v7", 128, "7v7", {"hypernet_layers": 1}, "h128/bwd-split/q2 + qmix1-e32", 11),
    Case("he32-e16-h32-13v13", 32, "13v13", {"mixing_embed_dim": 16, "hypernet_embed": 32},
         "h32/bwd-split/q2 + qmix-he32-e16", 11),
]
IDS = [c.id for c in CASES]

# (H, mixer part) pairs the earlier learner suites run against the oracle or a golden: the default shape (goldens of
# test_gpu_learner.py, qmix / vdn / MLG_MIX_GENERIC), TRAJ (H = 64) and WIDE_CASES (H = 32) of
# test_gpu_learner_shapes.py
ARMS_COVERED_ELSEWHERE = {
    (64, "qmix-split"), (64, "qmix-generic"), (64, "vdn-fast"), (64, "iql"), (64, "qmix1-e32"), (64, "qmix1-e64"),
    (64, "qmix-he32-e16"), (64, "qmix-he128-e64"), (64, "qmix-he128-e32"), (64, "qmix-he64-e16"),
    (32, "iql"), (32, "qmix1-e16"), (32, "qmix-he128-e64"),
}

# case -> (largest relative distance of a statistic over the three calls, largest absolute distance of a parameter
# after them, largest distance of a first-call gradient tensor before the clip relative to max(1, max|g|) of that
# tensor, the first call's grad_norm) between the fp32 oracle and the same oracle in float64: measured on the CPU by
# scripts/oracle_f64_distance.py, also in profiles/learner_shapes/README.md. A bound of the GPU tests is the project's
# usual one, or ten times the distance here where that is larger.
ORACLE_F64 = {
    "split-h32-2v2": (2.04e-07, 3.84e-07, 1.94e-07, 13.02),
    "split-h128-4v4": (6.90e-07, 9.44e-07, 2.07e-07, 7.853),
    "split-h64-1v1": (9.51e-08, 7.45e-07, 2.23e-07, 9.974),
    "split-h64-3v3": (6.02e-07, 6.55e-07, 2.27e-07, 16.75),
    "split-at-bounds": (4.60e-07, 9.73e-07, 3.20e-07, 18.97),
    "generic-n9": (8.91e-07, 8.30e-07, 2.20e-07, 24.29),
    "generic-n9-nodq": (8.09e-07, 8.31e-07, 2.20e-07, 24.29),
    "generic-a17": (5.87e-07, 8.06e-07, 3.04e-07, 19.17),
    "generic-s65": (5.12e-07, 4.52e-07, 2.91e-07, 18.61),
    "generic-h64-6v6": (1.36e-07, 1.12e-06, 3.29e-07, 17.41),
    "generic-h128-9v9": (2.07e-07, 1.00e-06, 2.76e-07, 16.59),
    "generic-h32-large": (2.93e-07, 1.27e-06, 4.97e-07, 85.5),
    "generic-h64-32v32": (4.05e-07, 8.48e-07, 5.05e-07, 209),
    "maxa-h128": (5.98e-07, 2.82e-06, 3.45e-07, 6.64),
    "vdn-fast-h32-3v3": (2.52e-07, 9.74e-08, 3.35e-08, 1.798),
    "vdn-fast-h128-2v2": (7.82e-07, 1.85e-07, 4.51e-08, 1.644),
    "vdn-h64-7v7": (1.50e-07, 1.55e-07, 8.14e-08, 8.618),
    "vdn-h64-7v7-nodq": (2.25e-07, 1.62e-07, 8.14e-08, 8.618),
    "vdn-h128-17v17": (1.49e-07, 4.83e-07, 1.31e-07, 32.17),
    "vdn-h32-9v9": (1.57e-07, 5.14e-07, 1.01e-07, 8.759),
    "iql-h128-2v2": (4.56e-07, 1.59e-07, 1.07e-08, 0.7773),
    "iql-h64-13v13": (1.16e-06, 7.09e-08, 3.77e-09, 0.2849),
    "h1-e32-h128-7v7": (4.84e-07, 5.31e-07, 4.19e-07, 284.1),
    "he32-e16-h32-13v13": (3.14e-07, 1.54e-06, 4.03e-07, 14.12),
}
STAT_RTOL, STAT_ATOL, PARAM_ATOL, GRAD_RTOL = 2e-4, 1e-6, 5e-5, 1e-4  # the project's bounds against the oracle


def bounds(cid):
    """(statistic rtol, parameter atol, gradient bound relative to max(1, max|g_ref|) per tensor): the project's, or
    ten times the oracle's own fp32 distance where that is larger (nowhere, with the figures above)."""
    s, p, g, _ = ORACLE_F64[cid]
    return max(STAT_RTOL, 10 * s), max(PARAM_ATOL, 10 * p), max(GRAD_RTOL, 10 * g)


def clips(cid, clip=10.0):
    """Whether the case's first call clips its gradient (float64 oracle)."""
    return ORACLE_F64[cid][3] > clip

B, T_STORED = 5, 8
LENS = (6, 5, 3, 2, 2)       # filled prefixes: max_t_filled = 6, two stored steps lie past it
T_FILLED = max(LENS)         # the learner trains on transitions 0 .. T_FILLED - 2: 5 x 5 = 25 mixer rows, two 16-row
                             # tiles with the second partial, of the 5 x 7 = 35 (three tiles) the stored length plans
TERMINATED = (0, 2, 3)       # episodes whose last filled step carries `terminated`
CALLS = [(0, 0), (0, 100), (0, 200)]  # target == online; stale target; stale target, ends with the sync


def case(cid):
    return next(c for c in CASES if c.id == cid)


def mixer_part(arm):
    return arm.split(" + ")[1]


def plan_dims(plan):
    """(N, A, S, d_obs) of a plan name, from the env's own spec."""
    from helpers import shape_plan
    from maleague.envs.teams_env import TeamsEnvSpec
    info = TeamsEnvSpec.from_env_args({"match_build_plan": shape_plan(plan), "grid_size": 20,
                                       "stochastic_spawns": True, "episode_limit": 20}).env_info()
    return info["n_agents"], info["n_actions"], info["state_shape"], info["obs_shape"]


def dims(c):
    return plan_dims(c.dims) if isinstance(c.dims, str) else tuple(c.dims)


def case_args(c, device="cuda"):
    from helpers import qmix_args
    N, A, S, _ = dims(c)
    return qmix_args(n_agents=N, n_actions=A, state_shape=S, rnn_hidden_dim=c.H, device=device, **c.mixer)


def learner_cfg(args, d_obs, B=B, T=T_FILLED):
    """The MlgLearnerCfg QLearner._cfg builds for ``args`` (no learner, no GPU)."""
    from maleague import _native
    mixer = {"qmix": 2, "vdn": 1, None: 0}[args.mixer]
    return _native.MlgLearnerCfg(B=B, T=T, N=args.n_agents, A=args.n_actions, d_obs=d_obs, H=args.rnn_hidden_dim,
                                 S=int(args.state_shape), E=int(args.mixing_embed_dim), HE=int(args.hypernet_embed),
                                 hypernet_layers=int(args.hypernet_layers), mixer=mixer,
                                 double_q=int(bool(args.double_q)), obs_last_action=int(bool(args.obs_last_action)),
                                 obs_agent_id=int(bool(args.obs_agent_id)), gamma=float(args.gamma),
                                 lr=float(args.lr), optim_alpha=float(args.optim_alpha),
                                 optim_eps=float(args.optim_eps), grad_norm_clip=float(args.grad_norm_clip))


def describe(c):
    from maleague import _native
    return _native.qlearner_describe(learner_cfg(case_args(c, "cpu"), dims(c)[3]))


def arm_batch(N, A, S, d_obs, seed):
    """test_gpu_learner_shapes.wide_batch() for any dims (CPU tensors, scheme dtypes): B = 5 episodes of 8 stored
    steps with filled prefixes 6 / 5 / 3 / 2 / 2, `terminated` on the last filled step of episodes 0, 2 and 3. Every
    agent has an available action and takes one; about a fifth of the (b, t, n) rows have exactly one available
    action, as dead units do in real batches (the masked argmax and max then meet the -9999999 fill everywhere but
    there). The contents are random at every step, filled or not: nothing past an episode's end may reach a result."""
    import torch
    rs = np.random.RandomState(seed)
    T = T_STORED
    filled = np.zeros((B, T, 1), np.int64)
    term = np.zeros((B, T, 1), np.uint8)
    for b, f in enumerate(LENS):
        filled[b, :f] = 1
    for b in TERMINATED:
        term[b, LENS[b] - 1] = 1
    avail = (rs.rand(B, T, N, A) < 0.5).astype(np.int32)
    single = rs.rand(B, T, N) < 0.2
    keep = rs.randint(0, A, size=(B, T, N))
    avail[single] = 0
    np.put_along_axis(avail, keep[..., None], 1, axis=-1)  # the one action of a single row; one at least elsewhere
    actions = np.zeros((B, T, N, 1), np.int64)
    for idx in np.ndindex(B, T, N):
        actions[idx][0] = rs.choice(np.flatnonzero(avail[idx]))
    onehot = np.zeros((B, T, N, A), np.float32)
    np.put_along_axis(onehot, actions, 1.0, axis=-1)
    out = {"state": rs.randn(B, T, S).astype(np.float32), "obs": rs.randn(B, T, N, d_obs).astype(np.float32),
           "actions": actions, "avail_actions": avail, "reward": rs.randn(B, T, 1).astype(np.float32),
           "terminated": term, "actions_onehot": onehot, "filled": filled}
    return {k: torch.from_numpy(v) for k, v in out.items()}


def case_batch(c):
    return arm_batch(*dims(c), seed=c.seed + 100)


def oracle_batch(tb):
    """The sample the reference trains on: truncated to max_t_filled."""
    return {k: v[:, :T_FILLED].clone() for k, v in tb.items()}


def case_weights(c, args):
    """(agent state_dict, mixer state_dict or None) of seeded CPU modules."""
    from test_gpu_learner_shapes import agent_state, mixer_state
    return (agent_state(args, dims(c)[3], seed=c.seed),
            mixer_state(args, seed=c.seed + 8) if args.mixer == "qmix" else None)


def mask_sum(tb):
    """sum of mask = filled[:, :-1] * (1 - terminated shifted) over the truncated sample, in numpy."""
    f = tb["filled"][:, :T_FILLED - 1, 0].numpy().astype(np.float64)
    t = tb["terminated"][:, :T_FILLED - 1, 0].numpy().astype(np.float64)
    m = f.copy()
    m[:, 1:] *= 1 - t[:, :-1]
    return float(m.sum())


# ---- the reference's golden off the default agent shape (tests/golden/make_learner_shapes_golden.py) ----------------
GOLDEN_9V9 = ("qlearner_qmix_9v9_h128.npz", "qlearner_qmix_9v9_h128_after.npz")
GOLDEN_9V9_KW = dict(n_agents=9, n_actions=23, state_shape=108, rnn_hidden_dim=128)  # d_obs 144: the 9v9 plan's dims


class SplitGolden:
    """The two files of the 9v9 / H = 128 golden read as one npz (``files``, ``[]``). The second file holds no third
    copy of the agent: it records whether the reference's target agent equalled its online agent after the last call
    (``target_is_online``), and p3.target_agent.* then reads p3.agent.*."""

    def __init__(self, golden):
        self.parts = [golden(n) for n in GOLDEN_9V9]
        assert bool(self.parts[1]["target_is_online"])
        self.files = [k for p in self.parts for k in p.files]

    def __getitem__(self, k):
        if k.startswith("p3.target_agent."):
            k = "p3.agent." + k[len("p3.target_agent."):]
        return next(p for p in self.parts if k in p.files)[k]
