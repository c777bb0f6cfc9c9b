"""Cases of the prioritized-replay tests, shared by tests/test_per.py (CPU: the near-tie condition on the sampling
inputs, the dispatch names) and tests/test_gpu_per.py (GPU parity).

Sampling cases: live slots 1 / 31 / 64 / 65 / 1000 / 5000 / 65536 (one lane, a partial wave, one wave, one wave and a
slot, a partial 1024-slot chunk, several chunks with the scan still in LDS, 64 chunks with the scan in the workspace)
x batch 1 / 32 / 64 x priorities flat (every slot at the initial maximum 1), skewed (one slot holds 90 % of the mass, the
rest uniform in [0.5, 1.5)) and partial (the buffer holds 37 more slots than are live, filled with 1e6: they must not
take part). The seed of a case is fixed here; test_per.py checks on the CPU that no draw of the float64 oracle lies
within 1e-9 of the total from a cumulative boundary, so that the device's fp64 scan, which adds in another order, must
pick the same slot for every draw: no draw is excluded on the GPU.

Learner cases: one per TD site and agent kind on learner_arm_shapes.arm_batch (B = 5 episodes of 8 stored steps, filled
prefixes 6 / 5 / 3 / 2 / 2: 35 mixer rows cross two 16-row tile boundaries, episode boundaries fall inside tiles, the
last two episodes are a single transition); the distinct-network case uses distinct_learner_shapes.batch (prefixes
6 / 5 / 0 / 3 / 1: a never-filled episode, whose error is 0).
"""
import functools
from collections import namedtuple

import numpy as np

import learner_arm_shapes as LA

LIVE = (1, 31, 64, 65, 1000, 5000, 65536)
BATCHES = (1, 32, 64)
KINDS = ("flat", "skewed", "partial")
SAMPLE_IDS = [f"{kind}-n{n}-b{B}" for kind in KINDS for n in LIVE for B in BATCHES]
NEAR_TIE = 1e-9
BETA = 0.4


@functools.lru_cache(maxsize=None)
def sample_case(sid):
    """-> (priorities float32 [capacity], n_live, B, seed, draw)"""
    kind, n, B = sid.split("-")
    n, B = int(n[1:]), int(B[1:])
    k = SAMPLE_IDS.index(sid)
    rs = np.random.RandomState(500 + k)
    if kind == "flat":
        p = np.ones(n, np.float32)
    elif kind == "skewed":
        p = rs.uniform(0.5, 1.5, size=n).astype(np.float32)
        if n > 1:
            heavy = rs.randint(0, n)
            rest = float(p.astype(np.float64).sum() - p[heavy])
            p[heavy] = np.float32(9.0 * rest)
    else:
        p = np.concatenate([rs.uniform(0.1, 2.0, size=n), np.full(37, 1e6)]).astype(np.float32)
    return p, n, B, 1000 + k, 3 + k % 5


# ---- learner cases: (id, kind, learner_arm_shapes.Case, environment) -------------------------------------------------
PCase = namedtuple("PCase", "id kind case env")
H1 = {"hypernet_layers": 1}
HE32_E16 = {"mixing_embed_dim": 16, "hypernet_embed": 32}
LEARNER_CASES = [
    PCase("qmix-split", "rnn", LA.Case("per-split", 64, "small", LA.QMIX, "h64/bwd-fused/q1 + qmix-split", 11), {}),
    PCase("qmix-generic", "rnn", LA.Case("per-generic", 64, "small", LA.QMIX, "h64/bwd-fused/q1 + qmix-generic", 11),
          {"MLG_MIX_GENERIC": "1"}),
    PCase("qmix1", "rnn", LA.Case("per-qmix1", 64, "small", H1, "h64/bwd-fused/q1 + qmix1-e32", 11), {}),
    PCase("qmix-he32-e16", "rnn", LA.Case("per-widths", 32, "2v2", HE32_E16, "h32/bwd-split/q1 + qmix-he32-e16", 11), {}),
    PCase("vdn", "rnn", LA.Case("per-vdn", 32, "small", LA.VDN, "h32/bwd-split/q1 + vdn-fast", 11), {}),
    PCase("iql", "rnn", LA.Case("per-iql", 64, "2v2", LA.IQL, "h64/bwd-fused/q1 + iql", 11), {}),
    PCase("dqn", "dqn", LA.Case("per-dqn", 64, "small", LA.QMIX, "ff-h64/q1 + qmix-generic", 11), {}),
    PCase("distinct", "distinct", LA.Case("per-dx", 32, (3, 11, 36, 23), LA.QMIX,
                                          "dx-h32/bwd-split/q1 + qmix-generic", 11), {}),
]
LEARNER_IDS = [c.id for c in LEARNER_CASES]
# the TD site behind each case (learner.hip): one case at least per site
TD_SITE = {"qmix-split": "mix_td2_kernel", "qmix-generic": "mix_td_kernel", "qmix1": "mix_td1_kernel",
           "qmix-he32-e16": "mix_td_kernel", "vdn": "mix_td_kernel", "iql": "iql_td_kernel", "dqn": "mix_td_kernel",
           "distinct": "mix_td_kernel"}


def learner_case(pid):
    return next(c for c in LEARNER_CASES if c.id == pid)


def case_args(pc, device="cuda"):
    c = pc.case
    if pc.kind == "distinct":
        from helpers import qmix_args
        N, A, S, _ = LA.dims(c)
        return qmix_args(n_agents=N, n_actions=A, state_shape=S, rnn_hidden_dim=c.H, obs_agent_id=False, mac="distinct",
                         device=device, **c.mixer)
    args = LA.case_args(c, device)
    if pc.kind == "dqn":
        args.agent = "dqn"
    return args


def learner_cfg(pc, per=0):
    """The MlgLearnerCfg of the case at the truncated length (no learner, no GPU)."""
    cfg = LA.learner_cfg(case_args(pc, "cpu"), LA.dims(pc.case)[3])
    cfg.agent = int(pc.kind == "dqn")
    cfg.distinct = int(pc.kind == "distinct")
    cfg.per = per
    return cfg


@functools.lru_cache(maxsize=None)
def learner_inputs(pid):
    """-> (case, args, agent parameters (a list of N for the distinct case), mixer parameters or None, batch)"""
    from test_gpu_learner_shapes import agent_state, mixer_state
    pc = learner_case(pid)
    c = pc.case
    args = case_args(pc)
    N, A, S, d_obs = LA.dims(c)
    mixer0 = mixer_state(args, seed=c.seed + 8) if args.mixer == "qmix" else None
    if pc.kind == "distinct":
        import distinct_learner_shapes as DLS
        import distinct_ref as DR
        agent0 = DR.all_agent_params(N, d_obs + A, c.H, A, c.seed)
        tb = DLS.batch(N, A, S, d_obs, LA.B, seed=c.seed + 100)
    else:
        if pc.kind == "dqn":
            import dqn_ref
            agent0 = dqn_ref.agent_state(args, d_obs, seed=c.seed)
        else:
            agent0 = agent_state(args, d_obs, seed=c.seed)
        tb = LA.case_batch(c)
    return pc, args, agent0, mixer0, tb


def is_weight(pid):
    """Random importance weights in (0.1, 1], the largest exactly 1 as mlg_per_sample's are."""
    w = np.random.RandomState(900 + LEARNER_IDS.index(pid)).uniform(0.1, 1.0, size=LA.B).astype(np.float32)
    w[int(np.argmax(w))] = 1.0
    return w


def oracle_class(pc):
    import learner_ref as LR
    import per_ref
    if pc.kind == "dqn":
        import dqn_ref
        return per_ref.per_ref_class(dqn_ref.DQNLearnerRef)
    if pc.kind == "distinct":
        import distinct_ref as DR
        return per_ref.per_ref_class(DR.DistinctLearnerRef)
    return per_ref.per_ref_class(LR.QLearnerRef)


@functools.lru_cache(maxsize=None)
def oracle_f64(pid):
    """The float64 weighted oracle's first call on the sample truncated to max_t_filled: (gradients before the clip in
    flat parameter order, td_abs [B], statistics)."""
    import torch

    import learner_ref as LR
    pc, args, agent0, mixer0, tb = learner_inputs(pid)
    T = int(tb["filled"].sum(dim=(1, 2)).max())
    ob = {k: v[:, :T].clone() for k, v in tb.items()}
    ref = oracle_class(pc)(agent0, mixer0, LR.clone_args(args, device="cpu"), dtype=torch.float64)
    ref.is_weight = is_weight(pid)
    stats = ref.train(ob, 0, 0)
    return [g.clone() for g in ref.last_grads], ref.last_td_abs.clone(), stats
