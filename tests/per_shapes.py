"""Cases, seeds and measured figures of the prioritized-replay parity pass off the fixture shapes of
tests/per_cases.py, shared by tests/test_per_shapes.py (CPU: the conditions on the float64 oracle alone),
tests/test_gpu_per_shapes.py (GPU parity), scripts/per_seed_search.py (CPU: the SAMPLE_SEEDS table) and
scripts/per_oracle_f64_distance.py (CPU: the ORACLE_F64 table). No GPU import.

1. mlg_per_sample at its own edges (replay.hip). Live slots 1024 / 1025 (the chunk carry of the scan: one whole
   1024-slot chunk, one chunk and a slot), 6144 / 6145 (kLdsSlots: the last count whose scan stays in LDS, the first in
   the workspace) and 2^20 (the documented maximum, 1024 chunks); draws 1024 / 1025 / 4096 (per_sample_kernel takes
   kDraws = 4 draws per thread: one whole pass, one pass and a draw, all four with the index field of mlg_ctr at its
   12-bit limit 4095), 64 and 1025 at 2^20 slots. 4096 draws are never paired with 2^20 slots: boundaries lie about
   total / n apart, so a case expects about 2e-9 n B near ties (8 there, at most 2.2 in the table below).
   Priorities: flat, skewed (per_cases'), zeros (about a third of the slots exactly 0, the last slot among them, slot 0
   not: reachable with per_eps = 0 and an episode whose error is 0). beta 0.4, and the clamp values 0 and 1 on a subset.
   The seed of a case's draws is SAMPLE_SEEDS', found on the CPU: the first seed from the case's base at which no draw of
   the float64 oracle lies within per_cases.NEAR_TIE (1e-9 of the total) of a cumulative boundary. No draw is excluded
   on the GPU.

2. The learner with per = 1 on every dispatch arm: the 24 cases of learner_arm_shapes.CASES, the 8 feed-forward cases of
   dqn_shapes and the 6 distinct-network cases of distinct_learner_shapes, each with its own batch and parameters and
   seeded weights in (0.1, 1], the largest exactly 1.

3. The time and batch axes of per_reduce_kernel (learner.hip; one wave per episode, lane l adds transitions l, l + 64,
   ...): REDUCE_CASES, at 2v2 / H 32.
"""
import functools
from collections import namedtuple

import numpy as np

import learner_arm_shapes as LA
import per_cases as PC

# ---- 1. sampling -------------------------------------------------------------------------------------------------------
MAX_SLOTS = 1 << 20
SCase = namedtuple("SCase", "id kind n B beta")


def _sid(kind, n, B, beta):
    return f"{kind}-n{n}-b{B}" + ("" if beta == PC.BETA else f"-beta{beta:g}")


SAMPLE_KINDS = ("flat", "skewed", "zeros")
SAMPLE_CASES = [SCase(_sid(k, n, B, PC.BETA), k, n, B, PC.BETA)
                for k in SAMPLE_KINDS for n in (1024, 1025, 6144, 6145) for B in (1024, 1025, 4096)]
SAMPLE_CASES += [SCase(_sid(k, MAX_SLOTS, 64, PC.BETA), k, MAX_SLOTS, 64, PC.BETA) for k in SAMPLE_KINDS]
SAMPLE_CASES += [SCase(_sid("flat", MAX_SLOTS, 1025, PC.BETA), "flat", MAX_SLOTS, 1025, PC.BETA)]
# the clamp values of beta: weights exactly 1 at beta = 0, the plain total / (n p) over its maximum at beta = 1
SAMPLE_CASES += [SCase(_sid(k, n, B, beta), k, n, B, beta)
                 for beta in (0.0, 1.0) for k, n, B in (("skewed", 1025, 1025), ("zeros", 6145, 4096))]
SAMPLE_IDS = [c.id for c in SAMPLE_CASES]

# case -> the seed of its draws: scripts/per_seed_search.py, the first seed from 3000 + 64 k (k the case's position) whose
# float64 margin exceeds per_cases.NEAR_TIE; the margin found is written beside it (relative to the total)
SAMPLE_SEEDS = {
    "flat-n1024-b1024": 3000,  # margin 6.69e-09, 1 tried
    "flat-n1024-b1025": 3064,  # margin 1.84e-07, 1 tried
    "flat-n1024-b4096": 3128,  # margin 2.45e-07, 1 tried
    "flat-n1025-b1024": 3192,  # margin 7.57e-07, 1 tried
    "flat-n1025-b1025": 3256,  # margin 2.45e-07, 1 tried
    "flat-n1025-b4096": 3320,  # margin 1.17e-07, 1 tried
    "flat-n6144-b1024": 3384,  # margin 3.05e-08, 1 tried
    "flat-n6144-b1025": 3448,  # margin 1.38e-09, 1 tried
    "flat-n6144-b4096": 3512,  # margin 2.77e-09, 1 tried
    "flat-n6145-b1024": 3576,  # margin 2.40e-07, 1 tried
    "flat-n6145-b1025": 3640,  # margin 5.58e-08, 1 tried
    "flat-n6145-b4096": 3704,  # margin 3.74e-08, 1 tried
    "skewed-n1024-b1024": 3768,  # margin 3.39e-07, 1 tried
    "skewed-n1024-b1025": 3833,  # margin 5.32e-07, 2 tried
    "skewed-n1024-b4096": 3896,  # margin 2.54e-08, 1 tried
    "skewed-n1025-b1024": 3960,  # margin 7.85e-07, 1 tried
    "skewed-n1025-b1025": 4024,  # margin 3.12e-07, 1 tried
    "skewed-n1025-b4096": 4088,  # margin 1.52e-07, 1 tried
    "skewed-n6144-b1024": 4152,  # margin 1.30e-08, 1 tried
    "skewed-n6144-b1025": 4216,  # margin 1.74e-07, 1 tried
    "skewed-n6144-b4096": 4280,  # margin 4.80e-08, 1 tried
    "skewed-n6145-b1024": 4344,  # margin 1.16e-07, 1 tried
    "skewed-n6145-b1025": 4408,  # margin 5.60e-08, 1 tried
    "skewed-n6145-b4096": 4472,  # margin 2.09e-08, 1 tried
    "zeros-n1024-b1024": 4536,  # margin 4.04e-07, 1 tried
    "zeros-n1024-b1025": 4600,  # margin 5.41e-07, 1 tried
    "zeros-n1024-b4096": 4664,  # margin 3.11e-07, 1 tried
    "zeros-n1025-b1024": 4728,  # margin 9.59e-08, 1 tried
    "zeros-n1025-b1025": 4792,  # margin 8.37e-08, 1 tried
    "zeros-n1025-b4096": 4856,  # margin 4.55e-07, 1 tried
    "zeros-n6144-b1024": 4920,  # margin 2.12e-07, 1 tried
    "zeros-n6144-b1025": 4984,  # margin 4.58e-09, 1 tried
    "zeros-n6144-b4096": 5048,  # margin 3.45e-08, 1 tried
    "zeros-n6145-b1024": 5112,  # margin 4.24e-08, 1 tried
    "zeros-n6145-b1025": 5176,  # margin 7.56e-08, 1 tried
    "zeros-n6145-b4096": 5240,  # margin 1.12e-08, 1 tried
    "flat-n1048576-b64": 5304,  # margin 1.86e-09, 1 tried
    "skewed-n1048576-b64": 5368,  # margin 1.11e-08, 1 tried
    "zeros-n1048576-b64": 5432,  # margin 1.40e-09, 1 tried
    "flat-n1048576-b1025": 5502,  # margin 1.10e-09, 7 tried
    "skewed-n1025-b1025-beta0": 5560,  # margin 4.14e-07, 1 tried
    "zeros-n6145-b4096-beta0": 5624,  # margin 1.10e-07, 1 tried
    "skewed-n1025-b1025-beta1": 5688,  # margin 3.30e-07, 1 tried
    "zeros-n6145-b4096-beta1": 5752,  # margin 1.35e-07, 1 tried
}


def sample_base_seed(sid):
    return 3000 + 64 * SAMPLE_IDS.index(sid)


@functools.lru_cache(maxsize=None)
def sample_priorities(kind, n, k):
    rs = np.random.RandomState(700 + k)
    if kind == "flat":
        return np.ones(n, np.float32)
    p = rs.uniform(0.5, 1.5, size=n).astype(np.float32)
    if kind == "skewed":
        heavy = rs.randint(0, n)
        rest = float(p.astype(np.float64).sum() - p[heavy])
        p[heavy] = np.float32(9.0 * rest)
        return p
    zero = rs.rand(n) < 1.0 / 3.0
    zero[0], zero[-1] = False, True
    p[zero] = 0.0
    return p


def sample_case(sid, seed=None):
    """-> (priorities float32 [n], n, B, seed, draw, beta)"""
    k = SAMPLE_IDS.index(sid)
    c = SAMPLE_CASES[k]
    return sample_priorities(c.kind, c.n, k), c.n, c.B, SAMPLE_SEEDS[sid] if seed is None else seed, 2 + k % 7, c.beta


# ---- 2. the learner with per = 1 on every dispatch arm --------------------------------------------------------------
def _arm_tables():
    import distinct_learner_shapes as DLS
    import dqn_shapes as DS
    return {"rnn": LA.IDS, "dqn": DS.LEARNER_IDS, "distinct": DLS.IDS}


ARM_IDS = [f"{kind}:{cid}" for kind, ids in _arm_tables().items() for cid in ids]


def arm_case(aid):
    """-> (kind, the table's case, its arm name)"""
    kind, cid = aid.split(":")
    if kind == "rnn":
        c = LA.case(cid)
    elif kind == "dqn":
        import dqn_shapes as DS
        c = DS.learner_case(cid)
    else:
        import distinct_learner_shapes as DLS
        c = DLS.case(cid)
    return kind, c, c.arm


def arm_cfg(aid, per):
    """The MlgLearnerCfg of the case at the truncated length (no learner, no GPU)."""
    kind, c, _ = arm_case(aid)
    if kind == "distinct":
        import distinct_learner_shapes as DLS
        cfg = DLS.learner_cfg(c)
    elif kind == "dqn":
        import dqn_shapes as DS
        cfg = DS.learner_cfg(c)
    else:
        cfg = LA.learner_cfg(LA.case_args(c, "cpu"), LA.dims(c)[3])
    cfg.per = per
    return cfg


@functools.lru_cache(maxsize=None)
def arm_inputs(aid):
    """-> (kind, case, args, agent parameters (a list of N for distinct), mixer parameters or None, batch)"""
    kind, c, _ = arm_case(aid)
    if kind == "distinct":
        import distinct_learner_shapes as DLS
        _, args, agents0, mixer0, tb = DLS.inputs(c.id)
        return kind, c, args, agents0, mixer0, tb
    from test_gpu_learner_shapes import mixer_state
    if kind == "dqn":
        import dqn_ref
        import dqn_shapes as DS
        args = DS.learner_args(c)
        agent0 = dqn_ref.agent_state(args, LA.dims(c)[3], seed=c.seed)
        mixer0 = mixer_state(args, seed=c.seed + 8) if args.mixer == "qmix" else None
    else:
        args = LA.case_args(c)
        agent0, mixer0 = LA.case_weights(c, args)
    return kind, c, args, agent0, mixer0, LA.case_batch(c)


def weights(seed, B):
    """Importance weights in (0.1, 1], the largest exactly 1 as mlg_per_sample's are."""
    w = np.random.RandomState(seed).uniform(0.1, 1.0, size=B).astype(np.float32)
    w[int(np.argmax(w))] = 1.0
    return w


def arm_weight(aid):
    return weights(1300 + ARM_IDS.index(aid), int(arm_inputs(aid)[5]["filled"].shape[0]))


def oracle_class(kind):
    import learner_ref as LR
    import per_ref
    if kind == "dqn":
        import dqn_ref
        return per_ref.per_ref_class(dqn_ref.DQNLearnerRef)
    if kind == "distinct":
        import distinct_ref as DR
        return per_ref.per_ref_class(DR.DistinctLearnerRef)
    return per_ref.per_ref_class(LR.QLearnerRef)


def oracle_first_call(kind, args, agent0, mixer0, tb, w, dtype):
    """The weighted oracle's first call on the sample truncated to max_t_filled: (gradients before the clip in flat
    parameter order, td_abs [B], statistics)."""
    import learner_ref as LR
    T = max(2, int(tb["filled"].sum(dim=(1, 2)).max()))
    ob = {k: v[:, :T].clone() for k, v in tb.items()}
    ref = oracle_class(kind)(agent0, mixer0, LR.clone_args(args, device="cpu"), dtype=dtype)
    ref.is_weight = w
    stats = ref.train(ob, 0, 0)
    return [g.detach().clone() for g in ref.last_grads], ref.last_td_abs.detach().clone(), stats


@functools.lru_cache(maxsize=None)
def arm_oracle_f64(aid):
    import torch
    kind, _, args, agent0, mixer0, tb = arm_inputs(aid)
    return oracle_first_call(kind, args, agent0, mixer0, tb, arm_weight(aid), torch.float64)


# ---- 3. the time and batch axes of the per-episode reduce --------------------------------------------------------------
# (id, episodes, stored steps, filled prefixes, {episode: steps that carry `terminated`}, the slot map of a sampled view
# or None)
RCase = namedtuple("RCase", "id B T lens term rows")
_B72_CYCLE = (6, 5, 3, 2, 1, 4, 6, 2)
_B72_EMPTY = (7, 23, 40, 71)
_B72_LENS = tuple(0 if b in _B72_EMPTY else _B72_CYCLE[b % 8] for b in range(72))
REDUCE_CASES = [
    # 64 transitions: exactly one per lane
    RCase("t65", 3, 65, (65, 64, 2), {1: (63,), 2: (1,)}, None),
    # 65: lane 0 takes a second step
    RCase("t66", 3, 66, (66, 65, 2), {1: (64,), 2: (1,)}, None),
    # 129 transitions, two wraps of the lane loop; 131 stored steps > 128: batch_mask_scan by length
    RCase("t130", 2, 131, (130, 40), {1: (39,)}, None),
    # one episode, one wave
    RCase("b1", 1, 8, (6,), {0: (5,)}, None),
    # 72 episodes > 64: batch_mask_scan by count; 72 reduce blocks; four episodes never filled
    RCase("b72", 72, 8, _B72_LENS, {b: (_B72_LENS[b] - 1,) for b in range(0, 72, 3) if _B72_LENS[b] > 0}, None),
    # `terminated` inside the filled prefix of episodes 0 and 2: the mask has a zero with live steps after it, so
    # mlen[b] (9 and 7) exceeds the number of masked steps (8 and 6)
    RCase("hole", 4, 12, (10, 10, 7, 3), {0: (4,), 1: (9,), 2: (2, 6)}, None),
    # the workload's stored length: six episodes in a device ReplayBuffer, sampled in place with a duplicated row; the
    # learner sees T = 101 and trains over max_t_filled = 100 (tdrow's row stride c.T - 1 = 100); one wrap of the lane loop
    RCase("view101", 6, 101, (100, 71, 65, 64, 2, 0), {1: (70,), 3: (63,)}, (2, 0, 2, 4, 1, 5, 3)),
]
REDUCE_MIXERS = {"qmix": (LA.QMIX, "h32/bwd-split/q1 + qmix-split"), "iql": (LA.IQL, "h32/bwd-split/q1 + iql"),
                 "vdn": (LA.VDN, "h32/bwd-split/q1 + vdn-fast")}
REDUCE_IDS = [f"{c.id}-{m}" for c in REDUCE_CASES for m in ("qmix", "iql")] + ["t66-vdn"]
REDUCE_LONG = ("t66", "t130", "view101")


def reduce_case(rid):
    """-> (RCase, mixer name, the learner_arm_shapes.Case that carries dims, H, mixer kwargs, arm and seed)"""
    name, mix = rid.split("-")
    rc = next(c for c in REDUCE_CASES if c.id == name)
    kw, arm = REDUCE_MIXERS[mix]
    return rc, mix, LA.Case("per-" + rid, 32, "2v2", kw, arm, 11)


def reduce_batch(N, A, S, d_obs, rc, seed):
    """learner_arm_shapes.arm_batch's recipe for any lengths and termination steps: random contents at every step,
    filled or not; every agent has an available action and takes one; about a fifth of the (b, t, n) rows have exactly
    one available action."""
    import torch
    rs = np.random.RandomState(seed)
    B, T = rc.B, rc.T
    filled = np.zeros((B, T, 1), np.int64)
    term = np.zeros((B, T, 1), np.uint8)
    for b, f in enumerate(rc.lens):
        filled[b, :f] = 1
    for b, steps in rc.term.items():
        for t in steps:
            assert t < rc.lens[b]
            term[b, t] = 1
    avail = (rs.rand(B, T, N, A) < 0.5).astype(np.int32)
    single = rs.rand(B, T, N) < 0.2
    keep = rs.randint(0, A, size=(B, T, N))
    avail[single] = 0
    np.put_along_axis(avail, keep[..., None], 1, axis=-1)
    actions = np.zeros((B, T, N, 1), np.int64)
    for idx in np.ndindex(B, T, N):
        actions[idx][0] = rs.choice(np.flatnonzero(avail[idx]))
    onehot = np.zeros((B, T, N, A), np.float32)
    np.put_along_axis(onehot, actions, 1.0, axis=-1)
    out = {"state": rs.randn(B, T, S).astype(np.float32), "obs": rs.randn(B, T, N, d_obs).astype(np.float32),
           "actions": actions, "avail_actions": avail, "reward": rs.randn(B, T, 1).astype(np.float32),
           "terminated": term, "actions_onehot": onehot, "filled": filled}
    return {k: torch.from_numpy(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reduce_inputs(rid):
    """-> (RCase, mixer name, Case, args, agent parameters, mixer parameters or None, the stored episodes, the batch the
    learner trains on: the stored episodes, or their rows through the case's slot map)"""
    import torch
    rc, mix, c = reduce_case(rid)
    args = LA.case_args(c)
    agent0, mixer0 = LA.case_weights(c, args)
    stored = reduce_batch(*LA.dims(c), rc, seed=c.seed + 100 + REDUCE_CASES.index(rc))
    tb = stored if rc.rows is None else {k: v[torch.as_tensor(rc.rows)].clone() for k, v in stored.items()}
    return rc, mix, c, args, agent0, mixer0, stored, tb


def reduce_weight(rid):
    rc = reduce_case(rid)[0]
    w = weights(1700 + REDUCE_IDS.index(rid), rc.B)
    return w if rc.rows is None else w[np.asarray(rc.rows)]  # a duplicated episode is drawn with one weight


def reduce_mask(tb):
    """mask = filled[:, :-1] * (1 - terminated shifted) over the sample truncated to max_t_filled, [B, Te - 1]."""
    Te = max(2, int(tb["filled"].sum(dim=(1, 2)).max()))
    f = tb["filled"][:, :Te - 1, 0].numpy().astype(np.float64)
    t = tb["terminated"][:, :Te - 1, 0].numpy().astype(np.float64)
    m = f.copy()
    m[:, 1:] *= 1 - t[:, :-1]
    return m


def reduce_mlen(tb):
    """Skip::mlen of the learner: 1 + the last transition with a non-zero mask, 0 without one."""
    m = reduce_mask(tb)
    return np.asarray([0 if not row.any() else 1 + int(np.flatnonzero(row)[-1]) for row in m])


@functools.lru_cache(maxsize=None)
def reduce_oracle_f64(rid):
    import torch
    _, _, _, args, agent0, mixer0, _, tb = reduce_inputs(rid)
    return oracle_first_call("rnn", args, agent0, mixer0, tb, reduce_weight(rid), torch.float64)


# ---- measured figures ----------------------------------------------------------------------------------------------
# case -> (statistics, gradients, td_abs): the largest distance of the fp32 weighted oracle's first call from the same
# oracle in float64, measured on the CPU by scripts/per_oracle_f64_distance.py. Statistics: the relative distance left
# after the absolute allowance STAT_ATOL, over loss / grad_norm / td_error_abs / q_taken_mean / target_mean; gradients:
# per tensor before the clip, relative to max(1, max|g|) of the float64 tensor; td_abs: relative to max(1, max|td_abs|).
# Listed for the cases that have no figure in learner_arm_shapes.ORACLE_F64: the dqn and distinct arm tables and the
# long reduce cases. A bound of the GPU tests is the project's (STAT_RTOL, GRAD_RTOL, OP_TOL), or ten times the distance
# here where that is larger; the resulting bound is bounds()'s.
ORACLE_F64 = {
    "dqn:ff-qmix-h64-5v5": (2.09e-08, 3.82e-07, 8.78e-08),  # grad_norm 18.41
    "dqn:ff-qmix-h32-1v1": (0.00e+00, 1.64e-07, 3.13e-08),  # grad_norm 7.626
    "dqn:ff-qmix-h128-17v17": (1.49e-07, 5.53e-07, 1.68e-07),  # grad_norm 88.94
    "dqn:ff-vdn-h32-3v3": (0.00e+00, 1.85e-07, 3.94e-08),  # grad_norm 3.532
    "dqn:ff-vdn-h64-17v17": (6.09e-08, 3.72e-07, 5.34e-08),  # grad_norm 63.5
    "dqn:ff-iql-h128-2v2": (0.00e+00, 2.43e-08, 4.47e-08),  # grad_norm 1.093
    "dqn:ff-h1-e32-h64-7v7": (7.57e-08, 7.08e-07, 2.28e-07),  # grad_norm 354.2
    "dqn:ff-he32-e16-h32-5v5": (0.00e+00, 8.42e-08, 1.12e-07),  # grad_norm 4.672
    "distinct:n2-h32-b17": (0.00e+00, 1.63e-07, 2.56e-07),  # grad_norm 3.921
    "distinct:n32-h32-b5": (1.32e-08, 1.57e-07, 1.57e-07),  # grad_norm 8.356
    "distinct:n3-h128-a17": (5.10e-08, 2.19e-07, 1.79e-07),  # grad_norm 23.67
    "distinct:n4-h64-b33": (0.00e+00, 2.56e-09, 5.54e-08),  # grad_norm 0.1403
    "distinct:n5-h64-b32": (0.00e+00, 7.06e-08, 1.93e-07),  # grad_norm 3.516
    "distinct:n1-h64-b16": (0.00e+00, 2.40e-07, 9.39e-08),  # grad_norm 9.729
    "t66-qmix": (0.00e+00, 9.03e-08, 7.75e-08),  # grad_norm 3.745
    "t66-iql": (0.00e+00, 2.34e-09, 2.66e-08),  # grad_norm 0.05966
    "t130-qmix": (0.00e+00, 3.48e-08, 8.80e-08),  # grad_norm 1.745
    "t130-iql": (0.00e+00, 1.24e-08, 6.39e-08),  # grad_norm 0.2157
    "view101-qmix": (0.00e+00, 8.10e-08, 4.49e-08),  # grad_norm 2.159
    "view101-iql": (0.00e+00, 3.01e-09, 5.17e-08),  # grad_norm 0.08738
    "t66-vdn": (0.00e+00, 1.30e-08, 2.13e-08),  # grad_norm 0.54
}
OP_TOL = 1e-4


def bounds(key):
    """(statistic rtol, gradient bound relative to max(1, max|g_ref|) per tensor, td_abs bound relative to
    max(1, max|ref|)) of an arm case ("kind:id") or a reduce case."""
    if key.startswith("rnn:"):
        s, _, g = LA.bounds(key[4:])
        return s, g, OP_TOL
    if key in ORACLE_F64:
        s, g, t = ORACLE_F64[key]
        return max(LA.STAT_RTOL, 10 * s), max(LA.GRAD_RTOL, 10 * g), max(OP_TOL, 10 * t)
    assert key in REDUCE_IDS and key.split("-")[0] not in REDUCE_LONG, key  # the short reduce cases: the project's
    return LA.STAT_RTOL, LA.GRAD_RTOL, OP_TOL
