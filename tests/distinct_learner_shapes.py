"""The fused distinct-network learner's cases (mlg_qlearner_train with cfg.distinct = 1), shared by
tests/test_distinct_learner_dispatch.py (CPU: names, counts, refusals, and the oracles' own agreement on every pick)
and tests/test_gpu_distinct_learner_fused.py (GPU parity).

A case is (id, N, H, A, B, mixer kwargs on top of helpers.qmix_args(), obs_last_action, arm, seed). S = 36 and
d_obs = 23 (d_in = 34 with the last action: no row is a whole number of 16-byte vectors) except at the timing shape's
arm, which keeps the 5-agent plan's S = 60, d_obs = 80. ``arm`` is what mlg_qlearner_describe reports. ``seed`` seeds the
N networks (distinct_ref.agent_params), the mixer (seed + 8) and the batch (seed + 100).

The agent kernels run N instances of R = B rows in 16-row tiles, so B is the size that matters: 17 = one full tile and
one row (and a 4-row recurrence tile with one row), 33 = three tiles, 32 and 16 = whole tiles, 5 = one partial tile.

Seeds. A pick (the double-Q argmax of the online Q at t + 1, or the argmax behind the masked max of the target Q where
double_q is off) that differs between the device and the oracle moves a target by a whole Q gap, which no tolerance
here covers. A seed is kept only if the fp32 and the float64 oracle, each on its own trajectory over the three calls,
agree on every live (b, t, n) pick: 0 disagreements, counted by test_distinct_learner_dispatch.py.
"""
import functools
from collections import namedtuple

import numpy as np

import learner_arm_shapes as LA

Case = namedtuple("Case", "id N H A B mixer last_action arm seed")

QMIX1_E16 = {"hypernet_layers": 1, "mixing_embed_dim": 16}
QMIX_NODQ = {"mixing_embed_dim": 32, "hypernet_embed": 64, "double_q": False}

CASES = [
    Case("n2-h32-b17", 2, 32, 11, 17, LA.QMIX, True, "dx-h32/bwd-split/q1 + qmix-generic", 11),
    Case("n32-h32-b5", 32, 32, 5, 5, LA.VDN, True, "dx-h32/bwd-split/q1 + vdn", 11),           # the largest N
    Case("n3-h128-a17", 3, 128, 17, 5, QMIX1_E16, True, "dx-h128/bwd-split/q2 + qmix1-e16", 11),  # two action tiles
    Case("n4-h64-b33", 4, 64, 11, 33, LA.IQL, False, "dx-h64/bwd-split/q1 + iql", 11),          # expanded mask
    Case("n5-h64-b32", 5, 64, 15, 32, QMIX_NODQ, True, "dx-h64/bwd-split/q1 + qmix-generic", 11),  # the timing shape's arm
    Case("n1-h64-b16", 1, 64, 11, 16, LA.QMIX, True, "dx-h64/bwd-split/q1 + qmix-generic", 11),  # degenerate N
]
IDS = [c.id for c in CASES]

T_STORED = 8
# filled prefixes by episode, cyclically: a never-filled episode (0) and a one-transition episode (1) in every batch
LENS = (6, 5, 0, 3, 1, 2, 6, 4)
T_FILLED = max(LENS)
TERMINATED = (0, 3, 4, 7)  # positions of the cycle whose last filled step carries `terminated`
CALLS = LA.CALLS           # target == online; stale target; stale target, ends with the sync


def case(cid):
    return next(c for c in CASES if c.id == cid)


def dims(c):
    """(N, A, S, d_obs)"""
    return (c.N, c.A, 60, 80) if c.id == "n5-h64-b32" else (c.N, c.A, 36, 23)


def case_args(c, device="cuda"):
    from helpers import qmix_args
    N, A, S, _ = dims(c)
    return qmix_args(n_agents=N, n_actions=A, state_shape=S, rnn_hidden_dim=c.H, obs_agent_id=False, mac="distinct",
                     obs_last_action=c.last_action, device=device, **c.mixer)


def learner_cfg(c, distinct=1):
    cfg = LA.learner_cfg(case_args(c, "cpu"), dims(c)[3], B=c.B, T=T_FILLED)
    cfg.distinct = distinct
    return cfg


def lens(B):
    return [LENS[b % len(LENS)] for b in range(B)]


def batch(N, A, S, d_obs, B, seed, T=T_STORED):
    """learner_arm_shapes.arm_batch for any B: filled prefixes LENS cyclically (a never-filled and a one-transition
    episode among them), `terminated` on the last filled step of the TERMINATED positions. Every agent has an available
    action and takes one; about a fifth of the (b, t, n) rows have exactly one. Random contents at every step, filled
    or not."""
    import torch
    rs = np.random.RandomState(seed)
    filled = np.zeros((B, T, 1), np.int64)
    term = np.zeros((B, T, 1), np.uint8)
    for b, f in enumerate(lens(B)):
        filled[b, :f] = 1
        if b % len(LENS) in TERMINATED and f > 0:
            term[b, f - 1] = 1
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


def oracle_batch(tb):
    """The sample the reference trains on: truncated to max_t_filled."""
    return {k: v[:, :T_FILLED].clone() for k, v in tb.items()}


def mask(tb):
    """mask = filled[:, :-1] * (1 - terminated shifted) over the truncated sample, [B, T_FILLED - 1] in numpy."""
    f = tb["filled"][:, :T_FILLED - 1, 0].numpy().astype(np.float64)
    t = tb["terminated"][:, :T_FILLED - 1, 0].numpy().astype(np.float64)
    m = f.copy()
    m[:, 1:] *= 1 - t[:, :-1]
    return m


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(case, args, N agent state dicts, mixer state dict or None, batch) of a case, built once."""
    import distinct_ref as DR
    from test_gpu_learner_shapes import mixer_state
    c = case(cid)
    args = case_args(c)
    N, A, S, d_obs = dims(c)
    agents0 = DR.all_agent_params(N, d_obs + (A if c.last_action else 0), c.H, A, c.seed)
    mixer0 = mixer_state(args, seed=c.seed + 8) if args.mixer == "qmix" else None
    tb = batch(N, A, S, d_obs, c.B, seed=c.seed + 100)
    return c, args, agents0, mixer0, tb


def make_oracle(agents0, mixer0, args, dtype=None):
    import torch

    import distinct_ref as DR
    import learner_ref as LR
    return DR.learner_ref(agents0, mixer0, LR.clone_args(args, device="cpu"), dtype=dtype or torch.float32)


@functools.lru_cache(maxsize=None)
def oracle(cid):
    """Once per case: the fp32 oracle's three calls (statistics per call, the oracle after them) and the float64
    oracle's first call (gradients before the clip in flat parameter order, its statistics)."""
    import torch
    _, args, agents0, mixer0, tb = inputs(cid)
    ob = oracle_batch(tb)
    ref = make_oracle(agents0, mixer0, args)
    stats = [ref.train({k: v.clone() for k, v in ob.items()}, t_env, ep) for t_env, ep in CALLS]
    ref64 = make_oracle(agents0, mixer0, args, torch.float64)
    s64 = ref64.train({k: v.clone() for k, v in ob.items()}, *CALLS[0])
    return stats, ref, [g.clone() for g in ref64.last_grads], s64
