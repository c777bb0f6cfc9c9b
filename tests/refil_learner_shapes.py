"""The REFIL learner's shape cases (mlg_refil_train off the refil_8 shape) shared by tests/test_refil_learner_shapes.py
(CPU: the conditions on the table below, checked with the float64 oracle alone), tests/test_gpu_refil_learner_shapes.py
(GPU: parity per case) and scripts/refil_oracle_f64_distance.py (CPU: how far the fp32 oracle is from a float64 run of
itself -- the ORACLE_F64 table below -- and the near-tie gap and grad_norm written beside each case).

A case is (id, agent, mixer, NA, NE, ED, A, last_action, B, T_stored, lens, reward_scale, softmax, double_q, seed).
``lens[b]`` is the number of transitions of episode b (steps 0 .. lens[b] filled; -1: never filled). ``seed`` seeds the
batch, the CPU modules the initial weights come from and the imagine group draws. The comment above a case says which
branch of csrc/refil_learner.hip it is there for; REACHES restates that claim in figures, and the CPU test recomputes
them from the table. The oracle is oracle/refil_ref.py (the imagine agent) or tests/refil_baseline_ref.py (the plain
agent), never the code under test.

Unless its comment says otherwise a case has B = 6 episodes of 12 stored steps with DEFAULT_LENS: the longest fills 11
of the 12 (max_t_filled < T), episode 1 is never filled, episode 2 holds one transition, the even episodes end with
``terminated``.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "id agent mixer NA NE ED A last_action B T lens reward_scale softmax double_q seed")

IMAGINE, PLAIN = "imagine_entity_attend_rnn", "entity_attend_rnn"
DEFAULT_LENS = (10, -1, 1, 6, 4, 7)
# 33 episodes of 6 stored steps: 1 to 4 transitions, episode 0 the longest (fills 5 of 6), one never filled
B33_LENS = (4, -1, 1) + tuple(1 + (7 * b) % 4 for b in range(30))
# terminated (even b): mix_len = lens[b]; not terminated: lens[b] + 1, capped at max_t_filled - 1 = 65
TWORDS_LENS = (31, 31, 33, 62, 64, 65)

Q_TOL = 1e-4          # the smallest top-two gap of the masked online Q a seed is kept at (helpers.Q_TOL, ten times the
                      # Q accuracy the README states)
CLIP = 10.0           # grad_norm_clip; the float64 first-call grad_norm is > 20 for the -clip cases, < 5 elsewhere
CALLS = (0, 100, 200)  # episode_num: target == online; stale target; stale target and the call ends with the sync


def _c(cid, agent, mixer, NA, NE, ED, A, la=True, B=6, T=12, lens=DEFAULT_LENS, scale=1.0, softmax=False, dq=True,
       seed=1):
    return Case(cid, agent, mixer, NA, NE, ED, A, la, B, T, tuple(lens), scale, softmax, dq, seed)


def _shape(name):
    """(NA, NE, ED, A, last_action) + batch kwargs of the shapes the baselines repeat."""
    return {"na8-ne12-a17": ((8, 12, 8, 17), {}),
            "na1-ne1": ((1, 1, 8, 6), dict(B=3, T=9, lens=(7, 1, -1))),
            "k48-a32": ((4, 11, 16, 32), {}),
            "nola-a16": ((5, 9, 8, 16), dict(la=False))}[name]


# Beside each case: gap = the smallest top-two gap of the float64 oracle's masked online Q over the three calls
# (top_two_gap below; a seed is kept at >= Q_TOL), gn = its first-call grad_norm; both printed by
# scripts/refil_oracle_f64_distance.py. gpu = the largest first-call gradient error over its bound, of any tensor, seen
# on the MI355X (tests/test_gpu_refil_learner_shapes.py prints it).
CASES = [
    # the static instantiation of the per-item kernels (refil_8 itself), and the generic one at the same shape
    _c("s8-static", IMAGINE, "flex_qmix", 8, 16, 8, 21, seed=2),           # gap 4.03e-04, gn 0.2784, gpu 0.005
    _c("s8-generic", IMAGINE, "flex_qmix", 8, 16, 8, 21, seed=2),          # MLG_REFIL_GENERIC=1; gap 4.03e-04, gn 0.2784, gpu 0.005
    # generic instantiation with NA % 8 == 0 (make_jobs' step skipping) off refil_8; A one past an action tile
    _c("na8-ne12-a17", IMAGINE, "flex_qmix", *_shape("na8-ne12-a17")[0], seed=1),   # gap 2.86e-04, gn 0.4375, gpu 0.005
    # D0 = 3 + 13 = 16 = K1: no padded input column; every entity is an agent
    _c("na8-ne8-d16", IMAGINE, "flex_qmix", 8, 8, 3, 13, seed=1),          # gap 4.17e-04, gn 0.2846, gpu 0.038
    # NA % 8 != 0 (no step skipping, conditional zeroing of d2 / dfc2 / dout) at the full entity width
    _c("na7-ne16", IMAGINE, "flex_qmix", 7, 16, 8, 21, seed=1),            # gap 2.75e-04, gn 0.2543, gpu 0.006
    # one agent, one entity; B * T = 27 is odd (ent_fwd / ent_bwd's last item pair is half empty); Ron = 3 * 3 * 1 = 9
    # rows: partial four-row (rec4) and 16-row (q_kernel) tiles. Episode 1 holds one transition, episode 2 none.
    _c("na1-ne1", IMAGINE, "flex_qmix", *_shape("na1-ne1")[0], seed=1, **_shape("na1-ne1")[1]),  # gap 2.29e-03, gn 1.121, gpu 0.007
    # one agent among 16 entities; the target's plain max instead of the double-Q gather
    _c("na1-ne16", IMAGINE, "flex_qmix", 1, 16, 8, 21, dq=False, seed=3),  # gap 6.31e-04, gn 0.1573, gpu 0.014
    # D0 = 16 + 32 = 48 = KMAX (three K tiles of ein_body / dense_lds); both action tiles full
    _c("k48-a32", IMAGINE, "flex_qmix", *_shape("k48-a32")[0], seed=9),    # gap 9.56e-04, gn 0.4049, gpu 0.004
    # D0 = 12 + 21 = 33: K1 = 48 with 15 padded columns; softmax mixing weights
    _c("k33", IMAGINE, "flex_qmix", 2, 5, 12, 21, softmax=True, seed=2),   # gap 1.67e-03, gn 0.2386, gpu 0.026
    # no last-action columns: D0 = ED = 8, K1 = 16; A = 16 fills one action wave exactly
    _c("nola-a16", IMAGINE, "flex_qmix", *_shape("nola-a16")[0], seed=3, **_shape("nola-a16")[1]),  # gap 3.61e-04, gn 0.5842, gpu 0.009
    # 33 episodes: one past the 32 the one-round-trip mask statistics hold (batch_mask_scan by the episode count)
    _c("b33", IMAGINE, "flex_qmix", 3, 7, 8, 12, B=33, T=6, lens=B33_LENS, seed=1),   # gap 1.18e-03, gn 0.0986, gpu 0.004
    # 131 stored steps (> 128): batch_mask_scan by the length; a 129-step recurrence
    _c("t130", IMAGINE, "flex_qmix", 2, 4, 8, 9, B=2, T=131, lens=(129, 40), seed=4),  # gap 2.63e-03, gn 0.2727, gpu 0.003
    # mix_len 31 / 32 / 33 / 63 / 64 / 65: either side of the 32-bit words of live bits in batch_mask_stats
    _c("twords", IMAGINE, "flex_qmix", 2, 4, 8, 9, T=67, lens=TWORDS_LENS, seed=1),   # gap 3.37e-04, gn 0.1162, gpu 0.008
    # clip_grad_norm_ engaged (the clipped branch of the optimiser launch). Rewards x 100 put k48-a32 at a grad_norm
    # of 38; with softmax mixing weights na7-ne16 reaches only 4.0 to 9.3 at x 100 (seeds 1 to 4), the wrong side of
    # the clip, so its rewards are x 400.
    _c("na7-ne16-clip", IMAGINE, "flex_qmix", 7, 16, 8, 21, scale=400.0, softmax=True, seed=1),  # gap 2.75e-04, gn 37.08, gpu 0.018
    _c("k48-a32-clip", IMAGINE, "flex_qmix", 4, 11, 16, 32, scale=100.0, seed=9),     # gap 1.65e-03, gn 43.9, gpu 0.004
    # the plain agent: the NC = 1 kernels, mix_td1 (flex_qmix and VDN) and the no-hypernet plan
    _c("attn-qmix-na8-ne12-a17", PLAIN, "flex_qmix", *_shape("na8-ne12-a17")[0], seed=1),  # gap 5.93e-04, gn 0.3316, gpu 0.005
    _c("attn-vdn-na8-ne12-a17", PLAIN, "vdn", *_shape("na8-ne12-a17")[0], seed=3),    # gap 2.21e-04, gn 3.349, gpu 0.003
    _c("attn-qmix-na1-ne1", PLAIN, "flex_qmix", *_shape("na1-ne1")[0], seed=11, **_shape("na1-ne1")[1]),  # gap 2.36e-02, gn 0.694, gpu 0.013
    _c("attn-vdn-na1-ne1", PLAIN, "vdn", *_shape("na1-ne1")[0], seed=2, **_shape("na1-ne1")[1]),  # gap 1.09e-02, gn 0.3926, gpu 0.004
    _c("attn-qmix-k48-a32", PLAIN, "flex_qmix", *_shape("k48-a32")[0], seed=9),       # gap 9.29e-04, gn 0.3818, gpu 0.004
    _c("attn-vdn-k48-a32", PLAIN, "vdn", *_shape("k48-a32")[0], seed=9),              # gap 5.61e-04, gn 0.7657, gpu 0.005
    _c("attn-qmix-nola-a16", PLAIN, "flex_qmix", *_shape("nola-a16")[0], seed=4, **_shape("nola-a16")[1]),  # gap 3.41e-04, gn 0.6779, gpu 0.012
    _c("attn-vdn-nola-a16", PLAIN, "vdn", *_shape("nola-a16")[0], seed=2, **_shape("nola-a16")[1]),  # gap 5.04e-04, gn 1.42, gpu 0.003
]
IDS = [c.id for c in CASES]
GENERIC = {"s8-generic"}   # cases run with MLG_REFIL_GENERIC=1
CLIPPED = {"na7-ne16-clip", "k48-a32-clip"}

# What each case's comment claims, in the kernels' own dimensions (make_plan, batch_mask_device.h); `derived` below
# recomputes every figure from the table. I = B * T items, Ron = copies * B * NA online rows, Te = max_t_filled.
REACHES = {
    "s8-static": dict(static=True, D0=29, K1=32, Ap=32, step_skip=True),
    "s8-generic": dict(static=False, D0=29, K1=32, Ap=32, step_skip=True),
    "na8-ne12-a17": dict(static=False, step_skip=True, A=17, Ap=32),
    "na8-ne8-d16": dict(static=False, D0=16, K1=16, NE_minus_NA=0, step_skip=True),
    "na7-ne16": dict(static=False, step_skip=False, D0=29, K1=32),
    "na1-ne1": dict(I_odd=True, Ron=9, Ron_mod4=1, Ron_mod16=9, step_skip=False),
    "na1-ne16": dict(Ron=18, step_skip=False, double_q=False),
    "k48-a32": dict(D0=48, K1=48, A=32, Ap=32),
    "k33": dict(D0=33, K1=48, softmax=True),
    "nola-a16": dict(D0=8, K1=16, A=16, Ap=16),
    "b33": dict(mask_path="scan", B_over_32=True, T_over_128=False),
    "t130": dict(mask_path="scan", B_over_32=False, T_over_128=True, Te=130),
    "twords": dict(mask_path="stats", mix_lens={31, 32, 33, 63, 64, 65}),
    "na7-ne16-clip": dict(step_skip=False, softmax=True),
    "k48-a32-clip": dict(D0=48, K1=48),
}
for _cid in IDS:
    if _cid.startswith("attn-"):
        _base = dict(REACHES[_cid.split("-", 2)[2]])
        _base.pop("static", None)
        if "Ron" in _base:  # one online copy
            _base.update(Ron=3, Ron_mod4=3, Ron_mod16=3)
        REACHES[_cid] = _base

KMAX, MASK_STATS_B, MASK_STATS_T = 48, 32, 128


def case(cid):
    return next(c for c in CASES if c.id == cid)


def case_env(c):
    return {"MLG_REFIL_GENERIC": "1"} if c.id in GENERIC else {}


def case_args(c, device="cuda"):
    from helpers import refil_args
    return refil_args(device=device, n_agents=c.NA, n_entities=c.NE, n_actions=c.A, entity_shape=c.ED,
                      entity_last_action=c.last_action, agent=c.agent, mixer=c.mixer,
                      softmax_mixing_weights=c.softmax, double_q=c.double_q)


def synthetic_entity_batch(B, T1, NA, NE, ED, A, lens, seed, reward_scale=1.0, next_avail=False):
    """A random entity-scheme batch of any shape (the env variant only produces NA = 8): episode b holds lens[b]
    transitions (filled t <= lens[b], terminated at lens[b] - 1 for even b; lens[b] = -1: never filled, every field
    zero), a random number of active entities (the rest padded: entity_mask 1, zero features), random observability,
    availability (>= 1 per agent row) and actions among the available ones. A is free of NE; whether the last action
    enters the networks is the args' entity_last_action, not the batch's concern. Rewards are N(0, 1) times
    ``reward_scale``. An episode that does not end with ``terminated`` has a live transition at t = lens[b] whose next
    step is not filled: with every action unavailable there (the default, what tests written on this batch expect)
    its target is built from the -9999999 fill -- FlexQMixer's ELU saturates on it, VDN sums it to -1e7 NA and a
    grad_norm of 1e7. ``next_avail`` keeps that one step's random availability, so the target is an ordinary Q of
    the target network (zero features, every entity present). Keys as EpisodeBatch.transition_data."""
    rng = np.random.RandomState(seed)
    ent = (0.5 * rng.randn(B, T1, NE, ED)).astype(np.float32)
    emask = np.zeros((B, T1, NE), np.uint8)
    omask = (rng.rand(B, T1, NE, NE) < 0.3).astype(np.uint8)
    avail = (rng.rand(B, T1, NA, A) < 0.5).astype(np.int32)
    avail[..., 0] = np.maximum(avail[..., 0], (avail.sum(-1) == 0).astype(np.int32))
    acts = np.zeros((B, T1, NA, 1), np.int64)
    filled = np.zeros((B, T1, 1), np.int64)
    term = np.zeros((B, T1, 1), np.uint8)
    rew = rng.randn(B, T1, 1).astype(np.float32)
    if reward_scale != 1.0:
        rew *= np.float32(reward_scale)
    for b in range(B):
        k = rng.randint(max(1, NA - 3), NA + 1)  # active agents
        kn = rng.randint(k, NE + 1)               # active entities
        emask[b, :, kn:] = 1
        emask[b, :, k:NA] = 1
        L = int(lens[b])
        filled[b, :L + 1] = 1
        if b % 2 == 0 and L >= 1:
            term[b, L - 1] = 1
        for t in range(T1):
            dead = rng.rand(NE) < 0.1
            emask[b, t, dead] = 1
            for n in range(NA):
                ok = np.nonzero(avail[b, t, n])[0]
                acts[b, t, n, 0] = ok[rng.randint(len(ok))]
        emask[b, L + 1:] = 0
    ent[emask.astype(bool)] = 0.0
    omask = np.maximum(omask, emask[:, :, None, :])
    omask = np.maximum(omask, emask[:, :, :, None])
    for x in (ent, rew, avail, acts):
        for b in range(B):
            keep = 1 if (x is avail and next_avail and lens[b] >= 0 and term[b].sum() == 0) else 0
            x[b, int(lens[b]) + 1 + keep:] = 0
    omask[filled[..., 0] == 0] = 0
    emask[filled[..., 0] == 0] = 0
    onehot = np.zeros((B, T1, NA, A), np.float32)
    np.put_along_axis(onehot, acts, 1.0, axis=-1)
    onehot[filled[..., 0] == 0] = 0
    return {"entities": ent, "obs_mask": omask, "entity_mask": emask, "actions": acts, "avail_actions": avail,
            "reward": rew, "terminated": term, "actions_onehot": onehot, "filled": filled}


def case_arrays(c):
    """The stored batch of a case (numpy, T stored steps)."""
    return synthetic_entity_batch(c.B, c.T, c.NA, c.NE, c.ED, c.A, c.lens, seed=c.seed + 100,
                                  reward_scale=c.reward_scale, next_avail=True)


def t_filled(arrs):
    """max_t_filled: the longest filled prefix, clamped to [2, T] (ma_experiment.py:235-239)."""
    f = arrs["filled"].reshape(len(arrs["filled"]), -1)
    return int(np.clip(f.sum(axis=1).max(), 2, f.shape[1]))


def oracle_batch(arrs):
    """The sample the reference trains on: truncated to max_t_filled, as torch tensors."""
    import torch
    Tf = t_filled(arrs)
    return {k: torch.from_numpy(np.ascontiguousarray(v[:, :Tf])) for k, v in arrs.items()}


def live_mask(arrs):
    """mask(b, t) = filled(b, t) * (1 - terminated(b, t - 1)) over t < max_t_filled - 1, float64 [B, Te - 1]."""
    Tf = t_filled(arrs)
    f = arrs["filled"][:, :Tf - 1, 0].astype(np.float64)
    t = arrs["terminated"][:, :Tf - 1, 0].astype(np.float64)
    m = f.copy()
    m[:, 1:] *= 1 - t[:, :-1]
    return m


def mask_sum(arrs):
    return float(live_mask(arrs).sum())


def mix_lens(arrs):
    """Per episode: 1 + the last live transition (0: none), batch_mask_device.h's mixlen."""
    m = live_mask(arrs)
    return [int(np.flatnonzero(r).max()) + 1 if r.any() else 0 for r in m]


def last_action_picks(c, arrs):
    """How often a present agent takes the last action at a live transition: the next step's input then carries a
    one in its last column (D0 - 1 with the last-action columns), and the chosen Q is read from the last action."""
    live = live_mask(arrs) != 0
    Tf = t_filled(arrs)
    present = arrs["entity_mask"][:, :Tf - 1, :c.NA] == 0
    return int(((arrs["actions"][:, :Tf - 1, :, 0] == c.A - 1) & present & live[:, :, None]).sum())


def derived(c, arrs=None):
    """The kernels' dimensions for a case (make_plan / is_s8 / make_jobs / batch_mask of csrc/refil_learner.hip)."""
    arrs = case_arrays(c) if arrs is None else arrs
    D0 = c.ED + (c.A if c.last_action else 0)
    nc = 3 if c.agent == IMAGINE else 1
    Ron = nc * c.B * c.NA
    stats_path = c.B <= MASK_STATS_B and c.T <= MASK_STATS_T
    return dict(D0=D0, K1=(D0 + 15) // 16 * 16, A=c.A, Ap=(c.A + 15) // 16 * 16, I_odd=(c.B * c.T) % 2 == 1, Ron=Ron,
                Ron_mod4=Ron % 4, Ron_mod16=Ron % 16, step_skip=c.NA % 8 == 0, NE_minus_NA=c.NE - c.NA,
                static=(c.NA, c.NE, c.ED, c.A, D0) == (8, 16, 8, 21, 29) and c.id not in GENERIC,
                mask_path="stats" if stats_path else "scan", B_over_32=c.B > MASK_STATS_B,
                T_over_128=c.T > MASK_STATS_T, Te=t_filled(arrs), mix_lens=set(mix_lens(arrs)), softmax=c.softmax,
                double_q=c.double_q)


def case_weights(c):
    """(agent state_dict, mixer state_dict or None) of seeded CPU modules, as numpy."""
    import torch
    from maleague.modules.agents import REGISTRY as agent_REGISTRY
    from maleague.modules.mixers import FlexQMixer
    a_cpu = case_args(c, "cpu")
    torch.manual_seed(c.seed)
    mixer_p = None
    if c.mixer == "flex_qmix":
        mixer_p = {k: v.detach().cpu().numpy().copy() for k, v in FlexQMixer(a_cpu).state_dict().items()}
    ag = agent_REGISTRY[c.agent](c.ED + (c.A if c.last_action else 0), a_cpu)
    return {k: v.detach().cpu().numpy().copy() for k, v in ag.state_dict().items()}, mixer_p


def case_groups(c):
    """The imagine group draw of each call ([B, 1, NE] uint8, entity_rnn_agent.py:95-97); None for the plain agent."""
    import torch
    if c.agent != IMAGINE:
        return [None] * len(CALLS)
    g = torch.Generator().manual_seed(c.seed + 7)
    return [torch.bernoulli(torch.rand(c.B, 1, 1, generator=g).repeat(1, 1, c.NE), generator=g).to(torch.uint8)
            for _ in CALLS]


def make_ref(c, dtype=None):
    """The case's CPU oracle in ``dtype`` (default float32)."""
    import torch
    import refil_baseline_ref as BR
    import refil_ref as RR
    agent_p, mixer_p = case_weights(c)
    dtype = torch.float32 if dtype is None else dtype
    if c.agent == IMAGINE:
        return RR.REFILLearnerRef(agent_p, mixer_p, case_args(c, "cpu"), dtype=dtype)
    return BR.REFILBaselineRef(agent_p, mixer_p or {}, case_args(c, "cpu"), dtype=dtype)


def ref_train(ref, c, batch, groupA, episode_num):
    batch = {k: v.clone() for k, v in batch.items()}
    if c.agent == IMAGINE:
        return ref.train(batch, groupA, episode_num=episode_num)
    return ref.train(batch, episode_num=episode_num)


def top_two_gap(ref, c, batch):
    """The smallest gap between the two largest masked online Q values of ``ref``'s current agent, over every step
    t >= 1 that is filled or is the next step of a live transition (what the double-Q argmax reads), live agents with
    at least two available actions."""
    import torch
    import refil_ref as RR
    with torch.no_grad():
        q, _ = RR.mac_forward({k: v.detach() for k, v in ref.agent.items()}, ref.cast(batch), ref.args)
    q = q.clone()
    avail = batch["avail_actions"]
    q[avail == 0] = -9999999
    top = q.topk(2, dim=3)[0]
    gap = top[..., 0] - top[..., 1]
    arrs = {k: v.numpy() for k, v in batch.items() if k in ("filled", "terminated")}
    read = batch["filled"][:, :, 0] != 0
    read[:, 1:] |= torch.from_numpy(live_mask(arrs) != 0)
    read[:, 0] = False
    use = read.unsqueeze(2) & (batch["entity_mask"][:, :, :c.NA] == 0) & (avail.sum(-1) >= 2)
    return float(gap[use].min()) if bool(use.any()) else float("inf")


def run_oracle(c, dtype, calls=CALLS, arrs=None):
    """``calls`` train calls of the case's oracle in ``dtype``: (statistics per call, the oracle after them, the
    first call's gradients before the clip, the smallest top-two gap seen before any of the calls)."""
    batch = oracle_batch(case_arrays(c) if arrs is None else arrs)
    ref = make_ref(c, dtype)
    groups = case_groups(c)
    stats, grads, gap = [], None, float("inf")
    for i, ep in enumerate(calls):
        gap = min(gap, top_two_gap(ref, c, batch))
        stats.append(ref_train(ref, c, batch, groups[i], ep))
        if grads is None:
            grads = [g.clone() for g in ref.last_grads]
    return stats, ref, grads, gap


# ---- the fp32 oracle's distance from the float64 oracle (scripts/refil_oracle_f64_distance.py) ----------------------
# case -> (statistics, parameters, gap, grad_norm): the largest |s32 - s64| / (STAT_ATOL / STAT_RTOL + |s64|) of a
# statistic over the three calls (the rtol at which assert_allclose's rtol / atol pair, scaled together, would just
# hold); the largest absolute distance of a parameter (online or target) after them; the float64 oracle's smallest
# top-two gap; its first-call grad_norm.
STAT_RTOL, STAT_ATOL, PARAM_ATOL, GRAD_RTOL = 2e-4, 1e-5, 2e-5, 1e-4  # this learner's bounds against the oracle
ORACLE_F64 = {
    "s8-static": (1.31e-07, 2.50e-08, 4.03e-04, 0.2784),  # largest d32 / max|g64| 3.9e-07
    "s8-generic": (1.31e-07, 2.50e-08, 4.03e-04, 0.2784),  # largest d32 / max|g64| 3.9e-07
    "na8-ne12-a17": (1.13e-07, 3.94e-08, 2.86e-04, 0.4375),  # largest d32 / max|g64| 5.4e-07
    "na8-ne8-d16": (1.70e-07, 5.41e-08, 4.17e-04, 0.2846),  # largest d32 / max|g64| 1.0e-06
    "na7-ne16": (1.22e-07, 2.21e-08, 2.75e-04, 0.2543),  # largest d32 / max|g64| 4.2e-07
    "na1-ne1": (1.27e-07, 1.32e-07, 2.29e-03, 1.121),  # largest d32 / max|g64| 3.4e-07
    "na1-ne16": (1.42e-07, 4.08e-08, 6.31e-04, 0.1573),  # largest d32 / max|g64| 7.3e-07
    "k48-a32": (1.12e-07, 2.91e-08, 9.56e-04, 0.4049),  # largest d32 / max|g64| 3.1e-07
    "k33": (8.98e-08, 2.10e-08, 1.67e-03, 0.2386),  # largest d32 / max|g64| 1.8e-06
    "nola-a16": (3.02e-07, 4.06e-08, 3.61e-04, 0.5842),  # largest d32 / max|g64| 8.5e-07
    "b33": (8.21e-08, 2.39e-08, 1.18e-03, 0.0986),  # largest d32 / max|g64| 4.0e-07
    "t130": (2.38e-07, 2.93e-08, 2.63e-03, 0.2727),  # largest d32 / max|g64| 4.4e-07
    "twords": (1.23e-07, 2.48e-08, 3.37e-04, 0.1162),  # largest d32 / max|g64| 8.7e-07
    "na7-ne16-clip": (9.40e-08, 3.11e-07, 2.75e-04, 37.08),  # largest d32 / max|g64| 1.6e-06
    "k48-a32-clip": (1.77e-07, 1.86e-07, 1.65e-03, 43.9),  # largest d32 / max|g64| 2.8e-07
    "attn-qmix-na8-ne12-a17": (1.27e-07, 6.47e-08, 5.93e-04, 0.3316),  # largest d32 / max|g64| 5.3e-07
    "attn-vdn-na8-ne12-a17": (1.18e-07, 8.59e-08, 2.21e-04, 3.349),  # largest d32 / max|g64| 2.5e-07
    "attn-qmix-na1-ne1": (1.37e-07, 8.41e-08, 2.36e-02, 0.694),  # largest d32 / max|g64| 4.1e-07
    "attn-vdn-na1-ne1": (7.32e-08, 3.47e-08, 1.09e-02, 0.3926),  # largest d32 / max|g64| 3.3e-07
    "attn-qmix-k48-a32": (9.06e-08, 5.87e-08, 9.29e-04, 0.3818),  # largest d32 / max|g64| 4.4e-07
    "attn-vdn-k48-a32": (1.11e-07, 7.60e-08, 5.61e-04, 0.7657),  # largest d32 / max|g64| 4.0e-07
    "attn-qmix-nola-a16": (3.55e-07, 5.13e-08, 3.41e-04, 0.6779),  # largest d32 / max|g64| 6.5e-07
    "attn-vdn-nola-a16": (8.93e-08, 7.23e-08, 5.04e-04, 1.42),  # largest d32 / max|g64| 3.2e-07
}
# case -> per tensor (flat parameter order), max|g32 - g64| of the first call's gradients before the clip
GRAD_D32 = {
    "s8-static": (
        6.36e-11, 1.27e-10, 1.24e-10, 1.10e-10, 8.49e-10, 4.49e-10, 1.50e-09, 7.95e-10, 3.24e-10, 2.56e-09, 9.63e-10,
        2.10e-09, 8.35e-09, 8.61e-11, 1.14e-10, 1.13e-10, 1.88e-10, 4.57e-10, 3.36e-10, 1.34e-09, 3.03e-10, 6.56e-10,
        4.33e-10, 4.74e-10, 3.63e-09, 2.54e-09, 8.01e-09, 2.58e-10, 4.38e-10, 5.04e-10, 6.00e-10, 2.74e-09, 1.78e-09,
        4.97e-09, 1.23e-10, 6.83e-10, 2.90e-10, 5.41e-10, 1.62e-09, 4.25e-10, 8.51e-10),
    "s8-generic": (
        6.36e-11, 1.27e-10, 1.24e-10, 1.10e-10, 8.49e-10, 4.49e-10, 1.50e-09, 7.95e-10, 3.24e-10, 2.56e-09, 9.63e-10,
        2.10e-09, 8.35e-09, 8.61e-11, 1.14e-10, 1.13e-10, 1.88e-10, 4.57e-10, 3.36e-10, 1.34e-09, 3.03e-10, 6.56e-10,
        4.33e-10, 4.74e-10, 3.63e-09, 2.54e-09, 8.01e-09, 2.58e-10, 4.38e-10, 5.04e-10, 6.00e-10, 2.74e-09, 1.78e-09,
        4.97e-09, 1.23e-10, 6.83e-10, 2.90e-10, 5.41e-10, 1.62e-09, 4.25e-10, 8.51e-10),
    "na8-ne12-a17": (
        3.68e-10, 2.94e-10, 3.13e-10, 4.91e-10, 1.80e-09, 8.85e-10, 2.89e-09, 1.85e-09, 7.01e-10, 5.56e-09, 3.73e-09,
        3.77e-09, 1.55e-08, 2.42e-10, 5.68e-10, 3.99e-10, 4.48e-10, 2.13e-09, 2.04e-09, 5.40e-09, 5.48e-10, 9.24e-10,
        1.05e-09, 1.35e-09, 7.08e-09, 3.74e-09, 2.10e-08, 1.27e-09, 1.31e-09, 1.22e-09, 1.82e-09, 4.28e-09, 3.68e-09,
        9.95e-09, 2.16e-10, 4.36e-10, 6.40e-10, 3.83e-10, 2.46e-09, 6.10e-10, 2.03e-10),
    "na8-ne8-d16": (
        1.69e-10, 4.84e-10, 3.88e-10, 4.56e-10, 1.17e-09, 6.06e-10, 3.72e-09, 1.44e-09, 5.81e-10, 4.54e-09, 1.99e-09,
        2.16e-09, 1.36e-08, 1.56e-10, 4.57e-10, 5.66e-10, 2.65e-10, 1.35e-09, 7.64e-10, 3.10e-09, 5.21e-10, 9.47e-10,
        1.12e-09, 1.08e-09, 4.14e-09, 2.86e-09, 8.67e-09, 5.76e-10, 7.48e-10, 1.83e-09, 1.52e-09, 4.62e-09, 1.99e-09,
        1.02e-08, 2.26e-10, 3.23e-10, 3.38e-10, 4.23e-10, 1.30e-09, 2.37e-10, 1.26e-10),
    "na7-ne16": (
        6.80e-11, 1.43e-10, 8.03e-11, 1.20e-10, 6.21e-10, 3.47e-10, 1.03e-09, 4.65e-10, 2.45e-10, 1.76e-09, 1.18e-09,
        1.41e-09, 7.44e-09, 1.32e-10, 2.60e-10, 3.23e-10, 3.57e-10, 9.31e-10, 4.69e-10, 2.30e-09, 2.44e-10, 6.04e-10,
        4.34e-10, 5.69e-10, 4.22e-09, 1.43e-09, 5.07e-09, 1.93e-10, 7.22e-10, 4.02e-10, 5.81e-10, 2.43e-09, 1.40e-09,
        6.59e-09, 1.34e-10, 4.32e-10, 2.87e-10, 4.39e-10, 2.05e-09, 3.15e-10, 1.01e-09),
    "na1-ne1": (
        2.25e-10, 2.25e-10, 2.61e-10, 2.33e-10, 1.03e-09, 6.32e-10, 1.60e-09, 7.89e-10, 2.74e-10, 3.24e-09, 1.19e-09,
        5.57e-09, 8.10e-09, 3.70e-10, 3.95e-10, 3.70e-10, 3.63e-10, 1.63e-09, 1.03e-09, 4.13e-09, 5.16e-09, 6.32e-09,
        7.25e-09, 5.43e-09, 1.31e-08, 7.75e-09, 2.64e-08, 3.76e-09, 3.94e-09, 3.75e-09, 3.42e-09, 8.46e-09, 8.26e-09,
        2.04e-08, 6.55e-10, 8.25e-10, 1.26e-09, 1.47e-09, 2.63e-09, 9.90e-10, 9.24e-11),
    "na1-ne16": (
        3.28e-11, 6.92e-11, 6.24e-11, 5.17e-11, 2.66e-10, 2.09e-10, 6.27e-10, 2.56e-10, 9.12e-11, 7.85e-10, 5.61e-10,
        8.68e-10, 2.68e-09, 5.04e-11, 9.87e-11, 7.59e-11, 4.65e-11, 3.87e-10, 2.55e-10, 9.19e-10, 7.48e-10, 1.25e-09,
        7.61e-10, 8.27e-10, 4.65e-09, 1.89e-09, 8.76e-09, 5.04e-10, 8.73e-10, 1.10e-09, 9.52e-10, 3.39e-09, 2.37e-09,
        9.68e-09, 2.54e-10, 3.69e-10, 2.16e-10, 2.28e-10, 7.51e-10, 2.04e-10, 4.52e-10),
    "k48-a32": (
        1.13e-10, 1.87e-10, 1.11e-10, 9.17e-11, 6.16e-10, 2.14e-10, 1.21e-09, 7.01e-10, 3.19e-10, 2.72e-09, 1.79e-09,
        2.38e-09, 7.90e-09, 1.07e-10, 1.26e-10, 1.40e-10, 8.82e-11, 8.99e-10, 2.40e-10, 1.62e-09, 4.04e-10, 7.83e-10,
        5.95e-10, 9.32e-10, 2.81e-09, 1.90e-09, 8.24e-09, 6.52e-10, 1.07e-09, 1.22e-09, 2.12e-09, 3.50e-09, 3.57e-09,
        7.77e-09, 2.53e-10, 3.19e-10, 3.80e-10, 5.03e-10, 1.31e-09, 5.71e-10, 5.90e-10),
    "k33": (
        1.43e-11, 3.06e-11, 4.35e-11, 3.03e-11, 1.06e-10, 6.40e-11, 2.43e-10, 1.29e-10, 6.11e-11, 5.84e-10, 2.46e-10,
        2.88e-10, 1.19e-09, 2.38e-13, 9.83e-13, 3.69e-13, 2.49e-13, 2.14e-12, 1.11e-12, 6.31e-12, 3.21e-11, 4.56e-11,
        3.99e-11, 4.96e-11, 4.13e-10, 1.17e-10, 3.99e-10, 2.78e-10, 5.33e-10, 6.35e-10, 4.08e-10, 3.53e-09, 1.20e-09,
        4.50e-09, 2.82e-10, 5.45e-10, 4.35e-10, 5.50e-10, 4.41e-09, 6.59e-10, 7.28e-10),
    "nola-a16": (
        8.13e-11, 2.03e-10, 1.96e-10, 2.21e-10, 6.55e-10, 5.56e-10, 1.63e-09, 7.37e-10, 3.77e-10, 4.32e-09, 1.91e-09,
        1.61e-09, 8.68e-09, 1.23e-10, 2.42e-10, 2.57e-10, 2.46e-10, 8.55e-10, 6.72e-10, 1.55e-09, 4.71e-10, 8.53e-10,
        1.19e-09, 2.40e-09, 3.90e-09, 5.09e-09, 1.70e-08, 3.96e-10, 1.79e-09, 1.05e-09, 1.80e-09, 3.13e-09, 5.50e-09,
        1.62e-08, 1.89e-10, 4.42e-10, 6.17e-10, 1.36e-09, 2.00e-09, 6.35e-10, 1.68e-09),
    "b33": (
        1.90e-11, 3.01e-11, 2.33e-11, 2.82e-11, 2.14e-10, 1.08e-10, 5.03e-10, 1.70e-10, 6.28e-11, 7.36e-10, 3.72e-10,
        4.93e-10, 3.40e-09, 5.71e-11, 1.28e-10, 1.56e-10, 9.36e-11, 3.78e-10, 2.43e-10, 6.08e-10, 1.92e-10, 2.92e-10,
        4.76e-10, 4.63e-10, 1.80e-09, 7.24e-10, 2.40e-09, 1.46e-10, 3.32e-10, 3.31e-10, 3.75e-10, 1.05e-09, 6.93e-10,
        3.57e-09, 1.07e-10, 1.07e-10, 1.72e-10, 2.22e-10, 4.45e-10, 1.33e-10, 3.70e-10),
    "t130": (
        3.08e-11, 4.91e-11, 4.56e-11, 9.41e-11, 3.58e-10, 2.47e-10, 6.25e-10, 8.22e-10, 4.13e-10, 2.83e-09, 2.62e-09,
        1.28e-09, 2.74e-09, 7.04e-11, 1.05e-10, 8.79e-11, 1.20e-10, 4.87e-10, 2.68e-10, 7.20e-10, 3.36e-10, 6.10e-10,
        9.69e-10, 1.31e-09, 1.81e-09, 3.01e-09, 3.15e-09, 3.60e-10, 5.96e-10, 1.75e-09, 1.81e-09, 3.07e-09, 3.25e-09,
        6.27e-09, 1.25e-10, 2.09e-10, 3.09e-10, 6.23e-10, 8.19e-10, 4.31e-10, 7.05e-10),
    "twords": (
        2.93e-11, 5.26e-11, 5.02e-11, 9.83e-11, 2.68e-10, 1.44e-10, 4.68e-10, 2.88e-10, 1.93e-10, 1.87e-09, 7.35e-10,
        8.76e-10, 2.22e-09, 3.98e-11, 7.11e-11, 6.14e-11, 7.92e-11, 4.25e-10, 1.33e-10, 3.76e-10, 2.66e-10, 4.73e-10,
        5.78e-10, 5.27e-10, 1.14e-09, 1.73e-09, 2.18e-09, 2.49e-10, 4.72e-10, 7.72e-10, 9.69e-10, 1.87e-09, 1.32e-09,
        2.70e-09, 1.38e-10, 1.98e-10, 2.45e-10, 4.26e-10, 5.81e-10, 1.68e-10, 1.25e-10),
    "na7-ne16-clip": (
        7.46e-09, 1.63e-08, 1.11e-08, 1.47e-08, 9.24e-08, 5.82e-08, 2.34e-07, 6.77e-08, 2.96e-08, 2.48e-07, 1.46e-07,
        1.53e-07, 6.96e-07, 2.19e-10, 4.58e-10, 2.80e-10, 3.15e-10, 1.83e-09, 6.72e-10, 4.51e-09, 2.32e-09, 7.08e-09,
        5.01e-09, 4.47e-09, 2.35e-08, 1.40e-08, 5.03e-08, 5.72e-08, 1.70e-07, 9.86e-08, 1.96e-07, 3.78e-07, 1.98e-07,
        7.22e-07, 1.02e-07, 1.41e-07, 1.02e-07, 1.18e-07, 6.18e-07, 6.76e-08, 9.68e-08),
    "k48-a32-clip": (
        1.03e-08, 1.58e-08, 1.30e-08, 1.03e-08, 6.64e-08, 2.35e-08, 2.01e-07, 7.48e-08, 4.27e-08, 3.20e-07, 1.44e-07,
        1.76e-07, 9.56e-07, 9.96e-09, 1.34e-08, 1.27e-08, 9.48e-09, 1.11e-07, 3.09e-08, 2.02e-07, 4.48e-08, 9.86e-08,
        6.64e-08, 1.22e-07, 3.48e-07, 1.91e-07, 6.52e-07, 7.51e-08, 1.79e-07, 7.80e-08, 2.00e-07, 5.48e-07, 2.76e-07,
        1.35e-06, 2.92e-08, 6.33e-08, 3.68e-08, 5.26e-08, 1.74e-07, 4.30e-08, 9.26e-08),
    "attn-qmix-na8-ne12-a17": (
        1.34e-10, 3.00e-10, 5.28e-10, 5.37e-10, 1.46e-09, 9.42e-10, 3.14e-09, 1.11e-09, 5.65e-10, 4.47e-09, 3.10e-09,
        2.54e-09, 7.50e-09, 2.04e-10, 4.45e-10, 5.78e-10, 6.01e-10, 2.29e-09, 2.05e-09, 4.33e-09, 7.44e-10, 1.18e-09,
        1.35e-09, 1.76e-09, 8.02e-09, 3.75e-09, 1.76e-08, 1.04e-09, 1.83e-09, 2.00e-09, 2.36e-09, 6.09e-09, 3.65e-09,
        9.29e-09, 3.38e-10, 5.74e-10, 6.70e-10, 6.26e-10, 2.88e-09, 4.40e-10, 9.85e-10),
    "attn-vdn-na8-ne12-a17": (
        8.88e-10, 2.52e-09, 2.82e-09, 4.64e-09, 1.17e-08, 9.33e-09, 2.35e-08, 9.37e-09, 3.23e-09, 4.41e-08, 1.54e-08,
        1.89e-08, 7.65e-08),
    "attn-qmix-na1-ne1": (
        1.83e-10, 1.89e-10, 1.81e-10, 1.65e-10, 5.74e-10, 3.99e-10, 1.44e-09, 2.97e-10, 1.49e-10, 1.31e-09, 9.49e-10,
        1.61e-09, 4.44e-09, 2.88e-10, 3.61e-10, 3.65e-10, 1.92e-10, 7.87e-10, 3.44e-10, 1.45e-09, 6.18e-09, 6.42e-09,
        5.57e-09, 2.81e-09, 1.20e-08, 8.10e-09, 2.63e-08, 4.28e-09, 5.47e-09, 4.08e-09, 2.81e-09, 1.33e-08, 7.79e-09,
        2.67e-08, 1.08e-09, 1.37e-09, 1.82e-09, 9.01e-10, 2.32e-09, 7.29e-10, 8.36e-10),
    "attn-vdn-na1-ne1": (
        3.41e-10, 6.78e-10, 5.36e-10, 3.17e-10, 2.42e-09, 8.18e-10, 5.47e-09, 1.34e-09, 4.37e-10, 4.93e-09, 2.47e-09,
        4.00e-09, 1.68e-08),
    "attn-qmix-k48-a32": (
        1.40e-10, 1.54e-10, 1.17e-10, 1.42e-10, 4.85e-10, 3.47e-10, 1.16e-09, 3.37e-10, 2.08e-10, 2.55e-09, 8.49e-10,
        1.87e-09, 4.77e-09, 9.76e-11, 2.35e-10, 1.93e-10, 1.49e-10, 6.01e-10, 3.00e-10, 1.32e-09, 5.97e-10, 8.56e-10,
        8.22e-10, 1.14e-09, 5.87e-09, 2.27e-09, 5.95e-09, 1.01e-09, 2.03e-09, 8.65e-10, 2.03e-09, 7.70e-09, 4.48e-09,
        6.54e-09, 3.13e-10, 4.59e-10, 4.80e-10, 5.79e-10, 2.02e-09, 6.71e-10, 1.36e-09),
    "attn-vdn-k48-a32": (
        5.70e-10, 7.15e-10, 5.37e-10, 8.95e-10, 4.67e-09, 1.54e-09, 7.09e-09, 3.78e-09, 1.29e-09, 1.50e-08, 5.92e-09,
        7.00e-09, 2.17e-08),
    "attn-qmix-nola-a16": (
        1.05e-10, 1.92e-10, 3.76e-10, 6.41e-10, 8.55e-10, 1.22e-09, 2.82e-09, 7.35e-10, 4.00e-10, 3.69e-09, 1.56e-09,
        3.65e-09, 1.13e-08, 1.47e-10, 2.71e-10, 4.08e-10, 3.90e-10, 1.26e-09, 6.17e-10, 1.59e-09, 6.54e-10, 1.23e-09,
        2.51e-09, 5.16e-09, 8.56e-09, 7.13e-09, 9.47e-09, 6.38e-10, 2.33e-09, 6.32e-09, 6.39e-09, 9.05e-09, 1.73e-08,
        1.56e-08, 3.67e-10, 1.17e-09, 1.34e-09, 2.32e-09, 3.11e-09, 1.15e-09, 2.55e-09),
    "attn-vdn-nola-a16": (
        6.53e-10, 1.22e-09, 1.18e-09, 1.80e-09, 4.26e-09, 3.69e-09, 5.70e-09, 6.35e-09, 1.72e-09, 2.14e-08, 9.48e-09,
        9.57e-09, 4.55e-08),
}


def bounds(cid):
    """(statistic rtol, statistic atol, parameter atol): this learner's, or ten times the fp32 oracle's own distance
    from float64 where that is larger (nowhere, with the figures above)."""
    s, p = ORACLE_F64[cid][:2]
    k = max(1.0, 10 * s / STAT_RTOL)
    return STAT_RTOL * k, STAT_ATOL * k, max(PARAM_ATOL, 10 * p)


def grad_bounds(cid, g64):
    """Per tensor: max(1e-4 max|g64|, 10 d32): the project's 1e-4 parity bound relative to the tensor's own scale
    (a first RMSprop step hides the magnitude; max|g| runs from 3e-4 to 1e-1 here, so max(1, max|g|) would be
    vacuous), or ten times the fp32 oracle's distance from float64 on that tensor."""
    d32 = GRAD_D32[cid]
    assert len(d32) == len(g64)
    return [max(GRAD_RTOL * float(np.abs(np.asarray(g)).max()), 10 * d) for g, d in zip(g64, d32)]


def clips(cid):
    return ORACLE_F64[cid][3] > CLIP
