"""The shape cases of the stand-alone DRQN and QMixer entry points (csrc/agent.hip, csrc/agent_grad.hip) off the
5-agent, A = 15, H = 64, S = 60 fixture, shared by tests/test_drqn_op_shapes.py (CPU: the conditions on the oracle's
values and the host-side size queries) and tests/test_gpu_drqn_ops.py (GPU: parity with the float64 oracle).

Plain data and seeded numpy / torch-CPU builders; nothing here touches a kernel. Every builder is a function of the
case and its recorded seed alone, so both files see the same inputs.

The conditions the seeds were chosen for (on the CPU, on the oracle's values, never on a kernel's):
  1. gradient cases: every ReLU / abs argument further from zero than 8 eps32 (|w| . |x| + |b|)
     (test_gpu_autograd._clear_of_kinks through agent_reference / mixer_reference with check=True);
  2. gradient cases: the fc1 pre-activation and the ELU argument take both signs;
  3. every case: the fp32 CPU oracle lies within a quarter of the bound 1e-4 max(1, max|y64|) of the float64 one, per
     tensor, so a kernel summing in another order keeps three quarters of the bound;
  4. the exact-tie rows of the selection cases are made by copying one Q value into another available slot.
Seed scan: the first seed >= 1 that meets 1-3 (MIXER_SEEDS, AGENT_GRAD_SEEDS hold the ones that are not 1).
"""
from collections import namedtuple

import numpy as np
import torch

import rollout_shapes as RS

F64 = torch.float64
BOUND = 1e-4            # the project's fp32 parity bound, times max(1, max|reference|), per tensor
ORACLE_SHARE = 0.25     # condition 3


def bound_of(ref64):
    return BOUND * max(1.0, float(ref64.detach().abs().max())) if ref64.numel() else BOUND


def to64(d):
    return {k: v.to(F64) for k, v in d.items()}


# ---- A. mlg_agent_forward -------------------------------------------------------------------------------------------
# d_obs = 48, N = 3, both flags on: d_in = 51 + A is no multiple of 16 for A = 5, 16, 17 (64 + 52 at A = 65 is not
# either). A: below one 16-wide action tile, exactly one, one past, five tiles. R: one row, one below / exactly / one
# past a 16-row tile, one past two tiles, one past a 4-tile workgroup.
FWD_D_OBS, FWD_N = 48, 3
FWD_H = (32, 64, 128)
FWD_A = (5, 16, 17, 65)
FWD_R = (1, 15, 16, 17, 33, 65)
FWD_R_NULL = 17  # the row count of the h_in = NULL call of every (H, A)


def fwd_d_in(A):
    return FWD_D_OBS + A + FWD_N


def fwd_params(H, A):
    """torch-default weight ranges (rollout_shapes.agent_params), seeded by the case."""
    return {k: torch.from_numpy(v) for k, v in RS.agent_params(fwd_d_in(A), H, A, 100 + H + A).items()}


def fwd_inputs(H, A):
    """[(R, x [R, d_in], h_in [R, H] or None)]: a random hidden state per R of FWD_R, then the h_in = NULL call."""
    g = torch.Generator().manual_seed(7000 + H + A)
    out = [(R, torch.randn(R, fwd_d_in(A), generator=g), torch.randn(R, H, generator=g) * 0.7) for R in FWD_R]
    out.append((FWD_R_NULL, torch.randn(FWD_R_NULL, fwd_d_in(A), generator=g), None))
    return out


def fwd_reference(p, x, h, dtype):
    import learner_ref as LR
    H = p["gru.weight_hh"].shape[1]
    hh = torch.zeros(x.shape[0], H, dtype=dtype) if h is None else h.to(dtype)
    with torch.no_grad():
        return LR.drqn_forward({k: v.to(dtype) for k, v in p.items()}, x.to(dtype), hh)


# ---- B. mlg_mac_forward ---------------------------------------------------------------------------------------------
MacCase = namedtuple("MacCase", "id H A N B last_action agent_id")
MAC_D_OBS, MAC_T1 = 48, 4
MAC_CASES = [MacCase(*c) for c in [
    ("h64-both", 64, 15, 3, 11, True, True),          # B N = 33: two tiles and one row
    ("h32-no-last-action", 32, 15, 3, 5, False, True),  # 15 rows: w1a absent from the packed block
    ("h128-no-agent-id", 128, 15, 3, 6, True, False),   # 18 rows: w1n absent
    ("h64-obs-only", 64, 15, 4, 4, False, False),       # 16 rows, d_in = d_obs: neither gathered block
    ("a23-n9", 64, 23, 9, 7, True, True),               # 63 rows: a ragged fourth tile, two action tiles
    ("a65-n7", 32, 65, 7, 5, True, True),               # 35 rows, five action tiles
]]
MAC_IDS = [c.id for c in MAC_CASES]
MAC_ROWS = {"h64-both": 33, "h32-no-last-action": 15, "h128-no-agent-id": 18, "h64-obs-only": 16, "a23-n9": 63,
            "a65-n7": 35}
SAMPLED_ROWS = [12, 0, 7, 7, 3, 11]  # episode b of the view sits in slot SAMPLED_ROWS[b] of a 13-slot buffer
SAMPLED_SLOTS = 13
MODULE_PATH_CASE = "h32-no-last-action"  # the case that also goes through BasicMAC.forward


def mac_case(cid):
    return next(c for c in MAC_CASES if c.id == cid)


def mac_d_in(c):
    return MAC_D_OBS + (c.A if c.last_action else 0) + (c.N if c.agent_id else 0)


def mac_params(c):
    return {k: torch.from_numpy(v) for k, v in RS.agent_params(mac_d_in(c), c.H, c.A, 200 + c.H + c.N).items()}


def mac_batch(slots, T1, N, A, d_obs, seed):
    """obs and the one-hot of random actions, [slots, T1, N, ...] float32."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(slots, T1, N, d_obs, generator=g)
    acts = torch.randint(0, A, (slots, T1, N), generator=g)
    return {"obs": obs, "actions_onehot": torch.zeros(slots, T1, N, A).scatter_(3, acts.unsqueeze(-1), 1.0)}


def mac_inputs(c, slots=None):
    """-> (batch, h0 [slots N, H]): a random initial hidden state, so that t = 0 reads h_in as well."""
    slots = c.B if slots is None else slots
    tb = mac_batch(slots, MAC_T1, c.N, c.A, MAC_D_OBS, 300 + c.H + c.N)
    g = torch.Generator().manual_seed(400 + c.H + c.N)
    return tb, torch.randn(slots * c.N, c.H, generator=g) * 0.7


def mac_reference(c, p, tb, h0, dtype):
    """-> (q [B, T1, N, A], the hidden state after the last step)."""
    import learner_ref as LR
    with torch.no_grad():
        return LR.mac_unroll({k: v.to(dtype) for k, v in p.items()}, {k: v.to(dtype) for k, v in tb.items()}, c.N,
                             h0=h0.to(dtype), last_action=c.last_action, agent_id=c.agent_id)


# ---- C. mlg_qmix_forward / mlg_qmix_backward ------------------------------------------------------------------------
MixerCase = namedtuple("MixerCase", "id N S E HE layers")
MIXER_CASES = [MixerCase(*c) for c in [
    ("n1", 1, 17, 32, 64, 2),          # one agent; state rows no 16-byte multiples: scalar x loads (BJob::vb off)
    ("e5", 3, 37, 5, 7, 2),            # no leading dimension a multiple of 4: va and vb off, every section padded
    ("e64-he256", 9, 60, 64, 256, 2),  # both limits of check_qmix_dims; 9 x 4 output blocks; E fills the wave
    ("n32", 32, 132, 32, 64, 2),       # the largest team: N E = 1024, 16 output blocks
    ("l1-n17-e16", 17, 91, 16, 0, 1),  # one-layer hypernets, M = 272 over an odd S
    ("l1-e64", 2, 8, 64, 0, 1),        # S below one 16-wide step
]]
MIXER_IDS = [c.id for c in MIXER_CASES]
MIXER_R = (1, 65, 257)  # one row, one past a 64-row chunk, one past a group of four chunks
MIXER_SEEDS = {("e5", 257): 2, ("e64-he256", 257): 3}  # (id, R) -> seed where it is not 1 (a hypernet argument at a kink)


def mixer_case_of(cid):
    return next(c for c in MIXER_CASES if c.id == cid)


def mixer_seed(cid, R):
    return MIXER_SEEDS.get((cid, R), 1)


def mixer_inputs(c, R, seed=None):
    """Parameters in torch's default ranges U(+-1 / sqrt(fan_in)) under QMixer's state_dict names, agent_qs 1.5 N(0, 1)
    (both signs, so the ELU argument takes both), states N(0, 1), and the upstream gradient of q_tot."""
    seed = mixer_seed(c.id, R) if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    mp = {}

    def lin(name, o, i):
        k = 1.0 / np.sqrt(i)
        mp[f"{name}.weight"] = (torch.rand(o, i, generator=g) * 2 - 1) * k
        mp[f"{name}.bias"] = (torch.rand(o, generator=g) * 2 - 1) * k

    if c.layers == 2:
        lin("hyper_w_1.0", c.HE, c.S), lin("hyper_w_1.2", c.N * c.E, c.HE)
        lin("hyper_w_final.0", c.HE, c.S), lin("hyper_w_final.2", c.E, c.HE)
    else:
        lin("hyper_w_1", c.N * c.E, c.S), lin("hyper_w_final", c.E, c.S)
    lin("hyper_b_1", c.E, c.S), lin("V.0", c.E, c.S), lin("V.2", 1, c.E)
    return (mp, torch.randn(R, c.N, generator=g) * 1.5, torch.randn(R, c.S, generator=g),
            torch.randn(R, generator=g))


def mixer_forward_reference(c, mp, qs, st, dtype):
    import learner_ref as LR
    R = qs.shape[0]
    with torch.no_grad():
        return LR.qmix_forward({k: v.to(dtype) for k, v in mp.items()}, qs.to(dtype).view(R, 1, c.N),
                               st.to(dtype).view(R, 1, c.S), c.N, c.E, c.layers).view(R)


def mixer_param_count(c):
    if c.layers == 2:
        hyper = c.HE * c.S + c.HE + c.N * c.E * c.HE + c.N * c.E + c.HE * c.S + c.HE + c.E * c.HE + c.E
    else:
        hyper = c.N * c.E * c.S + c.N * c.E + c.E * c.S + c.E
    return hyper + 2 * (c.E * c.S + c.E) + c.E + 1


# ---- D. mlg_agent_backward: the added edges -------------------------------------------------------------------------
# d_obs = 80, N = 5 as in tests/test_gpu_autograd.py. Weight-gradient chunks are at least 64 rows long and go four to a
# group: R = 64 / 65 is the first chunk edge, 257 one past a group.
AgentGradCase = namedtuple("AgentGradCase", "id R H A last_action agent_id")
GRAD_D_OBS, GRAD_N = 80, 5
AGENT_GRAD_CASES = [AgentGradCase(*c) for c in [
    ("r64", 64, 64, 15, True, True), ("r65", 65, 64, 15, True, True), ("r257", 257, 64, 15, True, True),
    ("h32-r65", 65, 32, 15, True, True), ("h128-r65", 65, 128, 15, True, True),
    ("a5", 37, 64, 5, True, True), ("a16", 37, 64, 16, True, True), ("a65", 37, 64, 65, True, True),
    ("no-last-action", 37, 64, 15, False, True), ("no-agent-id", 37, 64, 15, True, False),
    ("obs-only", 37, 64, 15, False, False),
]]
AGENT_GRAD_IDS = [c.id for c in AGENT_GRAD_CASES]
AGENT_GRAD_SEEDS = {}  # id -> seed where it is not 1


def agent_grad_case_of(cid):
    return next(c for c in AGENT_GRAD_CASES if c.id == cid)


def agent_grad_d_in(c):
    return GRAD_D_OBS + (c.A if c.last_action else 0) + (GRAD_N if c.agent_id else 0)


def agent_grad_inputs(c, seed=None):
    """test_gpu_autograd.agent_case at the case's input width: (parameters, x, h, gq, gh)."""
    from test_gpu_autograd import agent_case
    seed = AGENT_GRAD_SEEDS.get(c.id, 1) if seed is None else seed
    return agent_case(c.R, c.H, c.A, seed, d_in=agent_grad_d_in(c))


# ---- E. direct backward calls into poisoned buffers -----------------------------------------------------------------
POISON_MIXER, POISON_AGENT, POISON_R = "e5", "r65", 65
CANARY_FLOATS = 1024  # the tail behind the workspace; its pattern must survive the call


# ---- F. mlg_select_actions ------------------------------------------------------------------------------------------
GREEDY_SHAPES = [(1, 1, 1), (3, 5, 7), (60, 5, 15), (9, 32, 33)]  # (B, N, A); 300 and 288 rows: two 256-thread blocks
EPS_SHAPES = [(60, 5, 15), (9, 32, 33)]
EPS_VALUES = (0.6, 1.0)
EPS_T = (0, 29)
KEY_HIGH = 0xC0FFEE11  # the keys' high word: bit 63 set


def select_case(B, N, A, masked_row=True):
    """q, avail (about 40 % available, action A // 2 always) with, where the shape has room for them: rows with an
    exact tie at the maximum between two available slots (the copy placed below the argmax on even tie rows, above it
    on odd ones), rows whose largest Q is unavailable, and one fully masked row. -> (q, avail, {kind: row indices})."""
    import learner_ref as LR
    rng = np.random.RandomState(1000 * B + 10 * N + A)
    q = rng.randn(B, N, A).astype(np.float32)
    av = (rng.rand(B, N, A) < 0.4).astype(np.int32)
    av[..., A // 2] = 1
    R = B * N
    qf, af = q.reshape(R, A), av.reshape(R, A)
    rows = {"tie": [], "max_unavailable": [], "masked": []}
    if A >= 3 and R >= 8:
        picks = rng.permutation(R)
        n_special = max(2, R // 10)
        g = LR.greedy_select(torch.from_numpy(q), torch.from_numpy(av)).numpy().reshape(R)
        for i, r in enumerate(picks[:n_special]):  # condition 4: the tie is a copy, not a search
            others = [a for a in range(A) if a != g[r]]
            below = [a for a in others if a < g[r]]
            above = [a for a in others if a > g[r]]
            pool = (below or above) if i % 2 == 0 else (above or below)
            j = int(pool[rng.randint(len(pool))])
            af[r, j] = 1
            qf[r, j] = qf[r, g[r]]
            rows["tie"].append(int(r))
        for r in picks[n_special:2 * n_special]:
            k = int(rng.choice([a for a in range(A) if a != A // 2]))
            af[r, k] = 0
            qf[r, k] = np.float32(np.abs(qf[r]).max() + 5.0)
            rows["max_unavailable"].append(int(r))
        if masked_row:
            r = int(picks[2 * n_special])
            af[r] = 0
            rows["masked"].append(r)
    return q, av, rows


def select_keys(B):
    keys = np.array([(KEY_HIGH << 32) + 17 * b for b in range(B)], np.uint64)
    episodes = (np.arange(B, dtype=np.int64) * 7 + 3) % 11
    return keys, episodes.astype(np.int32)
