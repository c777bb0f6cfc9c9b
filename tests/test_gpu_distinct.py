"""GPU parity of distinct per-agent networks (mac: distinct): mlg_mac_forward_distinct and DistinctMAC's differentiable
path against the float64 oracle (tests/distinct_ref.py, pinned to the reference's golden by tests/test_distinct.py),
and mlg_rollout_distinct per dispatch arm and edge by the method of tests/test_gpu_dqn.py.

Bounds: Q and h within 1e-4 max(1, max|ref|) of the float64 oracle; every gradient tensor within 1e-4 of the float64
reference tensor's largest element. Each check prints its error next to its bound (`pytest -s`). Rollout: env tensors
bit-exact against the C env under teacher forcing, random picks those of the counter RNG, every greedy pick the float64
oracle's argmax except at a near tie (top-two masked Q within 1e-4), near ties accepted for at most 1 % of a case's
greedy picks (tests/distinct_shapes.py holds the cases and the oracle's own share). With N equal networks a run
stores, bit for bit, what a BasicMAC run stores on the generic fp32 kernel.
"""
import numpy as np
import pytest
import torch

import distinct_ref as DR
import distinct_shapes as DS
import helpers
from helpers import qmix_args, scheme_for, shape_plan

pytestmark = pytest.mark.gpu

F64 = torch.float64
NEAR_TIE_CAP = 0.01
D_OBS, A = 48, 11  # the 3v3 plan's obs width and action count: d_in = 59, no multiple of 16


def _bound_check(name, got, ref64):
    err = float((got.detach().cpu().to(F64) - ref64).abs().max())
    bound = 1e-4 * max(1.0, float(ref64.abs().max()))
    print(f"  {name:44s} err {err:.3e}  bound {bound:.3e}  ({100 * err / bound:.1f} %)")
    assert err <= bound, (name, err, bound)


def _episode_batch(device, args, tb, B, T1):
    from maleague.components.episode_batch import EpisodeBatch
    info = {"state_shape": args.state_shape, "obs_shape": tb["obs"].shape[-1], "n_actions": args.n_actions,
            "n_agents": args.n_agents}
    scheme, groups, preprocess = scheme_for(info, torch)
    batch = EpisodeBatch(scheme, groups, B, T1, preprocess=preprocess, device=device)
    batch.data.transition_data["obs"].copy_(tb["obs"])
    batch.data.transition_data["actions_onehot"].copy_(tb["actions_onehot"])
    return batch, scheme, groups


def _mac(device, N, H, last_action=True, seed=3, d_obs=D_OBS, n_actions=A):
    """A DistinctMAC on the device with the N seeded, different networks of distinct_ref.agent_params."""
    from maleague.controllers import DistinctMAC
    args = qmix_args(n_agents=N, n_actions=n_actions, rnn_hidden_dim=H, obs_last_action=last_action,
                     obs_agent_id=False, mac="distinct", device=str(device), state_shape=36)
    info = {"state_shape": 36, "obs_shape": d_obs, "n_actions": n_actions, "n_agents": N}
    scheme, groups, _ = scheme_for(info, torch)
    from maleague.components.episode_batch import EpisodeBatch
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=scheme_for(info, torch)[2], device=device)
    mac = DistinctMAC(proto.scheme, groups, args)
    ps = DR.all_agent_params(N, mac.input_shape, H, n_actions, seed)
    DR.load_agents(mac, ps)
    return mac, args, [{k: torch.from_numpy(v) for k, v in p.items()} for p in ps]


def _raw_batch(slots, T1, N, seed, d_obs=D_OBS, n_actions=A):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(slots, T1, N, d_obs, generator=g)
    acts = torch.randint(0, n_actions, (slots, T1, N), generator=g)
    oh = torch.zeros(slots, T1, N, n_actions).scatter_(3, acts.unsqueeze(-1), 1.0)
    return {"obs": obs, "actions_onehot": oh}


def _forward(device, mac, tb, B, T1, t, h_in, rows=None):
    """mlg_mac_forward_distinct called directly into NaN-filled q / h_out."""
    from maleague import _native
    dev = {k: v.to(device).contiguous() for k, v in tb.items()}
    rows_d = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=device)
    mb = _native.MlgBatch(None, dev["obs"].data_ptr(), None, None, None, None, dev["actions_onehot"].data_ptr(), None,
                          B, T1, 0, 0, 0, None if rows_d is None else rows_d.data_ptr())
    d = mac.dims()
    q = torch.full((B, d.n_agents, d.n_actions), float("nan"), device=device)
    h_out = torch.full((B, d.n_agents, d.hidden), float("nan"), device=device)
    hd = None if h_in is None else h_in.to(device).contiguous()
    _native.call("mlg_mac_forward_distinct", _native.byref(d), _native.ptr(mac.packed()), _native.byref(mb), int(t),
                 None if hd is None else _native.ptr(hd), _native.ptr(q), _native.ptr(h_out), _native.stream_ptr())
    torch.cuda.synchronize()
    return q, h_out


# ---- MAC forward ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,N,B,la", [(32, 1, 33, True), (64, 3, 11, True), (128, 9, 1, True), (64, 9, 33, True),
                                      (32, 3, 1, False), (128, 1, 11, True), (64, 1, 1, True), (32, 9, 11, False)],
                         ids=["h32-n1-b33", "h64-n3-b11", "h128-n9-b1", "h64-n9-b33", "h32-n3-b1-nola",
                              "h128-n1-b11", "h64-n1-b1", "h32-n9-b11-nola"])
def test_mac_forward_matches_float64_oracle(device, H, N, B, la):
    """B = 1 / 11 / 33 against the 16-row tile (one partial tile, three tiles with the last holding one row), N tiles
    per 16 rows; t = 0 (no last action, zero and NULL h_in) and t > 0 from a random hidden state."""
    T1 = 4
    mac, args, ps = _mac(device, N, H, last_action=la)
    tb = _raw_batch(B, T1, N, seed=H + N + B)
    ps64 = [{k: v.double() for k, v in p.items()} for p in ps]
    tb64 = {k: v.double() for k, v in tb.items()}
    g = torch.Generator().manual_seed(B)
    for t, h_in in ((0, None), (0, torch.zeros(B, N, H)), (2, torch.randn(B, N, H, generator=g)),
                    (3, torch.randn(B, N, H, generator=g))):
        q, h = _forward(device, mac, tb, B, T1, t, h_in)
        assert not torch.isnan(q).any() and not torch.isnan(h).any()
        h64 = torch.zeros(B, N, H, dtype=F64) if h_in is None else h_in.double()
        with torch.no_grad():
            q_ref, h_ref = DR.mac_step(ps64, tb64, t, h64, last_action=la)
        _bound_check(f"Q H={H} N={N} B={B} t={t}", q, q_ref)
        _bound_check(f"h H={H} N={N} B={B} t={t}", h, h_ref)


def test_mac_forward_sampled_rows_equal_gathered_copy(device):
    """A sampled view (episode b in slot rows[b] of a larger buffer) gives the bits of its gathered copy."""
    H, N, T1, slots = 64, 3, 4, 13
    mac, args, ps = _mac(device, N, H)
    tb = _raw_batch(slots, T1, N, seed=9)
    rows = [12, 0, 7, 7, 3, 11]
    gathered = {k: v[rows] for k, v in tb.items()}
    h_in = torch.randn(len(rows), N, H, generator=torch.Generator().manual_seed(1))
    for t in (0, 3):
        q_view, h_view = _forward(device, mac, tb, len(rows), T1, t, h_in, rows=rows)
        q_copy, h_copy = _forward(device, mac, gathered, len(rows), T1, t, h_in)
        assert torch.equal(q_view, q_copy) and torch.equal(h_view, h_copy), t
        assert not torch.isnan(q_view).any()


def test_networks_are_isolated(device):
    """Changing network j's weights leaves every other agent's Q and h bit-identical and changes agent j's."""
    H, N, B, T1, j = 64, 3, 33, 3, 1
    mac, args, ps = _mac(device, N, H)
    tb = _raw_batch(B, T1, N, seed=5)
    h_in = torch.randn(B, N, H, generator=torch.Generator().manual_seed(2))
    q0, h0 = _forward(device, mac, tb, B, T1, 2, h_in)
    mac.agents[j].load_state_dict({k: torch.from_numpy(v) for k, v in
                                   DR.agent_params(7, mac.input_shape, H, A, seed=99).items()})
    q1, h1 = _forward(device, mac, tb, B, T1, 2, h_in)
    for i in range(N):
        if i == j:
            assert not torch.equal(q0[:, i], q1[:, i]) and not torch.equal(h0[:, i], h1[:, i])
        else:
            assert torch.equal(q0[:, i], q1[:, i]) and torch.equal(h0[:, i], h1[:, i]), i


# ---- rollout --------------------------------------------------------------------------------------------------------

@pytest.fixture
def distinct_oracle(monkeypatch):
    """helpers.check_run with the per-agent oracle in place of the shared DRQN's (its env replay and pick rules as
    is; check_run reads nothing else of the MAC)."""
    monkeypatch.setattr(helpers, "oracle_q", DR.oracle_q)


def _stepper(device, cid, B=DS.B, shared=False):
    """A ParallelStepper over the case's plan with a DistinctMAC: N different seeded networks, or (shared) N copies
    of network 0."""
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import DistinctMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import ParallelStepper
    _, hidden, plan, la, arm, seed, scale = DS.case(cid)
    args = qmix_args(batch_size_run=B, seed=seed, rnn_hidden_dim=hidden, obs_last_action=la, obs_agent_id=False,
                     mac="distinct", env_args={"match_build_plan": shape_plan(plan), "grid_size": 20,
                                               "stochastic_spawns": True, "episode_limit": DS.EPISODE_LIMIT})
    stepper = ParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"], info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(info, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    mac = DistinctMAC(proto.scheme, groups, args)
    ps = DR.all_agent_params(args.n_agents, mac.input_shape, hidden, args.n_actions, seed, scale)
    DR.load_agents(mac, [ps[0]] * args.n_agents if shared else ps)
    mac.cuda()
    stepper.initialize(scheme, groups, preprocess, mac)
    return stepper, mac, args, arm, ps


def _cap(cid, mode, n):
    print(f"{cid} [{mode}]: {n}  ({100.0 * n['near_ties'] / n['greedy']:.3f} % near ties, cap 1 %)")
    assert n["near_ties"] <= NEAR_TIE_CAP * n["greedy"], (cid, mode, n)


@pytest.mark.parametrize("cid", DS.IDS)
def test_rollout_distinct_parity(device, cid, distinct_oracle):
    stepper, mac, args, arm, _ = _stepper(device, cid)
    name, lds = stepper.describe_rollout()
    print(f"{cid}: arm {name}, {lds} B of LDS, B = {DS.B}, N = {args.n_agents}")
    assert name == arm
    batch, infos = stepper.run(test_mode=True)
    n = helpers.check_run(stepper, mac, args, batch, infos, episode=0, test_mode=True, eps=0.0, dtype=F64)
    _cap(cid, "test", n)
    assert stepper.t_env == 0
    stepper.t_env = DS.T_ENV
    batch, infos = stepper.run(test_mode=False)
    n = helpers.check_run(stepper, mac, args, batch, infos, episode=1, test_mode=False, eps=DS.EPS, dtype=F64)
    _cap(cid, "train", n)
    assert n["epsilon_draws"] > 0
    assert stepper.t_env == DS.T_ENV + int(stepper.last_run["ep_len"].sum())


def _snapshot(stepper, batch):
    stepper.flush()
    out = {k: v.detach().cpu().clone() for k, v in batch.data.transition_data.items()}
    out["ep_len"] = stepper.last_run["ep_len"].clone()
    out["returns"] = stepper.last_run["returns"].clone()
    return out


@pytest.mark.parametrize("cid", DS.SHARED_CASES)
def test_shared_weights_equal_basic_mac_on_the_generic_kernel(device, cid, monkeypatch):
    """All N networks hold the same weights: a test-mode and a train-mode run store, bit for bit, what a BasicMAC
    (obs_agent_id off) with those weights stores under MLG_ROLLOUT_KERNEL=v1 -- actions, one-hot rows, obs, state,
    avail, rewards, terminated, filled, ep_len and returns. A row's arithmetic is agent_device.h's in both tilings
    (an MFMA column depends on its own row only), from global memory here and from the LDS image there."""
    monkeypatch.setenv("MLG_ROLLOUT_KERNEL", "v1")
    _, hidden, plan, la, arm, seed, _ = DS.case(cid)
    stepper, mac, args, _, ps = _stepper(device, cid, shared=True)
    ref_stepper, ref_mac, ref_args = helpers.build_stepper(device, plan=shape_plan(plan), B=DS.B,
                                                           episode_limit=DS.EPISODE_LIMIT, seed=seed,
                                                           rnn_hidden_dim=hidden, obs_agent_id=False, obs_last_action=la)
    ref_mac.agent.load_state_dict({k: torch.from_numpy(v) for k, v in ps[0].items()})
    ref_mac.agent.to(device)
    assert ref_stepper.describe_rollout()[0].startswith("v1-") and stepper.describe_rollout()[0] == arm
    for test_mode in (True, False):
        snaps = []
        for st in (stepper, ref_stepper):
            if not test_mode:
                st.t_env = DS.T_ENV
            batch, _ = st.run(test_mode=test_mode)
            snaps.append(_snapshot(st, batch))
        got, want = snaps
        assert int(want["ep_len"].min()) >= 1
        for k in want:
            assert torch.equal(got[k], want[k]), (cid, test_mode, k)


def test_rollout_distinct_single_env(device, distinct_oracle):
    """B = 1: one live column in every agent tile of a 16-env workgroup."""
    stepper, mac, args, arm, _ = _stepper(device, "dx-n3-h64", B=1)
    batch, infos = stepper.run(test_mode=True)
    helpers.check_run(stepper, mac, args, batch, infos, episode=0, test_mode=True, eps=0.0, dtype=F64)


def test_episode_stepper_goes_the_same_way(device, distinct_oracle):
    """EpisodeStepper (B = 1) with a DistinctMAC reports and runs the distinct arm."""
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import DistinctMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import EpisodeStepper
    args = qmix_args(batch_size_run=1, seed=4, obs_agent_id=False, mac="distinct",
                     env_args={"match_build_plan": "small", "grid_size": 20, "stochastic_spawns": True,
                               "episode_limit": 20})
    stepper = EpisodeStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"], info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(info, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    mac = DistinctMAC(proto.scheme, groups, args)
    DR.load_agents(mac, DR.all_agent_params(3, mac.input_shape, 64, args.n_actions, 4))
    mac.cuda()
    stepper.initialize(scheme, groups, preprocess, mac)
    assert stepper.describe_rollout()[0] == "dx-global/tpw1"
    batch, info = stepper.run(test_mode=True)
    assert set(info) == {"battle_won", "draw"}
    helpers.check_run(stepper, mac, args, batch, [info], episode=0, test_mode=True, eps=0.0, dtype=F64)


@pytest.mark.parametrize("cid", DS.RING_CASES)
def test_rollout_distinct_ring_mode_equals_plain_run(device, cid):
    """A train-mode run written straight into replay slots pre-filled with other bytes (full-write mode, wrapping
    around the ring's end) equals the plain run into a zero-initialised batch byte for byte; slot extents follow.
    The plain run repeated from the same state gives the same bits (two runs are bit-identical)."""
    from maleague.components.replay_buffer import ReplayBuffer
    from maleague.envs.teams_env import VecEnvState
    stepper, mac, args, arm, _ = _stepper(device, cid)
    assert stepper.describe_rollout()[0] == arm
    scheme, groups, preprocess = scheme_for(stepper.get_env_info(), torch)
    size = DS.B + 5
    ring = ReplayBuffer(scheme, groups, size, DS.EPISODE_LIMIT + 1, preprocess=preprocess, device=device)
    for v in ring.data.transition_data.values():
        v.fill_(7)
    for it in range(2):  # slots 0..36, then 37..41 and 0..31 (wraps)
        runs = []
        for use_ring in (False, False, True):
            st = VecEnvState(stepper.spec, DS.B, device)
            st.episode.fill_(it)
            stepper.envs = st
            stepper.t_env = DS.T_ENV
            stepper._ring = None
            if use_ring:
                assert stepper.attach_replay(ring)
            runs.append(stepper.run(test_mode=False)[0])
        b_plain, b_again, b_ring = runs
        for k in b_plain.data.transition_data:
            assert torch.equal(b_plain[k], b_again[k]), (cid, it, k)
            assert torch.equal(b_plain[k], b_ring[k]), (cid, it, k)
        ring.insert_episode_batch(b_ring)
        slots = (torch.arange(DS.B) + b_ring.slot0) % size
        want = (stepper.last_run["ep_len"] + 1).to(torch.int32)
        assert torch.equal(ring.slot_extent.cpu()[slots], want), (cid, it)


# ---- differentiable forward -----------------------------------------------------------------------------------------

def test_differentiable_forward_bits_and_gradients(device):
    """With enable_autograd() the values of a 4-step unroll are bit-identical to the fused forward's, and the
    gradients of a VDN-style loss (sum over agents of the chosen Q against a target), per agent and tensor, are within
    1e-4 of the float64 reference tensor's largest element."""
    H, N, B, T = 64, 3, 6, 4
    mac, args, ps = _mac(device, N, H, seed=5)
    mac.cuda()
    tb = _raw_batch(B, T, N, seed=21)
    batch, _, _ = _episode_batch(device, args, tb, B, T)
    g = torch.Generator().manual_seed(4)
    chosen = torch.randint(0, A, (B, T, N, 1), generator=g)
    target = torch.randn(B, T, generator=g)

    def loss_of(q):  # q [B, T, N, A]
        qt = torch.gather(q, 3, chosen.to(q.device)).squeeze(3).sum(dim=2)
        return ((qt - target.to(q.device, q.dtype)) ** 2).mean()

    pp = [{k: v.double().requires_grad_(True) for k, v in p.items()} for p in ps]
    q64, _ = DR.mac_unroll(pp, {k: v.double() for k, v in tb.items()})
    loss_of(q64).backward()
    mac.init_hidden(B)
    q_fused = torch.stack([mac.forward(batch, t) for t in range(T)], dim=1)  # autograd not enabled: the fused call
    assert not q_fused.requires_grad and tuple(mac.hidden_states.shape) == (B, N, H)
    h_fused = mac.hidden_states
    mac.enable_autograd()
    with torch.no_grad():
        mac.init_hidden(B)
        q_ng = torch.stack([mac.forward(batch, t) for t in range(T)], dim=1)
    assert not q_ng.requires_grad and torch.equal(q_ng, q_fused)
    mac.init_hidden(B)
    q_grad = torch.stack([mac.forward(batch, t) for t in range(T)], dim=1)
    assert q_grad.requires_grad and tuple(q_grad.shape) == (B, T, N, A)
    assert torch.equal(q_grad.detach(), q_fused) and torch.equal(mac.hidden_states.detach(), h_fused)
    _bound_check("differentiable MAC path, Q", q_grad, q64.detach())
    loss = loss_of(q_grad)
    loss.backward()
    assert abs(float(loss.detach()) - float(loss_of(q64.detach()))) <= 1e-4
    print("T = 4 unroll, VDN-style loss")
    for i, agent in enumerate(mac.agents):
        for k, v in agent.named_parameters():
            ref = pp[i][k].grad
            err = float((v.grad.detach().cpu().to(F64) - ref).abs().max())
            bound = 1e-4 * float(ref.abs().max())
            print(f"  agent {i} {k:16s} err {err:.3e}  bound {bound:.3e}  ({100 * err / bound:.1f} %)")
            assert err <= bound, (i, k, err, bound)
