"""GPU parity of the feed-forward agent (agent: dqn): mlg_ff_forward / mlg_ff_mac_forward and the autograd pair
maleague::dqn_forward / dqn_backward against the float64 oracle (tests/dqn_ref.py, pinned to the reference's goldens
by tests/test_dqn.py), and mlg_rollout_ff per dispatch arm by the method of tests/test_gpu_rollout_shapes.py.

Bounds (the project's own, tests/test_gpu_learner_arms.py and tests/test_gpu_autograd.py): Q within 1e-4 of the
float64 oracle; every gradient tensor max|g - g_ref| <= 1e-4 * max(1, max|g_ref|). Each check prints its error next
to its bound (`pytest -s`). Rollout: env tensors bit-exact against the C env under teacher forcing, random picks those
of the counter RNG, every greedy pick the float64 oracle's argmax except at a near tie (top-two masked Q within 1e-4),
near ties accepted for at most 1 % of a case's greedy picks (tests/dqn_shapes.py holds the cases and the oracle's own
share).
"""
import os

import numpy as np
import pytest
import torch

import dqn_ref
import dqn_shapes as DS
import helpers
from helpers import Q_TOL, build_stepper, qmix_args, scheme_for, shape_plan

pytestmark = pytest.mark.gpu

F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEAR_TIE_CAP = 0.01
D_OBS = 48  # the 3v3 plan's obs width: d_in = 48 + 11 + 3 = 62, no multiple of 16


def _agent(device, H, A, N=3, d_obs=D_OBS, last_action=True, agent_id=True, seed=3, enable=False):
    from maleague.modules.agents import DQNAgentNetwork
    d_in = d_obs + (A if last_action else 0) + (N if agent_id else 0)
    args = qmix_args(n_agents=N, n_actions=A, rnn_hidden_dim=H, obs_last_action=last_action, obs_agent_id=agent_id,
                     agent="dqn", device=str(device))
    ag = DQNAgentNetwork(d_in, args)
    p = dqn_ref.agent_params(d_in, H, A, seed)
    ag.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return (ag.enable_autograd() if enable else ag), {k: torch.from_numpy(v) for k, v in p.items()}, d_in


def _q_check(name, got, ref64):
    err = float((got.detach().cpu().to(F64) - ref64).abs().max()) if ref64.numel() else 0.0
    print(f"  {name:40s} max |q - q64| {err:.3e}  bound {Q_TOL:.1e}")
    assert err <= Q_TOL, (name, err)


def _g_check(name, got, ref64):
    err = float((got.detach().cpu().to(F64) - ref64).abs().max()) if ref64.numel() else 0.0
    scale = max(1.0, float(ref64.abs().max())) if ref64.numel() else 1.0
    print(f"  {name:40s} err {err:.3e}  bound {1e-4 * scale:.3e}")
    assert err <= 1e-4 * scale, (name, err)


# ---- 5. forward and MAC forward -----------------------------------------------------------------------------------

@pytest.mark.parametrize("A", [11, 23, 65])
@pytest.mark.parametrize("H", [32, 64, 128])
def test_ff_forward_matches_float64_oracle(device, H, A):
    """R = 1, 15, 16, 17, 33 rows (ragged against the 16-row tile, more than one tile, more than one 4-tile
    workgroup at 33 + the 65 of the golden check below); one, two and five action tiles."""
    ag, p, d_in = _agent(device, H, A)
    p64 = {k: v.double() for k, v in p.items()}
    g = torch.Generator().manual_seed(H + A)
    for R in (1, 15, 16, 17, 33):
        x = torch.randn(R, d_in, generator=g)
        q, h = ag(x.to(device), torch.zeros(R, 1, device=device))
        assert tuple(q.shape) == (R, A) and tuple(h.shape) == (R, 1)
        _q_check(f"ff_forward H={H} A={A} R={R}", q, dqn_ref.dqn_forward(p64, x.double()))


def test_ff_forward_matches_reference_golden(device, golden):
    from maleague.modules.agents import DQNAgentNetwork
    g = golden("dqn_forward.npz")
    ag = DQNAgentNetwork(100, qmix_args(agent="dqn", device=str(device)))
    ag.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("p.")})
    q, _ = ag(torch.from_numpy(g["inputs"]).to(device), torch.zeros(40, 1, device=device))
    np.testing.assert_allclose(q.cpu().numpy(), g["q"], rtol=0, atol=Q_TOL)


def _raw_batch(slots, T1, N, A, d_obs, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(slots, T1, N, d_obs, generator=g)
    acts = torch.randint(0, A, (slots, T1, N), generator=g)
    oh = torch.zeros(slots, T1, N, A).scatter_(3, acts.unsqueeze(-1), 1.0)
    return {"obs": obs, "actions_onehot": oh}


def _mac_forward(device, ag, tb, B, T1, t, rows=None):
    from maleague import _native
    dev = {k: v.to(device).contiguous() for k, v in tb.items()}
    rows_d = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=device)
    mb = _native.MlgBatch(None, dev["obs"].data_ptr(), None, None, None, None, dev["actions_onehot"].data_ptr(), None,
                          B, T1, 0, 0, 0, None if rows_d is None else rows_d.data_ptr())
    d = ag.dims()
    q = torch.full((B, d.n_agents, d.n_actions), float("nan"), device=device)
    _native.call("mlg_ff_mac_forward", _native.byref(d), _native.ptr(ag.packed()), _native.byref(mb), int(t),
                 _native.ptr(q), _native.stream_ptr())
    torch.cuda.synchronize()
    return q


@pytest.mark.parametrize("H,A,N,B,la,ai", [(64, 11, 3, 11, True, True), (32, 11, 3, 5, False, True),
                                           (128, 11, 3, 6, True, False), (64, 23, 9, 7, True, True),
                                           (32, 65, 7, 5, True, True)],
                         ids=["h64-3v3", "no-last-action", "no-agent-id", "a23-n9", "a65-n7"])
def test_ff_mac_forward_matches_float64_oracle(device, H, A, N, B, la, ai):
    """B N = 33 / 15 / 18 / 63 / 35 rows; t = 0 (no last action) and t > 0; inputs built in the kernel from the
    batch."""
    T1 = 4
    ag, p, d_in = _agent(device, H, A, N=N, last_action=la, agent_id=ai)
    tb = _raw_batch(B, T1, N, A, D_OBS, seed=H + N)
    p64 = {k: v.double() for k, v in p.items()}
    tb64 = {k: v.double() for k, v in tb.items()}
    for t in (0, 2, 3):
        q = _mac_forward(device, ag, tb, B, T1, t)
        ref = dqn_ref.mac_unroll(p64, tb64, N, last_action=la, agent_id=ai, ts=[t])[:, 0]
        _q_check(f"ff_mac_forward H={H} A={A} N={N} t={t}", q, ref)


def test_ff_mac_forward_sampled_rows_equal_gathered_copy(device):
    """A sampled view (episode b in slot rows[b] of a larger buffer) gives the bits of its gathered copy."""
    H, A, N, T1, slots = 64, 11, 3, 4, 13
    ag, p, d_in = _agent(device, H, A, N=N)
    tb = _raw_batch(slots, T1, N, A, D_OBS, seed=9)
    rows = [12, 0, 7, 7, 3, 11]
    gathered = {k: v[rows] for k, v in tb.items()}
    for t in (0, 3):
        q_view = _mac_forward(device, ag, tb, len(rows), T1, t, rows=rows)
        q_copy = _mac_forward(device, ag, gathered, len(rows), T1, t)
        assert torch.equal(q_view, q_copy), t
        assert not torch.isnan(q_view).any()


# ---- 6. autograd --------------------------------------------------------------------------------------------------

def _reference_grads(p, x, gq, dtype=F64):
    pp = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p.items()}
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    q = dqn_ref.dqn_forward(pp, xx)
    (q * gq.to(dtype)).sum().backward()
    out = {k: v.grad for k, v in pp.items()}
    out["d_inputs"] = xx.grad
    return out


@pytest.mark.parametrize("H,A", [(32, 11), (64, 23), (128, 65)])
@pytest.mark.parametrize("R", [1, 17, 33])
def test_dqn_forward_gradients(device, R, H, A):
    """Every parameter and the inputs against float64 autograd of the oracle; the op's values equal the plain path's
    bit for bit; two calls give identical bits."""
    ag, p, d_in = _agent(device, H, A, enable=True)
    g = torch.Generator().manual_seed(100 + R)
    x, gq = torch.randn(R, d_in, generator=g), torch.randn(R, A, generator=g)
    ref = _reference_grads(p, x, gq)
    runs = []
    for _ in range(2):
        for prm in ag.parameters():
            prm.grad = None
        xd = x.to(device).requires_grad_(True)
        q, _ = ag(xd, torch.zeros(R, 1, device=device))
        assert q.requires_grad
        q.backward(gq.to(device))
        runs.append([prm.grad.clone() for prm in ag.parameters()] + [xd.grad.clone(), q.detach().clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    with torch.no_grad():
        q_plain, _ = ag(x.to(device), torch.zeros(R, 1, device=device))
    assert torch.equal(q_plain, runs[0][-1])
    print(f"dqn_forward gradients R={R} H={H} A={A}")
    for (k, _), got in zip(ag.named_parameters(), runs[0]):
        _g_check(k, got, ref[k])
    _g_check("d_inputs", runs[0][-2], ref["d_inputs"])


def _ff_backward_into(device, ag, x, gq, fill):
    """mlg_ff_backward called directly, into dparams / d_inputs / workspace buffers pre-filled with ``fill``."""
    from maleague import _native
    d = ag.dims()
    R = x.shape[0]
    params = [t.detach().contiguous() for t in ag._live_params()]
    cparams = _native.MlgFFParams(*[_native.ptr(t) for t in params])
    dparams = torch.full((sum(t.numel() for t in params),), fill, device=device)
    d_inputs = torch.full((max(R, 1), d.d_in), fill, device=device)
    n_ws = _native.load().mlg_ff_backward_workspace_floats(_native.byref(d), R)
    assert n_ws >= 0
    ws = torch.full((max(int(n_ws), 4),), fill, device=device)
    _native.call("mlg_ff_backward", _native.byref(d), _native.byref(cparams), _native.ptr(ag.packed()),
                 _native.ptr(x) if R else None, None if gq is None else _native.ptr(gq), _native.ptr(d_inputs),
                 _native.ptr(dparams), _native.ptr(ws), R, _native.stream_ptr())
    torch.cuda.synchronize()
    return dparams, d_inputs[:R]


def test_ff_backward_overwrites_nan_filled_outputs(device):
    """mlg_ff_backward into NaN-filled dparams, d_inputs and workspace: gq = NULL and R = 0 leave dparams all zero
    (overwritten, not accumulated; a call reads no workspace word it did not write), and a call with an upstream
    gradient gives the bits it gives into zero-filled buffers."""
    ag, p, d_in = _agent(device, 64, 11)
    nan = float("nan")
    g = torch.Generator().manual_seed(8)
    x = torch.randn(21, d_in, generator=g).to(device)
    gq = torch.randn(21, 11, generator=g).to(device)
    dparams, d_inputs = _ff_backward_into(device, ag, x, None, nan)
    assert torch.equal(dparams, torch.zeros_like(dparams)) and torch.equal(d_inputs, torch.zeros_like(d_inputs))
    dparams, _ = _ff_backward_into(device, ag, x[:0], None, nan)
    assert torch.equal(dparams, torch.zeros_like(dparams))
    dparams, _ = _ff_backward_into(device, ag, x[:0], gq[:0], nan)
    assert torch.equal(dparams, torch.zeros_like(dparams))
    got_nan, din_nan = _ff_backward_into(device, ag, x, gq, nan)
    got_zero, din_zero = _ff_backward_into(device, ag, x, gq, 0.0)
    assert not torch.isnan(got_nan).any() and bool(got_nan.any()) and not torch.isnan(din_nan).any()
    assert torch.equal(got_nan, got_zero) and torch.equal(din_nan, din_zero)
    ref = _reference_grads(p, x.cpu(), gq.cpu())
    off = 0
    for k in dqn_ref.AGENT_KEYS:
        n = ref[k].numel()
        _g_check(k, got_nan[off:off + n].view(ref[k].shape), ref[k])
        off += n
    _g_check("d_inputs", din_nan, ref["d_inputs"])


def _episode_batch(device, args, tb, B, T1):
    from maleague.components.episode_batch import EpisodeBatch
    info = {"state_shape": args.state_shape, "obs_shape": tb["obs"].shape[-1], "n_actions": args.n_actions,
            "n_agents": args.n_agents}
    scheme, groups, preprocess = scheme_for(info, torch)
    batch = EpisodeBatch(scheme, groups, B, T1, preprocess=preprocess, device=device)
    batch.data.transition_data["obs"].copy_(tb["obs"])
    batch.data.transition_data["actions_onehot"].copy_(tb["actions_onehot"])
    return batch, scheme, groups


def test_mac_unroll_vdn_loss_gradients(device):
    """A T = 3 unroll through BasicMAC.enable_autograd() with a VDN-style loss (sum over agents of the chosen Q against
    a target) against float64 autograd of the oracle; under no_grad the MAC takes the fused path (mlg_ff_mac_forward)
    and leaves hidden_states alone."""
    from maleague.controllers import BasicMAC
    H, A, N, B, T = 64, 11, 3, 6, 3
    d_in = D_OBS + A + N
    args = qmix_args(n_agents=N, n_actions=A, rnn_hidden_dim=H, agent="dqn", device=str(device), state_shape=36)
    tb = _raw_batch(B, T, N, A, D_OBS, seed=21)
    batch, scheme, groups = _episode_batch(device, args, tb, B, T)
    mac = BasicMAC(batch.scheme, groups, args)
    p = {k: torch.from_numpy(v) for k, v in dqn_ref.agent_params(d_in, H, A, 5).items()}
    mac.agent.load_state_dict(p)
    mac.agent.to(device)
    g = torch.Generator().manual_seed(4)
    chosen = torch.randint(0, A, (B, T, N, 1), generator=g)
    target = torch.randn(B, T, generator=g)

    def loss_of(q):  # q [B, T, N, A]
        qt = torch.gather(q, 3, chosen.to(q.device)).squeeze(3).sum(dim=2)
        return ((qt - target.to(q.device, q.dtype)) ** 2).mean()

    pp = {k: v.double().requires_grad_(True) for k, v in p.items()}
    loss_of(dqn_ref.mac_unroll(pp, {k: v.double() for k, v in tb.items()}, N)).backward()
    mac.init_hidden(B)
    h_before = mac.hidden_states
    with torch.no_grad():
        q_fused = torch.stack([mac.forward(batch, t) for t in range(T)], dim=1)
    assert mac.hidden_states is h_before and tuple(h_before.shape) == (B, N, 1)
    mac.enable_autograd()
    q_grad = torch.stack([mac.forward(batch, t) for t in range(T)], dim=1)
    assert q_grad.requires_grad
    # the module path runs the dense fc1 over [obs | one-hot | id], the fused path gathers the one-hot and id columns:
    # the same sum in another order, so both are held to the oracle, not to each other's bits
    with torch.no_grad():
        q64 = dqn_ref.mac_unroll({k: v.detach() for k, v in pp.items()}, {k: v.double() for k, v in tb.items()}, N)
    _q_check("fused MAC path", q_fused, q64)
    _q_check("differentiable MAC path", q_grad, q64)
    loss = loss_of(q_grad)
    loss.backward()
    print("T = 3 unroll, VDN-style loss")
    with torch.no_grad():
        assert abs(float(loss.detach()) - float(loss_of(q64))) <= 1e-4
    for k, v in mac.agent.named_parameters():
        _g_check(k, v.grad, pp[k].grad)


# ---- 7. rollout per dispatch arm ------------------------------------------------------------------------------------

@pytest.fixture
def dqn_oracle(monkeypatch):
    """helpers.check_run with the feed-forward oracle in place of the DRQN's (its env replay and pick rules as is)."""
    monkeypatch.setattr(helpers, "oracle_q", dqn_ref.oracle_q)


def _stepper(device, cid, B=DS.B):
    _, hidden, plan, arm, seed, scale = DS.case(cid)
    stepper, mac, args = build_stepper(device, plan=shape_plan(plan), B=B, episode_limit=DS.EPISODE_LIMIT, seed=seed,
                                       rnn_hidden_dim=hidden, agent="dqn")
    a = mac.agent
    p = dqn_ref.agent_params(a.input_shape, hidden, a.args.n_actions, seed, scale)
    a.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return stepper, mac, args, arm


def _cap(cid, mode, n):
    print(f"{cid} [{mode}]: {n}")
    assert n["near_ties"] <= NEAR_TIE_CAP * n["greedy"], (cid, mode, n)


@pytest.mark.parametrize("cid", [c[0] for c in DS.CASES])
def test_rollout_ff_parity(device, cid, dqn_oracle):
    stepper, mac, args, arm = _stepper(device, cid)
    name, lds = stepper.describe_rollout()
    print(f"{cid}: arm {name}, {lds} B of LDS, B = {DS.B}")
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


def test_rollout_ff_single_env(device, dqn_oracle):
    """B = 1: one env in a 16-env workgroup."""
    stepper, mac, args, arm = _stepper(device, "ff-lds-h64-3v3", B=1)
    batch, infos = stepper.run(test_mode=True)
    helpers.check_run(stepper, mac, args, batch, infos, episode=0, test_mode=True, eps=0.0, dtype=F64)


@pytest.mark.parametrize("cid", DS.RING_CASES)
def test_rollout_ff_ring_mode_equals_plain_run(device, cid):
    """A train-mode run written straight into replay slots pre-filled with other bytes (full-write mode, wrapping
    around the ring's end) equals the plain run into a zero-initialised batch byte for byte; slot extents follow."""
    from maleague.components.replay_buffer import ReplayBuffer
    from maleague.envs.teams_env import VecEnvState
    stepper, mac, args, arm = _stepper(device, cid)
    assert stepper.describe_rollout()[0] == arm
    scheme, groups, preprocess = scheme_for(stepper.get_env_info(), torch)
    size = DS.B + 5
    ring = ReplayBuffer(scheme, groups, size, DS.EPISODE_LIMIT + 1, preprocess=preprocess, device=device)
    for v in ring.data.transition_data.values():
        v.fill_(7)
    for it in range(2):  # slots 0..36, then 37..41 and 0..31 (wraps)
        runs = []
        for use_ring in (False, True):
            st = VecEnvState(stepper.spec, DS.B, device)
            st.episode.fill_(it)
            stepper.envs = st
            stepper.t_env = DS.T_ENV
            stepper._ring = None
            if use_ring:
                assert stepper.attach_replay(ring)
            runs.append(stepper.run(test_mode=False)[0])
        b_plain, b_ring = runs
        for k in b_plain.data.transition_data:
            assert torch.equal(b_plain[k], b_ring[k]), (cid, it, k)
        ring.insert_episode_batch(b_ring)
        slots = (torch.arange(DS.B) + b_ring.slot0) % size
        want = (stepper.last_run["ep_len"] + 1).to(torch.int32)
        assert torch.equal(ring.slot_extent.cpu()[slots], want), (cid, it)


# ---- 9. end to end: rollout, then training steps through the differentiable path, then checkpoints -----------------

def test_rollout_then_training_steps_through_autograd(device):
    """3v3, 8 envs: the MAC trains on its own rollout's batch through the differentiable path (a VDN TD loss written
    the reference's way, torch RMSprop, a handful of steps; the fused QLearner's own end-to-end run is in
    tests/test_gpu_dqn_learner.py). Losses are finite, every parameter
    moved, and the stepped MAC's Q (the packed block must follow the optimizer) stay within 1e-4 of the oracle's
    forward with the stepped parameters, on the fused path and in the next rollout's picks."""
    stepper, mac, args = build_stepper(device, plan="small", B=8, episode_limit=20, seed=3, rnn_hidden_dim=64,
                                       agent="dqn")
    N, A = args.n_agents, args.n_actions
    stepper.t_env = DS.T_ENV
    batch, _ = stepper.run(test_mode=False)
    stepper.flush()
    T = int(batch.max_t_filled())
    sample = batch[:, :T]
    before = {k: v.detach().clone() for k, v in mac.agent.state_dict().items()}
    mac.enable_autograd()
    opt = torch.optim.RMSprop(list(mac.parameters()), lr=args.lr, alpha=args.optim_alpha, eps=args.optim_eps)
    rew, term = sample["reward"][:, :-1], sample["terminated"][:, :-1].float()
    mask = sample["filled"][:, :-1].float()
    mask[:, 1:] = mask[:, 1:] * (1 - term[:, :-1])
    losses = []
    for _ in range(5):
        mac.init_hidden(sample.batch_size)
        out = torch.stack([mac.forward(sample, t) for t in range(T)], dim=1)
        chosen = torch.gather(out[:, :-1], 3, sample["actions"][:, :-1]).squeeze(3).sum(dim=2, keepdim=True)
        with torch.no_grad():
            nxt = out[:, 1:].detach().masked_fill(sample["avail_actions"][:, 1:] == 0, -9999999).max(dim=3)[0]
            target = rew + args.gamma * (1 - term) * nxt.sum(dim=2, keepdim=True)
        loss = (((chosen - target) * mask) ** 2).sum() / mask.sum()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(mac.parameters()), args.grad_norm_clip)
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", losses)
    assert all(np.isfinite(losses))
    after = {k: v.detach().cpu() for k, v in mac.agent.state_dict().items()}
    for k, v in after.items():
        assert torch.isfinite(v).all() and not torch.equal(v, before[k].cpu()), k
    p64 = {k: v.double() for k, v in after.items()}
    tb = {k: sample[k].detach().cpu().double() for k in ("obs", "actions_onehot")}
    with torch.no_grad():
        mac.init_hidden(sample.batch_size)
        q = torch.stack([mac.forward(sample, t) for t in range(T)], dim=1)
        _q_check("stepped MAC, fused path", q, dqn_ref.mac_unroll(p64, tb, N, T=T))
    assert tuple(q.shape) == (8, T, N, A)


def test_trained_weights_drive_the_next_rollout(device, dqn_oracle):
    """Parameters changed by a torch optimizer step reach the rollout kernel: the run after the step is checked
    against the oracle with the stepped parameters."""
    stepper, mac, args, arm = _stepper(device, "ff-lds-h64-3v3", B=8)
    mac.enable_autograd()
    opt = torch.optim.SGD(list(mac.parameters()), lr=0.05)
    batch, infos = stepper.run(test_mode=True)
    helpers.check_run(stepper, mac, args, batch, infos, episode=0, test_mode=True, eps=0.0, dtype=F64)
    mac.init_hidden(8)
    mac.forward(batch, 0).square().sum().backward()
    opt.step()
    batch, infos = stepper.run(test_mode=True)
    helpers.check_run(stepper, mac, args, batch, infos, episode=1, test_mode=True, eps=0.0, dtype=F64)



# ---- checkpoints --------------------------------------------------------------------------------------------------

def test_checkpoint_round_trip_and_reference_file(device, tmp_path, golden):
    """save_models / load_models round trip, and the reference's recorded agent.th drives the kernels: Q along the
    golden batch within 1e-4 of the reference's own BasicMAC.forward."""
    from maleague.controllers import BasicMAC
    g = golden("dqn_mac_forward.npz")
    tb = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("b.")}
    B, T, N, A = 3, 4, 5, 15
    args = qmix_args(agent="dqn", device=str(device))
    batch, scheme, groups = _episode_batch(device, args, tb, B, T)
    mac = BasicMAC(batch.scheme, groups, args)
    mac.agent.to(device)
    mac.load_models(os.path.join(GOLDEN, "ckpt_dqn", "100"), "home_")
    mac.init_hidden(B)
    q = torch.stack([mac.forward(batch, t) for t in range(T)])
    np.testing.assert_allclose(q.cpu().numpy(), g["q"], rtol=0, atol=Q_TOL)
    mac.save_models(str(tmp_path), "x_")
    other = BasicMAC(batch.scheme, groups, args)
    other.agent.to(device)
    other.load_models(str(tmp_path), "x_")
    other.init_hidden(B)
    assert torch.equal(torch.stack([other.forward(batch, t) for t in range(T)]), q)
    sd = torch.load(os.path.join(str(tmp_path), "x_agent.th"), weights_only=True)
    assert list(sd) == ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
