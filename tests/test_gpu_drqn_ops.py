"""GPU parity of the stand-alone DRQN and QMixer entry points off the fixture shape: mlg_agent_forward,
mlg_mac_forward, mlg_qmix_forward, mlg_qmix_backward, mlg_agent_backward and mlg_select_actions (csrc/agent.hip,
csrc/agent_grad.hip) against the float64 oracle (oracle/learner_ref.py, pinned to the reference's goldens by
tests/test_oracle_golden.py). The cases, their seeds and the conditions on them are in tests/drqn_op_shapes.py;
tests/test_drqn_op_shapes.py asserts the conditions on the CPU.

Bounds (the project's own): every value tensor (q, h', q_tot) and every gradient tensor
max|y - y64| <= 1e-4 max(1, max|y64|) (tests/test_gpu_autograd.py _check, helpers.Q_TOL for the DRQN's O(1) values);
picks equal the oracle's exactly. Each check prints its error next to its bound and next to the fp32 CPU oracle's own
distance from float64 (`pytest -s`), and each test prints the largest error / bound ratio of its group so far.

What each test runs that no earlier test ran:
  test_agent_forward            agent_forward_kernel<32 / 64 / 128, true> values at A below / at / past one action tile
                                and at five tiles, d_in no multiple of 16, R at the 16-row tile and 4-tile workgroup
                                edges, and the h_in == NULL branch
  test_mac_forward              agent_forward_kernel<H, false> with obs_last_action / obs_agent_id off (w1a / w1n absent
                                from make_agent_layout, RowIn built without them), ragged last tiles, t = 0 .. 3 chained
  test_mac_forward_sampled_rows MlgBatch.rows
  test_basic_mac_flag_off       BasicMAC._fused_forward with a flag off: the Python-side dims
  test_mixer                    qmix_forward_kernel values (also hypernet_layers == 1); qmix_backward_kernel and the
                                weight-gradient jobs with BJob::va / vb off (scalar delta and x loads: n1, e5), every
                                workspace section padded by take() (e5), 9 x 4 and 16 output blocks, chunk edges
  test_mixer_golden             the reference's own qmix_fwd.npz through the kernel
  test_agent_gradients          mlg_agent_backward at the chunk edges 64 / 65 / 257, H = 32 / 128 at 65 rows, A = 5 / 16
                                / 65, flags off
  test_*_backward_poisoned      the exact workspace size the query reports, NaN-filled outputs and workspace, R = 0
  test_select_greedy / _epsilon select_actions_kernel over two blocks, exact ties, a fully masked row, an unavailable
                                maximum, is_greedy == NULL, episodes == NULL, epsilon = 1, keys with bit 63 set

Largest measured error / bound ratios per group (MI355X, all 72 tests pass; the fp32 CPU oracle's own share of the
bound is at most 0.0082 over every case, tests/test_drqn_op_shapes.py):
  agent forward   0.0045  (q and h' of test_agent_forward and of the gradient cases)
  MAC forward     0.0029
  mixer forward   0.0029
  mixer gradients 0.0124
  agent gradients 0.0148
No case came near its bound and no kernel bug was found at these shapes.
"""
import numpy as np
import pytest
import torch

import drqn_op_shapes as DS
import learner_ref as LR
from helpers import qmix_args, scheme_for
from test_gpu_autograd import _check, agent_reference, mixer_reference

pytestmark = pytest.mark.gpu

f64, f32 = torch.float64, torch.float32
NAN = float("nan")
RATIOS = {}


def _chk(group, name, got, ref64, ref32):
    """_check, with the largest error / bound ratio of the group kept for the module docstring."""
    assert tuple(got.shape) == tuple(ref64.shape), (name, tuple(got.shape), tuple(ref64.shape))
    assert not torch.isnan(got).any(), name
    ratio = _check(name, got, ref64, ref32) / 1e-4
    RATIOS[group] = max(RATIOS.get(group, 0.0), ratio)
    return ratio


def _report(group):
    print(f"  [{group}] largest error / bound so far: {RATIOS.get(group, 0.0):.4f}")


def _agent(device, d_in, H, A, N, p, last_action=True, agent_id=True, enable=False):
    from maleague.modules.agents.drqn_agent import DRQNAgentNetwork
    ag = DRQNAgentNetwork(d_in, qmix_args(n_agents=N, n_actions=A, rnn_hidden_dim=H, obs_last_action=last_action,
                                          obs_agent_id=agent_id, device=str(device)))
    ag.load_state_dict(p)
    d = ag.dims()
    assert (d.d_in, d.obs_last_action, d.obs_agent_id) == (d_in, int(last_action), int(agent_id))
    return ag.enable_autograd() if enable else ag


# ---- A. mlg_agent_forward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", DS.FWD_A)
@pytest.mark.parametrize("H", DS.FWD_H)
def test_agent_forward(device, H, A):
    from maleague import _native
    p = DS.fwd_params(H, A)
    ag = _agent(device, DS.fwd_d_in(A), H, A, DS.FWD_N, p)
    print(f"agent forward H={H} A={A}")
    for R, x, h in DS.fwd_inputs(H, A):
        q64, h64 = DS.fwd_reference(p, x, h, f64)
        q32, h32 = DS.fwd_reference(p, x, h, f32)
        xd = x.to(device)
        if h is None:  # the kernel's zero-hidden branch, against the module's init_hidden() rows
            q = torch.full((R, A), NAN, device=device)
            hn = torch.full((R, H), NAN, device=device)
            _native.call("mlg_agent_forward", _native.byref(ag.dims()), _native.ptr(ag.packed()), _native.ptr(xd), None,
                         _native.ptr(q), _native.ptr(hn), R, _native.stream_ptr())
            torch.cuda.synchronize()
            q2, hn2 = ag(xd, ag.init_hidden().expand(R, -1))
        else:
            q, hn = ag(xd, h.to(device))
            q2, hn2 = ag(xd, h.to(device))
        assert not q.requires_grad and not hn.requires_grad
        assert torch.equal(q, q2) and torch.equal(hn, hn2), R
        tag = f"R={R}" + (" h_in=NULL" if h is None else "")
        _chk("agent forward", f"q {tag}", q, q64, q32)
        _chk("agent forward", f"h' {tag}", hn, h64, h32)
    _report("agent forward")


# ---- B. mlg_mac_forward ---------------------------------------------------------------------------------------------
def _mac_forward(device, ag, dev, B, T1, t, h_in, rows=None):
    """mlg_mac_forward called directly into NaN-filled q / h_out. dev: the batch's device tensors."""
    from maleague import _native
    rows_d = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=device)
    mb = _native.MlgBatch(None, dev["obs"].data_ptr(), None, None, None, None, dev["actions_onehot"].data_ptr(), None,
                          B, T1, 0, 0, 0, None if rows_d is None else rows_d.data_ptr())
    d = ag.dims()
    q = torch.full((B, d.n_agents, d.n_actions), NAN, device=device)
    h_out = torch.full((B * d.n_agents, d.hidden), NAN, device=device)
    _native.call("mlg_mac_forward", _native.byref(d), _native.ptr(ag.packed()), _native.byref(mb), int(t),
                 _native.ptr(h_in), _native.ptr(q), _native.ptr(h_out), _native.stream_ptr())
    torch.cuda.synchronize()
    assert not torch.isnan(q).any() and not torch.isnan(h_out).any()
    return q, h_out


def _mac_chain(device, c, ag, tb, h0):
    dev = {k: v.to(device).contiguous() for k, v in tb.items()}
    h = h0.to(device)
    qs = []
    for t in range(DS.MAC_T1):
        q, h = _mac_forward(device, ag, dev, c.B, DS.MAC_T1, t, h)
        qs.append(q)
    return torch.stack(qs, dim=1), h


@pytest.mark.parametrize("cid", DS.MAC_IDS)
def test_mac_forward(device, cid):
    c = DS.mac_case(cid)
    p = DS.mac_params(c)
    ag = _agent(device, DS.mac_d_in(c), c.H, c.A, c.N, p, c.last_action, c.agent_id)
    tb, h0 = DS.mac_inputs(c)
    q64, h64 = DS.mac_reference(c, p, tb, h0, f64)
    q32, h32 = DS.mac_reference(c, p, tb, h0, f32)
    q, h = _mac_chain(device, c, ag, tb, h0)
    print(f"mac forward {cid}: {c.B * c.N} rows")
    for t in range(DS.MAC_T1):
        _chk("MAC forward", f"q t={t}", q[:, t], q64[:, t], q32[:, t])
    _chk("MAC forward", "h after t=3", h, h64, h32)
    _report("MAC forward")


def test_mac_forward_sampled_rows(device):
    """A sampled view (episode b in slot rows[b] of a 13-slot buffer) gives the bits of its gathered copy."""
    c = DS.mac_case("h64-both")
    ag = _agent(device, DS.mac_d_in(c), c.H, c.A, c.N, DS.mac_params(c))
    tb, _ = DS.mac_inputs(c, slots=DS.SAMPLED_SLOTS)
    rows = DS.SAMPLED_ROWS
    g = torch.Generator().manual_seed(5)
    h_in = torch.randn(len(rows), c.N, c.H, generator=g) * 0.7
    h_in[3] = h_in[2]  # episodes 2 and 3 are both slot 7: with one hidden state they must give the same bits
    h_in = h_in.view(len(rows) * c.N, c.H).to(device)
    whole = {k: v.to(device).contiguous() for k, v in tb.items()}
    gathered = {k: v[rows].to(device).contiguous() for k, v in tb.items()}
    for t in (0, 3):
        q_view, h_view = _mac_forward(device, ag, whole, len(rows), DS.MAC_T1, t, h_in, rows=rows)
        q_copy, h_copy = _mac_forward(device, ag, gathered, len(rows), DS.MAC_T1, t, h_in)
        assert torch.equal(q_view, q_copy) and torch.equal(h_view, h_copy), t
        assert torch.equal(q_view[2], q_view[3]) and not torch.equal(q_view[0], q_view[1])  # slot 7 twice


def test_basic_mac_flag_off(device):
    """BasicMAC.forward with obs_last_action off gives the bits of the direct call: the Python-side dims are right."""
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    c = DS.mac_case(DS.MODULE_PATH_CASE)
    p = DS.mac_params(c)
    tb, h0 = DS.mac_inputs(c)
    args = qmix_args(n_agents=c.N, n_actions=c.A, rnn_hidden_dim=c.H, obs_last_action=c.last_action,
                     obs_agent_id=c.agent_id, state_shape=36, device=str(device))
    info = {"state_shape": 36, "obs_shape": DS.MAC_D_OBS, "n_actions": c.A, "n_agents": c.N}
    scheme, groups, preprocess = scheme_for(info, torch)
    batch = EpisodeBatch(scheme, groups, c.B, DS.MAC_T1, preprocess=preprocess, device=device)
    batch.data.transition_data["obs"].copy_(tb["obs"])
    batch.data.transition_data["actions_onehot"].copy_(tb["actions_onehot"])
    mac = BasicMAC(batch.scheme, groups, args)
    mac.load_state_dict(p)
    d = mac.agent.dims()
    assert (d.d_obs, d.d_in, d.obs_last_action, d.obs_agent_id) == (DS.MAC_D_OBS, DS.MAC_D_OBS + c.N, 0, 1)
    mac.hidden_states = h0.to(device).view(c.B, c.N, c.H)
    q_mac = torch.stack([mac.forward(batch, t) for t in range(DS.MAC_T1)], dim=1)
    ag = _agent(device, DS.mac_d_in(c), c.H, c.A, c.N, p, c.last_action, c.agent_id)
    q, h = _mac_chain(device, c, ag, tb, h0)
    assert torch.equal(q_mac, q) and torch.equal(mac.hidden_states.reshape(-1, c.H), h)


# ---- C. mlg_qmix_forward / mlg_qmix_backward ------------------------------------------------------------------------
def _mixer(c, mp, device, enable=False):
    from maleague.modules.mixers import QMixer
    mx = QMixer(qmix_args(n_agents=c.N, hypernet_layers=c.layers, state_shape=c.S, mixing_embed_dim=c.E,
                          hypernet_embed=c.HE if c.layers == 2 else 64, device=str(device)))
    mx.load_state_dict(mp)
    assert sum(v.numel() for v in mx.parameters()) == DS.mixer_param_count(c)
    return mx.enable_autograd() if enable else mx


@pytest.mark.parametrize("R", DS.MIXER_R)
@pytest.mark.parametrize("cid", DS.MIXER_IDS)
def test_mixer(device, cid, R):
    c = DS.mixer_case_of(cid)
    mp, qs, st, g_out = DS.mixer_inputs(c, R)
    ref = mixer_reference(mp, qs, st, g_out, c.layers, c.N, f64, check=True, S_DIM=c.S, E_DIM=c.E)
    r32 = mixer_reference(mp, qs, st, g_out, c.layers, c.N, f32, S_DIM=c.S, E_DIM=c.E)
    y64 = DS.mixer_forward_reference(c, mp, qs, st, f64)
    y32 = DS.mixer_forward_reference(c, mp, qs, st, f32)
    std = st.to(device).view(R, 1, c.S)
    y_plain = _mixer(c, mp, device)(qs.to(device).view(R, 1, c.N), std)
    assert tuple(y_plain.shape) == (R, 1, 1) and not y_plain.requires_grad
    print(f"mixer {cid} R={R} (N={c.N} S={c.S} E={c.E} HE={c.HE} layers={c.layers})")
    _chk("mixer forward", "q_tot", y_plain.view(R), y64, y32)
    mx = _mixer(c, mp, device, enable=True)
    runs = []
    for _ in range(2):
        for prm in mx.parameters():
            prm.grad = None
        qd = qs.to(device).requires_grad_(True)
        out = mx(qd.view(R, 1, c.N), std)
        assert tuple(out.shape) == (R, 1, 1) and out.requires_grad
        assert torch.equal(out.detach(), y_plain)  # the autograd path gives the plain path's bits
        out.backward(g_out.to(device).view(R, 1, 1))
        runs.append({**{k: v.grad.clone() for k, v in mx.named_parameters()}, "d_agent_qs": qd.grad.clone()})
    assert set(runs[0]) == set(ref)
    for k in ref:
        assert torch.equal(runs[0][k], runs[1][k]), k
        _chk("mixer gradients", k, runs[0][k], ref[k], r32[k])
    _report("mixer forward")
    _report("mixer gradients")


def test_mixer_golden(device, golden):
    """The reference's own QMixer.forward vector (read by the CPU oracle's test only, so far) through the kernel."""
    from maleague.modules.mixers import QMixer
    d = golden("qmix_fwd.npz")
    mx = QMixer(qmix_args(device=str(device)))
    mx.load_state_dict({k[2:]: torch.from_numpy(np.array(d[k])) for k in d.files if k.startswith("p.")})
    y = mx(torch.from_numpy(d["agent_qs"]).to(device), torch.from_numpy(d["states"]).to(device))
    assert tuple(y.shape) == tuple(d["q_tot"].shape)
    np.testing.assert_allclose(y.cpu().numpy(), d["q_tot"], rtol=0, atol=1e-4)


# ---- D. mlg_agent_backward: the added edges -------------------------------------------------------------------------
@pytest.mark.parametrize("cid", DS.AGENT_GRAD_IDS)
def test_agent_gradients(device, cid):
    c = DS.agent_grad_case_of(cid)
    p, x, h, gq, gh = DS.agent_grad_inputs(c)
    ref = agent_reference(p, x, h, gq, gh, f64, check=True)
    r32 = agent_reference(p, x, h, gq, gh, f32)
    q64, h64 = DS.fwd_reference(p, x, h, f64)
    q32, h32 = DS.fwd_reference(p, x, h, f32)
    ag = _agent(device, DS.agent_grad_d_in(c), c.H, c.A, DS.GRAD_N, p, c.last_action, c.agent_id, enable=True)
    xd, hd = x.to(device).requires_grad_(True), h.to(device).requires_grad_(True)
    q, hn = ag(xd, hd)
    assert q.requires_grad and hn.requires_grad
    torch.autograd.backward([q, hn], [gq.to(device), gh.to(device)])
    print(f"agent gradients {cid}: R={c.R} H={c.H} A={c.A} last_action={c.last_action} agent_id={c.agent_id}")
    _chk("agent forward", "q", q.detach(), q64, q32)
    _chk("agent forward", "h'", hn.detach(), h64, h32)
    for k, v in ag.named_parameters():
        _chk("agent gradients", k, v.grad, ref[k], r32[k])
    _chk("agent gradients", "d_inputs", xd.grad, ref["d_inputs"], r32["d_inputs"])
    _chk("agent gradients", "d_h_in", hd.grad, ref["d_h_in"], r32["d_h_in"])
    _report("agent forward")
    _report("agent gradients")


# ---- E. direct backward calls into poisoned buffers -----------------------------------------------------------------
def _canary(n, device):
    return torch.arange(n, dtype=torch.float32, device=device) * 0.5 + 3.0


def _workspace_with_canary(n_ws, fill, device):
    """A workspace of exactly n_ws floats as the front of a larger tensor; the tail holds the canary pattern."""
    assert n_ws > 0 and n_ws % 4 == 0
    big = torch.full((n_ws + DS.CANARY_FLOATS,), fill, device=device)
    big[n_ws:] = _canary(DS.CANARY_FLOATS, device)
    assert big.data_ptr() % 16 == 0
    return big


def _qmix_backward_into(device, mx, qs, st, g_out, fill):
    from maleague import _native
    p, keep = mx._cparams()
    R = qs.shape[0]
    n_ws = int(_native.load().mlg_qmix_backward_workspace_floats(_native.byref(p), R))
    big = _workspace_with_canary(n_ws, fill, device)
    dparams = torch.full((sum(t.numel() for t in keep if t is not None),), fill, device=device)
    d_qs = torch.full((max(R, 1), p.n_agents), fill, device=device)
    _native.call("mlg_qmix_backward", _native.byref(p), _native.ptr(qs) if R else None, _native.ptr(st) if R else None,
                 _native.ptr(g_out) if R else None, _native.ptr(d_qs), _native.ptr(dparams), _native.ptr(big), R,
                 _native.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(big[n_ws:], _canary(DS.CANARY_FLOATS, device)), "the call wrote past the size its query reports"
    del keep
    return dparams, d_qs[:R]


def test_qmix_backward_poisoned(device):
    c = DS.mixer_case_of(DS.POISON_MIXER)
    R = DS.POISON_R
    mp, qs, st, g_out = DS.mixer_inputs(c, R)
    ref = mixer_reference(mp, qs, st, g_out, c.layers, c.N, f64, S_DIM=c.S, E_DIM=c.E)
    r32 = mixer_reference(mp, qs, st, g_out, c.layers, c.N, f32, S_DIM=c.S, E_DIM=c.E)
    mx = _mixer(c, mp, device)
    qd, sd, gd = qs.to(device), st.to(device), g_out.to(device)
    got_nan, dq_nan = _qmix_backward_into(device, mx, qd, sd, gd, NAN)
    got_zero, dq_zero = _qmix_backward_into(device, mx, qd, sd, gd, 0.0)
    assert not torch.isnan(got_nan).any() and not torch.isnan(dq_nan).any() and bool(got_nan.any())
    assert torch.equal(got_nan, got_zero) and torch.equal(dq_nan, dq_zero)
    print(f"mlg_qmix_backward into NaN-filled buffers, {DS.POISON_MIXER} R={R}")
    off = 0
    for k, v in mx.named_parameters():  # dparams: the parameters in named_parameters() order
        _chk("mixer gradients", k, got_nan[off:off + v.numel()].view(v.shape), ref[k], r32[k])
        off += v.numel()
    assert off == got_nan.numel()
    _chk("mixer gradients", "d_agent_qs", dq_nan, ref["d_agent_qs"], r32["d_agent_qs"])
    empty, _ = _qmix_backward_into(device, mx, qd[:0], sd[:0], gd[:0], NAN)
    assert torch.equal(empty, torch.zeros_like(empty))
    _report("mixer gradients")


def _agent_backward_into(device, ag, x, h, gq, gh, fill):
    from maleague import _native
    d = ag.dims()
    R = x.shape[0]
    fc1w, fc1b, wih, whh, bih, bhh, fc2w, fc2b = [t.detach().contiguous() for t in ag._live_params()]
    cparams = _native.MlgAgentParams(*[_native.ptr(t) for t in (fc1w, fc1b, wih, bih, whh, bhh, fc2w, fc2b)])
    n_ws = int(_native.load().mlg_agent_backward_workspace_floats(_native.byref(d), R))
    big = _workspace_with_canary(n_ws, fill, device)
    dparams = torch.full((sum(t.numel() for t in ag._live_params()),), fill, device=device)
    d_inputs = torch.full((max(R, 1), d.d_in), fill, device=device)
    d_h_in = torch.full((max(R, 1), d.hidden), fill, device=device)
    opt = lambda t: _native.ptr(t) if R else None  # noqa: E731
    _native.call("mlg_agent_backward", _native.byref(d), _native.byref(cparams), _native.ptr(ag.packed()), opt(x), opt(h),
                 opt(gq), opt(gh), _native.ptr(d_inputs), _native.ptr(d_h_in), _native.ptr(dparams), _native.ptr(big), R,
                 _native.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(big[n_ws:], _canary(DS.CANARY_FLOATS, device)), "the call wrote past the size its query reports"
    return dparams, d_inputs[:R], d_h_in[:R]


def test_agent_backward_poisoned(device):
    c = DS.agent_grad_case_of(DS.POISON_AGENT)
    p, x, h, gq, gh = DS.agent_grad_inputs(c)
    ref = agent_reference(p, x, h, gq, gh, f64)
    r32 = agent_reference(p, x, h, gq, gh, f32)
    ag = _agent(device, DS.agent_grad_d_in(c), c.H, c.A, DS.GRAD_N, p)
    dev = [t.to(device) for t in (x, h, gq, gh)]
    nan_run = _agent_backward_into(device, ag, *dev, NAN)
    zero_run = _agent_backward_into(device, ag, *dev, 0.0)
    for a, b in zip(nan_run, zero_run):
        assert not torch.isnan(a).any() and bool(a.any()) and torch.equal(a, b)
    print(f"mlg_agent_backward into NaN-filled buffers, {DS.POISON_AGENT}")
    off = 0
    for k, v in ag.named_parameters():
        _chk("agent gradients", k, nan_run[0][off:off + v.numel()].view(v.shape), ref[k], r32[k])
        off += v.numel()
    assert off == nan_run[0].numel()
    _chk("agent gradients", "d_inputs", nan_run[1], ref["d_inputs"], r32["d_inputs"])
    _chk("agent gradients", "d_h_in", nan_run[2], ref["d_h_in"], r32["d_h_in"])
    empty = _agent_backward_into(device, ag, *[t[:0] for t in dev], NAN)[0]
    assert torch.equal(empty, torch.zeros_like(empty))
    _report("agent gradients")


# ---- F. mlg_select_actions ------------------------------------------------------------------------------------------
def _select(device, q, av, keys=None, episodes=None, t=0, eps=0.0, want_greedy=True):
    from maleague import _native
    B, N, A = q.shape
    qd, ad = torch.from_numpy(q).to(device), torch.from_numpy(av).to(device)
    kd = None if keys is None else torch.from_numpy(keys.view(np.int64)).to(device)
    ed = None if episodes is None else torch.from_numpy(episodes).to(device)
    acts = torch.full((B, N), -1, dtype=torch.int64, device=device)
    greedy = torch.full((B, N), -1, dtype=torch.int64, device=device) if want_greedy else None
    _native.call("mlg_select_actions", _native.ptr(qd), _native.ptr(ad), B * N, A, N, _native.ptr(kd), _native.ptr(ed),
                 int(t), float(eps), _native.ptr(acts), _native.ptr(greedy), _native.stream_ptr())
    torch.cuda.synchronize()
    return acts.cpu().numpy(), None if greedy is None else greedy.cpu().numpy()


@pytest.mark.parametrize("B,N,A", DS.GREEDY_SHAPES)
def test_select_greedy(device, B, N, A):
    q, av, rows = DS.select_case(B, N, A)
    exp = LR.greedy_select(torch.from_numpy(q), torch.from_numpy(av)).numpy()
    acts, greedy = _select(device, q, av)
    np.testing.assert_array_equal(acts, exp)
    assert (greedy == 1).all()
    acts2, none = _select(device, q, av, want_greedy=False)  # is_greedy = NULL
    assert none is None
    np.testing.assert_array_equal(acts2, exp)
    for r in rows["masked"]:
        assert acts.reshape(-1)[r] == 0
    print(f"select greedy B={B} N={N} A={A}: {B * N} rows, {len(rows['tie'])} tie rows, "
          f"{len(rows['max_unavailable'])} with the maximum unavailable, {len(rows['masked'])} fully masked")


@pytest.mark.parametrize("with_episodes", [True, False], ids=["episodes", "episodes-null"])
@pytest.mark.parametrize("t", DS.EPS_T)
@pytest.mark.parametrize("eps", DS.EPS_VALUES)
@pytest.mark.parametrize("B,N,A", DS.EPS_SHAPES)
def test_select_epsilon(device, B, N, A, eps, t, with_episodes):
    q, av, _ = DS.select_case(B, N, A, masked_row=False)
    keys, episodes = DS.select_keys(B)
    exp, exp_g = LR.eps_select(torch.from_numpy(q), torch.from_numpy(av), eps, [int(k) for k in keys],
                               episodes.tolist() if with_episodes else [0] * B, t)
    acts, greedy = _select(device, q, av, keys, episodes if with_episodes else None, t, eps)
    np.testing.assert_array_equal(acts, exp)
    np.testing.assert_array_equal(greedy, exp_g)
    if eps == 1.0:
        assert not greedy.any()
    else:
        assert 0 < greedy.sum() < greedy.size
