"""GPU parity of the autograd path (maleague::drqn_forward / qmix_forward with the HIP backward kernels
mlg_agent_backward / mlg_qmix_backward) against torch autograd over the CPU oracle (oracle/learner_ref.py) in
float64.

Tolerance, for every gradient tensor: max|g - g_ref| <= 1e-4 * max(1, max|g_ref|) -- the project's fp32 parity
bound, applied per tensor. Each check prints its error next to the error of the same oracle run in float32, so the
margin is visible (`pytest -s`).

The reference derivative jumps where a ReLU or abs argument is zero, so a comparison only means something away from
those points: the tests assert on the ORACLE's values (never on the kernels') that every such argument is further
from zero than 8 eps32 * (|w| . |x| + |b|), eight times the first-order rounding error of an fp32 dot product of
those terms; the seeds were chosen on the CPU so that this, and the both-signs conditions, hold.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import learner_ref as LR
from helpers import qmix_args, scheme_for

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
D_OBS, N_AGENTS, S_DIM, E_DIM, HE_DIM = 80, 5, 60, 32, 64
f64 = torch.float64


def _check(name, got, ref64, ref32=None):
    ref64 = ref64.detach()
    err = float((got.detach().cpu().to(f64) - ref64).abs().max()) if ref64.numel() else 0.0
    scale = max(1.0, float(ref64.abs().max())) if ref64.numel() else 1.0
    o32 = float("nan") if ref32 is None else float((ref32.detach().to(f64) - ref64).abs().max())
    print(f"  {name:28s} err {err:.3e}  bound {1e-4 * scale:.3e}  (fp32 CPU oracle vs float64: {o32:.3e})")
    assert err <= 1e-4 * scale, f"{name}: max error {err:.3e} > {1e-4 * scale:.3e}"
    return err / scale


def _clear_of_kinks(what, pre, x, w, b):
    """Oracle-side input check: every ReLU / abs argument clear of zero by 8x its fp32 rounding error."""
    margin = 8 * EPS32 * (F.linear(x.abs(), w.abs(), b.abs()))
    assert bool((pre.abs() > margin).all()), f"{what}: an argument within rounding error of a kink; pick another seed"


# ---- agent step ----------------------------------------------------------------------------------------------
def agent_case(R, H, A, seed, h_zero=False, d_in=None):
    """Seeded parameters (state_dict names), inputs, hidden state and upstream gradients, float32 on the CPU.
    d_in: the input width when it is not the fixture's [obs | last action | agent id] (tests/drqn_op_shapes.py)."""
    g = torch.Generator().manual_seed(seed)
    d_in = D_OBS + A + N_AGENTS if d_in is None else d_in
    u = lambda *s, k=1.0: (torch.rand(*s, generator=g) * 2 - 1) * k  # noqa: E731
    p = {"fc1.weight": u(H, d_in, k=0.15), "fc1.bias": u(H, k=0.3), "gru.weight_ih": u(3 * H, H, k=0.25),
         "gru.weight_hh": u(3 * H, H, k=0.25), "gru.bias_ih": u(3 * H, k=0.3), "gru.bias_hh": u(3 * H, k=0.3),
         "fc2.weight": u(A, H, k=0.25), "fc2.bias": u(A, k=0.3)}
    x = torch.randn(R, d_in, generator=g)
    h = torch.zeros(R, H) if h_zero else torch.randn(R, H, generator=g) * 0.7
    return p, x, h, torch.randn(R, A, generator=g), torch.randn(R, H, generator=g)


def agent_reference(p, x, h, gq, gh, dtype, check=False):
    """Gradients of sum(q gq) + sum(h' gh) by torch autograd over the oracle's DRQN step."""
    pp = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p.items()}
    xx, hh = (t.detach().clone().to(dtype).requires_grad_(True) for t in (x, h))
    if check:
        pre = F.linear(xx, pp["fc1.weight"], pp["fc1.bias"]).detach()
        assert bool((pre > 0).any()) and bool((pre < 0).any()), "fc1 pre-activation must have both signs"
        _clear_of_kinks("fc1", pre, xx.detach(), pp["fc1.weight"].detach(), pp["fc1.bias"].detach())
    q, hn = LR.drqn_forward(pp, xx, hh)
    loss = 0
    if gq is not None:
        loss = loss + (q * gq.to(dtype)).sum()
    if gh is not None:
        loss = loss + (hn * gh.to(dtype)).sum()
    loss.backward()
    out = {k: v.grad for k, v in pp.items()}
    out["d_inputs"], out["d_h_in"] = xx.grad, hh.grad
    return out


def _make_agent(p, H, A, device, enable=True):
    from maleague.modules.agents.drqn_agent import DRQNAgentNetwork
    ag = DRQNAgentNetwork(D_OBS + A + N_AGENTS, qmix_args(n_agents=N_AGENTS, n_actions=A, rnn_hidden_dim=H))
    ag.load_state_dict(p)
    return ag.enable_autograd() if enable else ag


# seeds chosen on the CPU (both signs of the fc1 pre-activation, clear of kinks); see the module docstring
AGENT_SEEDS = {(4113, 64, 15): 5}


def _agent_seed(R, H, A):
    return AGENT_SEEDS.get((R, H, A), 1)


def _run_agent(device, R, H, A, use_q=True, use_h=True, h_zero=False):
    p, x, h, gq, gh = agent_case(R, H, A, _agent_seed(R, H, A), h_zero)
    gq, gh = (gq if use_q else None), (gh if use_h else None)
    ref = agent_reference(p, x, h, gq, gh, f64, check=True)
    r32 = agent_reference(p, x, h, gq, gh, torch.float32)
    ag = _make_agent(p, H, A, device)
    xd = x.to(device).requires_grad_(True)
    if h_zero:
        hd = ag.init_hidden().expand(R, -1)
    else:
        hd = h.to(device).requires_grad_(True)
    q, hn = ag(xd, hd)
    assert q.requires_grad and hn.requires_grad
    outs, grads = [], []
    if use_q:
        outs.append(q), grads.append(gq.to(device))
    if use_h:
        outs.append(hn), grads.append(gh.to(device))
    torch.autograd.backward(outs, grads)
    print(f"agent R={R} H={H} A={A} q={use_q} h={use_h} h_zero={h_zero}")
    for k, v in ag.named_parameters():
        if ref[k] is None:  # fc2 when only h' is used
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, k
            continue
        _check(k, v.grad, ref[k], r32[k])
    _check("d_inputs", xd.grad, ref["d_inputs"], r32["d_inputs"])
    if not h_zero:
        _check("d_h_in", hd.grad, ref["d_h_in"], r32["d_h_in"])


@pytest.mark.parametrize("A", [15, 21])
@pytest.mark.parametrize("H", [32, 64, 128])
@pytest.mark.parametrize("R", [1, 17, 37])
def test_agent_step_gradients(device, R, H, A):
    _run_agent(device, R, H, A)


def test_agent_step_gradients_many_rows(device):
    """4113 rows: past one group of four 1024-row weight-gradient chunks, plus a ragged 16-row tile."""
    _run_agent(device, 4113, 64, 15)


@pytest.mark.parametrize("kw", [dict(use_h=False), dict(use_q=False), dict(h_zero=True)],
                         ids=["only_q", "only_h_out", "h_in_from_init_hidden"])
def test_agent_step_partial_gradients(device, kw):
    _run_agent(device, 37, 64, 15, **kw)


# ---- mixer ---------------------------------------------------------------------------------------------------
def mixer_case(layers, N, R, seed):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s, k=1.0: (torch.rand(*s, generator=g) * 2 - 1) * k  # noqa: E731
    S, E, HE = S_DIM, E_DIM, HE_DIM
    mp = {}

    def lin(name, o, i, k):
        mp[f"{name}.weight"], mp[f"{name}.bias"] = u(o, i, k=k), u(o, k=0.3)

    if layers == 2:
        lin("hyper_w_1.0", HE, S, 0.2), lin("hyper_w_1.2", N * E, HE, 0.2)
        lin("hyper_w_final.0", HE, S, 0.2), lin("hyper_w_final.2", E, HE, 0.2)
    else:
        lin("hyper_w_1", N * E, S, 0.2), lin("hyper_w_final", E, S, 0.2)
    lin("hyper_b_1", E, S, 0.2), lin("V.0", E, S, 0.2), lin("V.2", 1, E, 0.3)
    # agent_qs of both signs and O(1): the ELU argument sum_n q_n |w1_ne| + b1_e then takes both signs
    return mp, torch.randn(R, N, generator=g) * 1.5, torch.randn(R, S_DIM, generator=g), torch.randn(R, generator=g)


def mixer_reference(mp, qs, st, g_out, layers, N, dtype, check=False, S_DIM=S_DIM, E_DIM=E_DIM):
    """S_DIM / E_DIM: the state and embedding widths when they are not the fixture's (tests/drqn_op_shapes.py)."""
    pp = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in mp.items()}
    q, s = qs.detach().clone().to(dtype).requires_grad_(True), st.to(dtype)
    if check:
        d = {k: v.detach() for k, v in pp.items()}
        for name in ("hyper_w_1", "hyper_w_final"):
            if layers == 2:
                pre0 = F.linear(s, d[f"{name}.0.weight"], d[f"{name}.0.bias"])
                _clear_of_kinks(name + ".0", pre0, s, d[f"{name}.0.weight"], d[f"{name}.0.bias"])
                a = F.relu(pre0)
                _clear_of_kinks(name + ".2", F.linear(a, d[f"{name}.2.weight"], d[f"{name}.2.bias"]), a,
                                d[f"{name}.2.weight"], d[f"{name}.2.bias"])
            else:
                _clear_of_kinks(name, F.linear(s, d[f"{name}.weight"], d[f"{name}.bias"]), s, d[f"{name}.weight"],
                                d[f"{name}.bias"])
        _clear_of_kinks("V.0", F.linear(s, d["V.0.weight"], d["V.0.bias"]), s, d["V.0.weight"], d["V.0.bias"])

        def mlp(prefix):
            if layers == 2:
                return F.linear(F.relu(F.linear(s, d[f"{prefix}.0.weight"], d[f"{prefix}.0.bias"])),
                                d[f"{prefix}.2.weight"], d[f"{prefix}.2.bias"])
            return F.linear(s, d[f"{prefix}.weight"], d[f"{prefix}.bias"])

        w1 = mlp("hyper_w_1").abs().view(-1, N, E_DIM)
        pre = torch.bmm(q.detach().view(-1, 1, N), w1).squeeze(1) + F.linear(s, d["hyper_b_1.weight"],
                                                                            d["hyper_b_1.bias"])
        assert bool((pre > 0).any()) and bool((pre < 0).any()), "ELU pre-activation must have both signs"
    out = LR.qmix_forward(pp, q.view(-1, 1, N), s.view(-1, 1, S_DIM), N, E_DIM, layers).view(-1)
    (out * g_out.to(dtype)).sum().backward()
    res = {k: v.grad for k, v in pp.items()}
    res["d_agent_qs"] = q.grad
    return res


def _make_mixer(mp, layers, N, device, enable=True):
    from maleague.modules.mixers import QMixer
    mx = QMixer(qmix_args(n_agents=N, hypernet_layers=layers, state_shape=S_DIM, mixing_embed_dim=E_DIM,
                          hypernet_embed=HE_DIM))
    mx.load_state_dict(mp)
    return mx.enable_autograd() if enable else mx


MIXER_SEEDS = {(1, 5, 4113): 3, (2, 3, 4113): 2, (2, 5, 4113): 14}  # as AGENT_SEEDS; every other case: seed 1


@pytest.mark.parametrize("R", [1, 129, 4113])
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("layers", [1, 2])
def test_mixer_gradients(device, layers, N, R):
    mp, qs, st, g_out = mixer_case(layers, N, R, MIXER_SEEDS.get((layers, N, R), 1))
    ref = mixer_reference(mp, qs, st, g_out, layers, N, f64, check=True)
    r32 = mixer_reference(mp, qs, st, g_out, layers, N, torch.float32)
    mx = _make_mixer(mp, layers, N, device)
    qd = qs.to(device).requires_grad_(True)
    out = mx(qd.view(R, 1, N), st.to(device).view(R, 1, S_DIM))
    assert out.shape == (R, 1, 1) and out.requires_grad
    out.backward(g_out.to(device).view(R, 1, 1))
    print(f"mixer layers={layers} N={N} R={R}")
    for k, v in mx.named_parameters():
        _check(k, v.grad, ref[k], r32[k])
    _check("d_agent_qs", qd.grad, ref["d_agent_qs"], r32["d_agent_qs"])


# ---- the reference-style learner loop ------------------------------------------------------------------------
T_STEPS = 6


def chain_batch(B, A, seed):
    """A random filled / terminated batch [B, T_STEPS, ...] with episode 1 ending mid-way (CPU tensors)."""
    g = torch.Generator().manual_seed(seed)
    T, N = T_STEPS, N_AGENTS
    avail = (torch.rand(B, T, N, A, generator=g) < 0.7).int()
    actions = torch.randint(0, A, (B, T, N, 1), generator=g)
    avail.scatter_(3, actions.int().long(), 1)  # the taken action is available
    term = torch.zeros(B, T, 1, dtype=torch.uint8)
    filled = torch.ones(B, T, 1, dtype=torch.long)
    term[1, 2] = 1
    filled[1, 4:] = 0
    term[0, T - 2] = 1
    return {"state": torch.randn(B, T, S_DIM, generator=g), "obs": torch.randn(B, T, N, D_OBS, generator=g),
            "actions": actions, "avail_actions": avail, "reward": torch.randn(B, T, 1, generator=g),
            "terminated": term, "filled": filled, "actions_onehot": F.one_hot(actions.squeeze(3), A).float()}


def td_loss(unroll, mix, b, args):
    """The loss of the reference learner (q_learner.py:47-103) over `unroll(online) -> [B, T, N, A]` and
    `mix(online, qs [B, T-1, N], states) -> [B, T-1, 1]`."""
    rewards, actions = b["reward"][:, :-1], b["actions"][:, :-1]
    terminated = b["terminated"][:, :-1].to(rewards.dtype)
    mask = b["filled"][:, :-1].to(rewards.dtype).clone()
    mask[:, 1:] = mask[:, 1:] * (1 - terminated[:, :-1])
    avail = b["avail_actions"]
    mac_out = unroll(True)
    chosen = torch.gather(mac_out[:, :-1], dim=3, index=actions).squeeze(3)
    with torch.no_grad():
        tmac = unroll(False)[:, 1:].clone()
        tmac[avail[:, 1:] == 0] = -9999999
        if args.double_q:
            md = mac_out.clone().detach()
            md[avail == 0] = -9999999
            target_max = torch.gather(tmac, 3, md[:, 1:].max(dim=3, keepdim=True)[1]).squeeze(3)
        else:
            target_max = tmac.max(dim=3)[0]
        target_max = mix(False, target_max, b["state"][:, 1:])
    chosen = mix(True, chosen, b["state"][:, :-1])
    targets = rewards + args.gamma * (1 - terminated) * target_max
    td = chosen - targets.detach()
    mask = mask.expand_as(td)
    return ((td * mask) ** 2).sum() / mask.sum()


def _episode_batch(b, device):
    from maleague.components.episode_batch import EpisodeBatch
    B, T, N, _ = b["obs"].shape
    info = {"state_shape": b["state"].shape[-1], "obs_shape": b["obs"].shape[-1],
            "n_actions": b["avail_actions"].shape[-1], "n_agents": N}
    scheme, groups, preprocess = scheme_for(info, torch)
    eb = EpisodeBatch(scheme, groups, B, T, preprocess=preprocess, device=device)
    for k, v in b.items():
        eb.data.transition_data[k].copy_(v)
    return eb


class _Log:
    def log_stat(self, *a):
        pass

    def info(self, *a):
        pass


def _chain_setup(device, B, mixer, seed=5):
    """mac + mixer (and equal targets) with seeded weights, the batch on both sides, and the float64 reference."""
    from maleague.controllers import BasicMAC
    A = 15
    args = qmix_args(mixer=mixer, n_agents=N_AGENTS, n_actions=A, state_shape=S_DIM)
    b = chain_batch(B, A, seed)
    eb = _episode_batch(b, device)
    p = agent_case(1, 64, A, seed)[0]
    mp = mixer_case(2, N_AGENTS, 1, seed)[0]
    mac = BasicMAC(eb.scheme, eb.groups, args)
    mac.load_state_dict(p)
    mac.enable_autograd()
    target_mac = copy.deepcopy(mac)
    mx = _make_mixer(mp, 2, N_AGENTS, device) if mixer == "qmix" else None
    target_mx = copy.deepcopy(mx)
    return args, b, eb, p, mp, mac, target_mac, mx, target_mx


def _gpu_loss(args, eb, mac, target_mac, mx, target_mx):
    def unroll(online):
        m = mac if online else target_mac
        m.init_hidden(eb.batch_size)
        return torch.stack([m.forward(eb, t) for t in range(eb.max_seq_length)], dim=1)

    def mix(online, qs, states):
        if args.mixer == "vdn":
            return qs.sum(dim=2, keepdim=True)
        return (mx if online else target_mx)(qs, states)

    return td_loss(unroll, mix, {k: eb[k] for k in ("reward", "actions", "terminated", "filled", "avail_actions",
                                                     "state")}, args)


def _ref_loss(args, b, p, mp, dtype):
    pp = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p.items()}
    mpp = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in mp.items()}
    bb = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in b.items()}
    B = bb["obs"].shape[0]

    def unroll(online):
        return LR.mac_unroll(pp, bb, N_AGENTS, h0=torch.zeros(B * N_AGENTS, 64, dtype=dtype))[0]

    def mix(online, qs, states):
        if args.mixer == "vdn":
            return qs.sum(dim=2, keepdim=True)
        return LR.qmix_forward(mpp, qs, states, N_AGENTS, E_DIM, 2)

    loss = td_loss(unroll, mix, bb, args)
    loss.backward()
    return loss.detach(), pp, mpp


@pytest.mark.parametrize("mixer", ["qmix", "vdn"])
@pytest.mark.parametrize("B", [3, 4])
def test_reference_style_loop(device, B, mixer):
    """mac.forward over t, gather, QMixer, masked TD loss, loss.backward(): the loss and every agent and mixer gradient
    equal autograd over the oracle's mac_unroll + qmix_forward. B * 5 = 15 / 20 rows: below / above one tile."""
    args, b, eb, p, mp, mac, target_mac, mx, target_mx = _chain_setup(device, B, mixer)
    loss = _gpu_loss(args, eb, mac, target_mac, mx, target_mx)
    loss.backward()
    ref_loss, pp, mpp = _ref_loss(args, b, p, mp, f64)
    loss32, pp32, mpp32 = _ref_loss(args, b, p, mp, torch.float32)
    print(f"chain B={B} mixer={mixer}")
    _check("loss", loss, ref_loss, loss32)
    for k, v in mac.agent.named_parameters():
        _check(k, v.grad, pp[k].grad, pp32[k].grad)
    if mixer == "qmix":
        for k, v in mx.named_parameters():
            _check(k, v.grad, mpp[k].grad, mpp32[k].grad)


def test_gradients_match_fused_learner(device):
    """Two independent HIP paths: the autograd gradients of the reference-style loss, clipped, against the clipped
    gradients mlg_qlearner_train leaves in QLearner._grads (same batch and weights, targets equal to online)."""
    from maleague.controllers import BasicMAC
    from maleague.learners import QLearner
    args, b, eb, p, mp, mac, target_mac, mx, target_mx = _chain_setup(device, 4, "qmix")
    _gpu_loss(args, eb, mac, target_mac, mx, target_mx).backward()
    params = list(mac.parameters()) + list(mx.parameters())
    torch.nn.utils.clip_grad_norm_(params, args.grad_norm_clip)
    mac2 = BasicMAC(eb.scheme, eb.groups, args)
    mac2.load_state_dict(p)
    learner = QLearner(mac2, eb.scheme, _Log(), args, name="home")
    learner.mixer.load_state_dict(mp)
    learner.target_mixer.load_state_dict(mp)
    learner.build_optimizer()
    learner.train(eb, 0, 0)
    print("autograd vs fused learner")
    for (q, off, k), mine in zip(learner._flat.views, params):
        _check(f"param {off}", mine.grad, learner._grads[off:off + k].view_as(q).cpu().to(f64))


# ---- determinism, opt-in, errors, opcheck, compile -----------------------------------------------------------
def _agent_op_args(device, R=4113, H=64, A=15, requires_grad=False):
    from maleague.ops import struct_fields
    p, x, h, gq, gh = agent_case(R, H, A, 3)
    ag = _make_agent(p, H, A, device)
    params = [v.detach().clone().requires_grad_(requires_grad) for v in ag._live_params()]
    return ag, params, [t.to(device) for t in (x, h, gq, gh)], struct_fields(ag.dims())


def _mixer_op_args(device, R=4113, layers=2, requires_grad=False):
    mp, qs, st, g_out = mixer_case(layers, N_AGENTS, R, 3)
    mx = _make_mixer(mp, layers, N_AGENTS, device)
    _, keep = mx._cparams()
    empty = torch.empty(0, device=device)
    params = [empty if t is None else t.clone().requires_grad_(requires_grad) for t in keep]
    return params, [t.to(device) for t in (qs, st, g_out)], [N_AGENTS, S_DIM, E_DIM, HE_DIM if layers == 2 else 0,
                                                            layers]


def test_backward_is_deterministic(device):
    ag, params, (x, h, gq, gh), dims = _agent_op_args(device)
    a = torch.ops.maleague.drqn_backward(params, ag.packed(), x, h, gq, gh, dims)
    b = torch.ops.maleague.drqn_backward(params, ag.packed(), x, h, gq, gh, dims)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    mparams, (qs, st, g_out), mdims = _mixer_op_args(device)
    a = torch.ops.maleague.qmix_backward(mparams, qs, st, g_out, mdims)
    b = torch.ops.maleague.qmix_backward(mparams, qs, st, g_out, mdims)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_empty_batch_zeroes_parameter_gradients(device):
    ag, params, (x, h, gq, gh), dims = _agent_op_args(device, R=16)
    dx, dh, dflat = torch.ops.maleague.drqn_backward(params, ag.packed(), x[:0], h[:0], gq[:0], gh[:0], dims)
    assert dx.shape == (0, x.shape[1]) and dh.shape == (0, 64) and float(dflat.abs().max()) == 0.0
    mparams, (qs, st, g_out), mdims = _mixer_op_args(device, R=16)
    dq, mflat = torch.ops.maleague.qmix_backward(mparams, qs[:0], st[:0], g_out[:0], mdims)
    assert dq.shape == (0, N_AGENTS) and float(mflat.abs().max()) == 0.0


def test_opt_in_leaves_default_path_unchanged(device):
    p, x, h, _, _ = agent_case(37, 64, 15, 2)
    plain, live = _make_agent(p, 64, 15, device, enable=False), _make_agent(p, 64, 15, device)
    q0, h0 = plain(x.to(device), h.to(device))
    q1, h1 = live(x.to(device), h.to(device))
    assert not q0.requires_grad and not h0.requires_grad and q1.requires_grad and h1.requires_grad
    assert torch.equal(q0, q1) and torch.equal(h0, h1)
    with torch.no_grad():
        q2, _ = live(x.to(device), h.to(device))
    assert not q2.requires_grad and torch.equal(q2, q0)
    mp, qs, st, _ = mixer_case(2, N_AGENTS, 37, 2)
    mplain, mlive = _make_mixer(mp, 2, N_AGENTS, device, enable=False), _make_mixer(mp, 2, N_AGENTS, device)
    qs, st = qs.to(device).view(37, 1, N_AGENTS), st.to(device).view(37, 1, S_DIM)
    y0, y1 = mplain(qs, st), mlive(qs, st)
    assert not y0.requires_grad and y1.requires_grad and torch.equal(y0, y1)


@pytest.mark.parametrize("flat", [False, True], ids=["module_params", "flat_param_views"])
def test_torch_optimizer_step_reaches_the_kernels(device, flat):
    """Parameters stepped by torch.optim.RMSprop (also as the learner's FlatParams views): the next forward differs
    and equals a fresh module loaded with the stepped state dict (the packed block follows the parameters)."""
    from maleague.learners.q_learner import FlatParams
    p, x, h, gq, _ = agent_case(20, 64, 15, 4)
    ag = _make_agent(p, 64, 15, device)
    mp, qs, st, _ = mixer_case(2, N_AGENTS, 20, 4)
    mx = _make_mixer(mp, 2, N_AGENTS, device)
    params = list(ag.parameters()) + list(mx.parameters())
    if flat:
        keep = FlatParams(params, device)  # noqa: F841
        ag.mark_dirty()
    x, h, st = x.to(device), h.to(device), st.to(device).view(20, 1, S_DIM)

    def forward(a, m):
        q, _ = a(x, h)
        return q, m(q[:, :N_AGENTS].reshape(20, 1, N_AGENTS), st)

    opt = torch.optim.RMSprop(params, lr=1e-2)
    q0, y0 = forward(ag, mx)
    (y0.sum() + (q0 * gq.to(device)).sum()).backward()
    opt.step()
    q1, y1 = forward(ag, mx)
    assert not torch.equal(q0, q1) and not torch.equal(y0, y1)
    fresh_a = _make_agent({k: v.detach().cpu() for k, v in ag.state_dict().items()}, 64, 15, device, enable=False)
    fresh_m = _make_mixer({k: v.detach().cpu() for k, v in mx.state_dict().items()}, 2, N_AGENTS, device, enable=False)
    q2, y2 = forward(fresh_a, fresh_m)
    assert torch.equal(q1.detach(), q2) and torch.equal(y1.detach(), y2)


def test_documented_errors(device):
    from maleague._native import NativeError
    mp, qs, st, _ = mixer_case(2, N_AGENTS, 8, 2)
    mx = _make_mixer(mp, 2, N_AGENTS, device)
    qs, st = qs.to(device).view(8, 1, N_AGENTS), st.to(device).view(8, 1, S_DIM)
    with pytest.raises(NativeError, match="states are not implemented"):
        mx(qs, st.clone().requires_grad_())
    y = mx(qs, st)
    (g,) = torch.autograd.grad(y.sum(), mx.hyper_b_1.weight, create_graph=True)
    with pytest.raises(RuntimeError, match="qmix_backward"):
        g.sum().backward()
    p, x, h, _, _ = agent_case(8, 64, 15, 2)
    ag = _make_agent(p, 64, 15, device)
    q, _ = ag(x.to(device), h.to(device))
    (g,) = torch.autograd.grad(q.sum(), ag.fc1.weight, create_graph=True)
    with pytest.raises(RuntimeError, match="drqn_backward"):
        g.sum().backward()


def test_opcheck(device):
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    ag, params, (x, h, _, _), dims = _agent_op_args(device, R=20, requires_grad=True)
    torch.library.opcheck(torch.ops.maleague.drqn_forward.default, (params, ag.packed(), x, h, dims),
                          test_utils=utils)
    for layers in (1, 2):
        mparams, (qs, st, _), mdims = _mixer_op_args(device, R=20, layers=layers, requires_grad=True)
        torch.library.opcheck(torch.ops.maleague.qmix_forward.default, (mparams, qs, st, mdims), test_utils=utils)


def test_compiled_loss_gradients_match_eager(device):
    """A scalar loss of drqn_forward under torch.compile(backend="aot_eager", fullgraph=True): AOT autograd traces
    the backward through the fake implementations; the parameter gradients equal eager's bit for bit."""
    ag, params, (x, h, gq, gh), dims = _agent_op_args(device, R=20, requires_grad=True)
    packed = ag.packed()

    def loss_fn(ps, xx, hh):
        q, hn = torch.ops.maleague.drqn_forward(ps, packed, xx, hh, dims)
        return (q * gq).sum() + (hn * gh).sum()

    def grads(fn):
        for t in params:
            t.grad = None
        loss = fn(params, x, h)
        loss.backward()
        return loss.detach(), [t.grad.clone() for t in params]

    l0, g0 = grads(loss_fn)
    l1, g1 = grads(torch.compile(loss_fn, backend="aot_eager", fullgraph=True))
    assert torch.allclose(l0, l1, rtol=1e-6, atol=0)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
