"""GPU parity of the REFIL autograd path (maleague::refil_attention / flex_qmix_forward / entity_agent_forward with the
HIP backward kernels mlg_refil_attention_backward / mlg_refil_mixer_backward / mlg_refil_agent_backward) against torch
autograd over the CPU oracle (oracle/refil_ref.py attn_layer / flex_qmix / entity_agent) in float64.

Tolerance, for every gradient tensor: max|g - g_ref| <= 1e-4 * max(1, max|g_ref|) -- the project's fp32 parity bound
(tests/test_gpu_autograd.py), applied per tensor. Each check prints its error next to the error of the same oracle run
in float32, so the margin is visible (`pytest -s`). With softmax mixing weights g_qtot is drawn with std 8 so that the
largest gradients are O(1) and the bound is not vacuous.

The forward outputs of the three ops (y, q_tot, q and hs) are held to the same rule against the same float64 oracle
run, at every parametrised shape: the kernels' values, not only their equality with the no-autograd call. As in
tests/test_gpu_learner_shapes.py, where ten times the fp32 oracle's own distance from float64 exceeds the bound the
bound is ten times that distance; measured on the CPU, no case here is widened (the largest fp32 distance is 6.2e-6,
q_tot at R = 130 without softmax, against a bound of 2.8e-3; for the agent 6.5e-7 against 1.5e-4).

The reference derivative jumps where a ReLU or abs argument is zero, so a comparison only means something away from
those points: the tests assert on the ORACLE's values (never on the kernels') that every ReLU argument (entity fc1,
agent fc2, hypernet fc1) and every abs argument on a live agent row (mixer fc2 output without softmax) is further from
zero than 8 eps32 * (|w| . |x| + |b|), and that the fc1 pre-activation and the ELU argument take both signs; the
seeds (AGENT_SEEDS, MIXER_SEEDS) were chosen on the CPU so that this holds. Entity-masked agent rows are exact zeros
behind a masked_fill and are exempt from the abs check; the attention layer alone has no kink.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import refil_ref as RR
from helpers import entity_scheme_for, refil_args

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
ED = 8
f64 = torch.float64
HYPERS = ("hyper_w_1", "hyper_w_final", "hyper_b_1", "V")


def _check(name, got, ref64, ref32=None, forward=False):
    """forward: a forward value: shapes must agree, and where ten times the fp32 oracle's own distance from float64
    exceeds the bound, the bound is ten times that distance (module docstring)."""
    ref64 = ref64.detach()
    if forward:
        assert tuple(got.shape) == tuple(ref64.shape), (name, tuple(got.shape), tuple(ref64.shape))
    err = float((got.detach().cpu().to(f64) - ref64).abs().max()) if ref64.numel() else 0.0
    scale = max(1.0, float(ref64.abs().max())) if ref64.numel() else 1.0
    o32 = float("nan") if ref32 is None else float((ref32.detach().to(f64) - ref64).abs().max())
    bound = 1e-4 * scale
    if forward:
        assert ref32 is not None
        bound = max(bound, 10 * o32)
    print(f"  {name:36s} err {err:.3e}  bound {bound:.3e}  max|{'y' if forward else 'g'}| "
          f"{float(ref64.abs().max()):.3e}  (fp32 CPU oracle vs float64: {o32:.3e})")
    assert err <= bound, f"{name}: max error {err:.3e} > {bound:.3e}"


def _clear_of_kinks(what, pre, x, w, b, rows=None):
    """Oracle-side input check: every ReLU / abs argument clear of zero by 8x its fp32 rounding error."""
    ok = pre.abs() > 8 * EPS32 * F.linear(x.abs(), w.abs(), b.abs())
    if rows is not None:
        ok = ok | ~rows.unsqueeze(-1)
    assert bool(ok.all()), f"{what}: an argument within rounding error of a kink; pick another seed"


def _both_signs(what, pre):
    assert bool((pre > 0).any()) and bool((pre < 0).any()), f"{what} must take both signs; pick another seed"


def _u(g, *s, k=1.0):
    """Uniform in [-k, k]."""
    return (torch.rand(*s, generator=g) * 2 - 1) * k


def _entity_mask(g, R, NA, NE):
    """About 0.3 masked, entity 0 alive, at least one masked agent (agent 1 of row 0)."""
    em = (torch.rand(R, NE, generator=g) < 0.3).to(torch.uint8)
    em[:, 0] = 0
    em[0, 1] = 1
    return em


def _to(p, dtype, grad=True):
    return {k: v.detach().clone().to(dtype).requires_grad_(grad) for k, v in p.items()}


# ---- attention layer -----------------------------------------------------------------------------------------
def attn_case(bs, ne, nq, seed=1):
    g = torch.Generator().manual_seed(seed)
    p = {"in_trans.weight": _u(g, 192, 64, k=0.25), "out_trans.weight": _u(g, 64, 64, k=0.25),
         "out_trans.bias": _u(g, 64, k=0.3)}
    x = torch.randn(bs, ne, 64, generator=g)
    pre = (torch.rand(bs, nq, ne, generator=g) < 0.3).to(torch.uint8)
    post = (torch.rand(bs, nq, generator=g) < 0.2).to(torch.uint8)
    pre[0, 0, :] = 1   # a query row whose every key is pre-masked
    post[0, 0] = 0     # ... and which is not post-masked, so the NaN -> 0 path carries an upstream gradient
    post[0, 1] = 1     # a post-masked row
    pre[0, 1, :] = 0
    if bs >= 3:
        pre[2] = 1     # an item whose entities are all masked
        post[2] = 0
    return p, x, pre, post, torch.randn(bs, nq, 64, generator=g)


def attn_reference(p, x, pre, post, gy, dtype):
    pp = _to(p, dtype)
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    y = RR.attn_layer(pp, xx, pre, post, 4)
    (y * gy.to(dtype)).sum().backward()
    out = {k: v.grad for k, v in pp.items()}
    out["dx"] = xx.grad
    out["y"] = y.detach()
    return out


def _make_attn(p, device, enable=True):
    from maleague.modules.layers.attention import EntityAttentionLayer
    layer = EntityAttentionLayer(64, 64, 64, refil_args(device=str(device)))
    sd = layer.state_dict()
    sd.update({k: v.to(device) for k, v in p.items()})
    layer.load_state_dict(sd)
    return layer.enable_autograd() if enable else layer


@pytest.mark.parametrize("ne,nq", [(16, 8), (16, 16), (11, 5)])
@pytest.mark.parametrize("bs", [1, 3, 70, 257])
def test_attention_gradients(device, bs, ne, nq):
    """bs 70: 1120 / 560 rows, several weight-gradient chunk groups with a ragged last one; 257: 4112 entity rows,
    past one group of four 1024-row chunks."""
    p, x, pre, post, gy = attn_case(bs, ne, nq)
    ref = attn_reference(p, x, pre, post, gy, f64)
    r32 = attn_reference(p, x, pre, post, gy, torch.float32)
    layer, plain = _make_attn(p, device), _make_attn(p, device, enable=False)
    xd = x.to(device).requires_grad_(True)
    y = layer(xd, pre.to(device), post.to(device))
    y0 = plain(x.to(device), pre.to(device), post.to(device))
    assert y.requires_grad and not y0.requires_grad and torch.equal(y.detach(), y0)
    y.backward(gy.to(device))
    print(f"attention bs={bs} ne={ne} nq={nq}")
    _check("y (forward)", y, ref["y"], r32["y"], forward=True)
    for k, v in layer.named_parameters():
        _check(k, v.grad, ref[k], r32[k])
    _check("dx", xd.grad, ref["dx"], r32["dx"])


# ---- FlexQMixer ----------------------------------------------------------------------------------------------
def _margs(NA, NE, softmax=False, A=21, **kw):
    return refil_args(n_agents=NA, n_entities=NE, n_actions=A, softmax_mixing_weights=softmax, **kw)


def hyper_params(g, D0, prefix=""):
    return {prefix + "fc1.weight": _u(g, 64, D0, k=0.25), prefix + "fc1.bias": _u(g, 64, k=0.3),
            prefix + "attn.in_trans.weight": _u(g, 192, 64, k=0.2), prefix + "attn.out_trans.weight": _u(g, 64, 64, k=0.2),
            prefix + "attn.out_trans.bias": _u(g, 64, k=0.3), prefix + "fc2.weight": _u(g, 32, 64, k=0.25),
            prefix + "fc2.bias": _u(g, 32, k=0.3)}


def mixer_case(R, NA, NE, softmax, imagine, seed, A=21):
    g = torch.Generator().manual_seed(seed)
    D0 = ED + A
    mp = {}
    for h in HYPERS:
        mp.update(hyper_params(g, D0, h + "."))
    ent = torch.randn(R, 1, NE, D0, generator=g)
    em = _entity_mask(g, R, NA, NE).view(R, 1, NE)
    qs = torch.randn(R, 1, (2 if imagine else 1) * NA, generator=g) * 1.5
    groups = None
    if imagine:
        groupA = torch.bernoulli(torch.rand(R, 1, 1, generator=g).repeat(1, 1, NE), generator=g).to(torch.uint8)
        _, _, Wn, In = RR.imagine_masks(groupA, em, torch.zeros(R, 1, NE, NE, dtype=torch.uint8))
        groups = (Wn, In)
    g_out = torch.randn(R, 1, 1, generator=g) * (8.0 if softmax else 1.0)
    return mp, qs, ent, em, groups, g_out


def _hyper_checks(d, name, ent, em, NA, attn_mask, check_abs):
    """fc1 ReLU argument and, without softmax, the abs argument (fc2 output) of one hypernet, oracle side."""
    pre1 = F.linear(ent, d[name + ".fc1.weight"], d[name + ".fc1.bias"])
    _both_signs(name + ".fc1", pre1)
    _clear_of_kinks(name + ".fc1", pre1, ent, d[name + ".fc1.weight"], d[name + ".fc1.bias"])
    if not check_abs:
        return
    agent_mask = em[:, :NA].bool()
    if attn_mask is None:
        attn_mask = 1 - torch.bmm((1 - agent_mask.to(ent.dtype)).unsqueeze(2), (1 - em.to(ent.dtype)).unsqueeze(1))
    x2 = RR.attn_layer(d, F.relu(pre1), attn_mask.bool(), agent_mask, 4, name + ".attn.")
    w, b = d[name + ".fc2.weight"], d[name + ".fc2.bias"]
    x3 = F.linear(x2, w, b)
    live = ~agent_mask
    if name == "hyper_w_1":
        _clear_of_kinks(name + ".fc2 (abs)", x3, x2, w, b, rows=live)
    else:  # hyper_w_final: abs of the agent mean of the masked rows
        lv = live.unsqueeze(-1).to(x3.dtype)
        mean = (x3 * lv).sum(1) / NA
        margin = 8 * EPS32 * (F.linear(x2.abs(), w.abs(), b.abs()) * lv).sum(1) / NA
        assert bool((mean.abs() > margin).all()), "hyper_w_final mean within rounding error of abs' kink"


def mixer_reference(mp, qs, ent, em, groups, g_out, args, dtype, check=False):
    pp = _to(mp, dtype)
    q = qs.detach().clone().to(dtype).requires_grad_(True)
    e = ent.to(dtype)
    if check:
        d = {k: v.detach() for k, v in pp.items()}
        R, _, NE, D0 = e.shape
        e2, m2, NA = e.reshape(R, NE, D0), em.reshape(R, NE), args.n_agents
        ab = not args.softmax_mixing_weights
        for name in HYPERS:
            masks = [None] if (groups is None or name != "hyper_w_1") else [gm.reshape(R, NE, NE) for gm in groups]
            for am in masks:
                _hyper_checks(d, name, e2, m2, NA, am, ab and name in ("hyper_w_1", "hyper_w_final"))
        hn = lambda name, mode, am=None: RR.hypernet(d, name + ".", e2, m2, NA, 4, mode, am)  # noqa: E731
        w1 = hn("hyper_w_1", "matrix") if groups is None else torch.cat(
            [hn("hyper_w_1", "matrix", gm.reshape(R, NE, NE)) for gm in groups], dim=1)
        w1 = F.softmax(w1, dim=-1) if args.softmax_mixing_weights else w1.abs()
        _both_signs("ELU argument", torch.bmm(q.detach().reshape(R, 1, -1), w1) + hn("hyper_b_1", "vector").unsqueeze(1))
    out = RR.flex_qmix(pp, q, e, em, args, imagine_groups=groups)
    (out * g_out.to(dtype)).sum().backward()
    res = {k: v.grad for k, v in pp.items()}
    res["d_agent_qs"] = q.grad
    res["q_tot"] = out.detach()
    return res


def _make_mixer(mp, args, device, enable=True):
    from maleague.modules.mixers.flex_qmix import FlexQMixer
    a = copy.copy(args)
    a.device = str(device)
    mx = FlexQMixer(a)
    sd = mx.state_dict()
    sd.update({k: v.to(device) for k, v in mp.items()})
    mx.load_state_dict(sd)
    return mx.enable_autograd() if enable else mx


# seeds chosen on the CPU (kink rule of the module docstring); every other case: seed 1
MIXER_SEEDS = {(1, 8, 16, False, True): 2, (5, 8, 16, False, False): 2, (5, 8, 16, False, True): 2,
               (5, 8, 16, True, False): 2, (5, 8, 16, True, True): 2, (130, 8, 16, False, False): 5,
               (130, 8, 16, False, True): 5, (130, 8, 16, True, False): 5, (130, 8, 16, True, True): 5,
               (130, 5, 11, False, False): 5, (130, 5, 11, False, True): 5, (130, 5, 11, True, False): 5,
               (130, 5, 11, True, True): 5}


def _mixer_seed(R, NA, NE, softmax, imagine):
    return MIXER_SEEDS.get((R, NA, NE, softmax, imagine), 1)


@pytest.mark.parametrize("imagine", [False, True], ids=["plain", "imagine"])
@pytest.mark.parametrize("softmax", [False, True], ids=["abs", "softmax"])
@pytest.mark.parametrize("NA,NE", [(8, 16), (5, 11)])
@pytest.mark.parametrize("R", [1, 5, 130])
def test_flex_qmixer_gradients(device, R, NA, NE, softmax, imagine):
    args = _margs(NA, NE, softmax)
    mp, qs, ent, em, groups, g_out = mixer_case(R, NA, NE, softmax, imagine, _mixer_seed(R, NA, NE, softmax, imagine))
    ref = mixer_reference(mp, qs, ent, em, groups, g_out, args, f64, check=True)
    r32 = mixer_reference(mp, qs, ent, em, groups, g_out, args, torch.float32)
    mx, plain = _make_mixer(mp, args, device), _make_mixer(mp, args, device, enable=False)
    qd = qs.to(device).requires_grad_(True)
    gd = None if groups is None else tuple(t.to(device) for t in groups)
    out = mx(qd, (ent.to(device), em.to(device)), imagine_groups=gd)
    out0 = plain(qs.to(device), (ent.to(device), em.to(device)), imagine_groups=gd)
    assert out.shape == (R, 1, 1) and out.requires_grad and not out0.requires_grad and torch.equal(out.detach(), out0)
    out.backward(g_out.to(device))
    print(f"flex_qmix R={R} NA={NA} NE={NE} softmax={softmax} imagine={imagine}")
    _check("q_tot (forward)", out, ref["q_tot"], r32["q_tot"], forward=True)
    for k, v in mx.named_parameters():
        _check(k, v.grad, ref[k], r32[k])
    _check("d_agent_qs", qd.grad, ref["d_agent_qs"], r32["d_agent_qs"])


# ---- agent step ----------------------------------------------------------------------------------------------
def agent_params(g, D0, A):
    p = {"fc1.weight": _u(g, 64, D0, k=0.25), "fc1.bias": _u(g, 64, k=0.3),
         "attn.in_trans.weight": _u(g, 192, 64, k=0.2), "attn.out_trans.weight": _u(g, 64, 64, k=0.2),
         "attn.out_trans.bias": _u(g, 64, k=0.3), "fc2.weight": _u(g, 64, 64, k=0.25), "fc2.bias": _u(g, 64, k=0.3),
         "rnn.weight_ih": _u(g, 192, 64, k=0.25), "rnn.weight_hh": _u(g, 192, 64, k=0.25),
         "rnn.bias_ih": _u(g, 192, k=0.3), "rnn.bias_hh": _u(g, 192, k=0.3), "fc3.weight": _u(g, A, 64, k=0.25),
         "fc3.bias": _u(g, A, k=0.3)}
    return p


def agent_case(R, NA, NE, A, seed, h_zero=False):
    g = torch.Generator().manual_seed(seed)
    D0 = ED + A
    p = agent_params(g, D0, A)
    ent = torch.randn(R, 1, NE, D0, generator=g)
    om = (torch.rand(R, 1, NE, NE, generator=g) < 0.3).to(torch.uint8)
    em = _entity_mask(g, R, NA, NE).view(R, 1, NE)
    h = torch.zeros(R, NA, 64) if h_zero else torch.randn(R, NA, 64, generator=g) * 0.7
    return p, ent, om, em, h, torch.randn(R, 1, NA, A, generator=g), torch.randn(R, 1, NA, 64, generator=g)


def _agent_kink_checks(d, ent, om, em, args):
    R, ts, NE, D0 = ent.shape
    e2 = ent.reshape(R * ts, NE, D0)
    pre1 = F.linear(e2, d["fc1.weight"], d["fc1.bias"])
    _both_signs("fc1", pre1)
    _clear_of_kinks("fc1", pre1, e2, d["fc1.weight"], d["fc1.bias"])
    x2 = RR.attn_layer(d, F.relu(pre1), om.reshape(R * ts, NE, NE).bool(),
                       em.reshape(R * ts, NE)[:, :args.n_agents].bool(), 4, "attn.")
    _clear_of_kinks("fc2", F.linear(x2, d["fc2.weight"], d["fc2.bias"]), x2, d["fc2.weight"], d["fc2.bias"])


def agent_reference(p, ent, om, em, h, gq, gh, args, dtype, check=False):
    pp = _to(p, dtype)
    hh = h.detach().clone().to(dtype).requires_grad_(True)
    e = ent.to(dtype)
    if check:
        _agent_kink_checks({k: v.detach() for k, v in pp.items()}, e, om, em, args)
    q, hs = RR.entity_agent(pp, e, om, em, hh, args)
    loss = 0
    if gq is not None:
        loss = loss + (q * gq.to(dtype)).sum()
    if gh is not None:
        loss = loss + (hs * gh.to(dtype)).sum()
    loss.backward()
    out = {k: v.grad for k, v in pp.items()}
    out["d_h_in"] = hh.grad
    out["q"], out["hs"] = q.detach(), hs.detach()
    return out


def _make_agent(p, args, device, enable=True, cls=None):
    from maleague.modules.agents.entity_agent import EntityAttentionRNNAgent
    a = copy.copy(args)
    a.device = str(device)
    ag = (cls or EntityAttentionRNNAgent)(ED + args.n_actions, a)
    sd = ag.state_dict()
    sd.update({k: v.to(device) for k, v in p.items()})
    ag.load_state_dict(sd)
    return ag.enable_autograd() if enable else ag


AGENT_SEEDS = {(67, 8, 16, 21): 2}  # as MIXER_SEEDS


def _agent_seed(R, NA, NE, A):
    return AGENT_SEEDS.get((R, NA, NE, A), 1)


def _run_agent(device, R, NA, NE, A, use_q=True, use_h=True, h_zero=False):
    args = _margs(NA, NE, A=A)
    p, ent, om, em, h, gq, gh = agent_case(R, NA, NE, A, _agent_seed(R, NA, NE, A), h_zero)
    gq, gh = (gq if use_q else None), (gh if use_h else None)
    ref = agent_reference(p, ent, om, em, h, gq, gh, args, f64, check=True)
    r32 = agent_reference(p, ent, om, em, h, gq, gh, args, torch.float32)
    ag, plain = _make_agent(p, args, device), _make_agent(p, args, device, enable=False)
    if h_zero:
        hd = ag.init_hidden().unsqueeze(0).expand(R, NA, -1)
    else:
        hd = h.to(device).requires_grad_(True)
    inputs = (ent.to(device), om.to(device), em.to(device))
    q, hs = ag(inputs, hd)
    q0, hs0 = plain(inputs, hd.detach())
    assert q.requires_grad and hs.requires_grad and not q0.requires_grad and not hs0.requires_grad
    assert torch.equal(q.detach(), q0) and torch.equal(hs.detach(), hs0)
    outs, grads = [], []
    if use_q:
        outs.append(q), grads.append(gq.to(device))
    if use_h:
        outs.append(hs), grads.append(gh.to(device))
    torch.autograd.backward(outs, grads)
    print(f"entity agent R={R} NA={NA} NE={NE} A={A} q={use_q} h={use_h} h_zero={h_zero}")
    _check("q (forward)", q, ref["q"], r32["q"], forward=True)
    _check("hs (forward)", hs, ref["hs"], r32["hs"], forward=True)
    for k, v in ag.named_parameters():
        if ref[k] is None:  # fc3 when only h_out is used
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, k
            continue
        _check(k, v.grad, ref[k], r32[k])
    if not h_zero:
        _check("d_h_in", hd.grad, ref["d_h_in"], r32["d_h_in"])


@pytest.mark.parametrize("NA,NE,A", [(8, 16, 21), (5, 11, 9)])
@pytest.mark.parametrize("R", [1, 2, 3, 67])
def test_agent_step_gradients(device, R, NA, NE, A):
    _run_agent(device, R, NA, NE, A)


@pytest.mark.parametrize("NA,NE,A", [(1, 2, 7), (8, 16, 32)], ids=["K1=16", "K1=48"])
@pytest.mark.parametrize("R", [1, 2, 3])
def test_agent_step_other_input_widths(device, R, NA, NE, A):
    """The two entity input widths check_dims accepts that no other test reaches: D0 = 8 + 7 = 15 (K1 = 16; one agent
    among two entities) and D0 = 8 + 32 = 40 (K1 = 48, the widest; 32 actions fill both fc3 tiles). Forward values and
    every gradient, with the kink conditions asserted on the oracle as for the other shapes."""
    from maleague import _native
    d = _make_agent(agent_case(R, NA, NE, A, _agent_seed(R, NA, NE, A))[0], _margs(NA, NE, A=A), device).dims()
    assert (d.entity_shape + d.n_actions + 15) // 16 * 16 == (16 if A == 7 else 48)
    assert _native.load().mlg_refil_packed_agent_size(_native.byref(d)) > 0  # check_dims accepts the width
    _run_agent(device, R, NA, NE, A)


@pytest.mark.parametrize("kw", [dict(use_h=False), dict(use_q=False), dict(h_zero=True)],
                         ids=["only_q", "only_h_out", "h_in_from_init_hidden"])
def test_agent_step_partial_gradients(device, kw):
    _run_agent(device, 67, 8, 16, 21, **kw)


# ---- the reference-style REFIL loop --------------------------------------------------------------------------
LOOP_B, LOOP_T = 3, 5


def loop_batch(args, seed, B=LOOP_B, T=LOOP_T):
    """A random filled / terminated entity batch [B, T, ...] with episode 1 ending mid-way (CPU tensors)."""
    g = torch.Generator().manual_seed(seed)
    NA, NE, A = args.n_agents, args.n_entities, args.n_actions
    avail = (torch.rand(B, T, NA, A, generator=g) < 0.7).int()
    actions = torch.randint(0, A, (B, T, NA, 1), generator=g)
    avail.scatter_(3, actions, 1)  # the taken action is available
    term = torch.zeros(B, T, 1, dtype=torch.uint8)
    filled = torch.ones(B, T, 1, dtype=torch.long)
    term[1, 1] = 1
    filled[1, 3:] = 0
    term[0, T - 2] = 1
    em = (torch.rand(B, 1, NE, generator=g) < 0.3).to(torch.uint8).repeat(1, T, 1)
    em[:, :, 0] = 0
    em[0, :, 1] = 1
    om = ((torch.rand(B, T, NE, NE, generator=g) < 0.3).to(torch.uint8) | RR.entity_to_attn_mask(em)).to(torch.uint8)
    return {"entities": torch.randn(B, T, NE, ED, generator=g), "obs_mask": om, "entity_mask": em, "actions": actions,
            "avail_actions": avail, "reward": torch.randn(B, T, 1, generator=g), "terminated": term, "filled": filled,
            "actions_onehot": F.one_hot(actions.squeeze(3), A).float()}


def entity_inputs(b, args):
    """EntityMAC._build_inputs for the whole episode (entity_controller.py:11-30) on b's device: the entities with
    the previous step's action one-hot appended to the agent entities."""
    ent = b["entities"]
    bs, T, ne, _ = ent.shape
    la = torch.zeros(bs, T, ne, args.n_actions, dtype=ent.dtype, device=ent.device)
    la[:, 1:, :args.n_agents] = b["actions_onehot"][:, :-1].to(ent.dtype)
    return torch.cat([ent, la], dim=3)


def mixer_ins(b, args):
    """REFILLearner._get_mixer_ins (refil_learner.py): the same inputs and the entity mask, at t and t + 1."""
    ent = entity_inputs(b, args)
    em = b["entity_mask"]
    return (ent[:, :-1], em[:, :-1]), (ent[:, 1:], em[:, 1:])


def refil_loss(unroll, mix, b, args):
    """The loss of REFILLearnerRef.train / the reference learner (refil_learner.py:102-177) over
    `unroll(online, imagine) -> (q, groups)` and `mix(online, qs, ins, groups) -> [B, T-1, 1]`."""
    rewards, actions = b["reward"][:, :-1], b["actions"][:, :-1]
    terminated = b["terminated"][:, :-1].to(rewards.dtype)
    mask = b["filled"][:, :-1].to(rewards.dtype).clone()
    mask[:, 1:] = mask[:, 1:] * (1 - terminated[:, :-1])
    avail = b["avail_actions"]
    all_q, groups = unroll(True, True)
    all_chosen = torch.gather(all_q[:, :-1], dim=3, index=actions.repeat(3, 1, 1, 1)).squeeze(3)
    mac_out = all_q.chunk(3, dim=0)[0]
    caq, caq_w, caq_i = all_chosen.chunk(3, dim=0)
    caq_imagine = torch.cat([caq_w, caq_i], dim=2)
    ins, targ_ins = mixer_ins(b, args)
    with torch.no_grad():
        tq = unroll(False, False)[0][:, 1:].clone()
        tq[avail[:, 1:] == 0] = -9999999
        if args.double_q:
            mo = mac_out.clone().detach()
            mo[avail == 0] = -9999999
            tmax = torch.gather(tq, 3, mo[:, 1:].max(dim=3, keepdim=True)[1]).squeeze(3)
        else:
            tmax = tq.max(dim=3)[0]
        tmax = mix(False, tmax, targ_ins, None)
    chosen = mix(True, caq, ins, None)
    caq_imagine = mix(True, caq_imagine, ins, [gm[:, :-1] for gm in groups])
    targets = (rewards + args.gamma * (1 - terminated) * tmax).detach()
    mask = mask.expand_as(chosen)
    loss = (((chosen - targets) * mask) ** 2).sum() / mask.sum()
    im_loss = (((caq_imagine - targets) * mask) ** 2).sum() / mask.sum()
    return (1 - args.lmbda) * loss + args.lmbda * im_loss


def _episode_batch(b, args, device):
    from maleague.components.episode_batch import EpisodeBatch
    B, T = b["entities"].shape[:2]
    info = {"n_agents": args.n_agents, "n_actions": args.n_actions, "n_entities": args.n_entities, "entity_shape": ED,
            "episode_limit": T - 1}
    scheme, groups, pre = entity_scheme_for(info, torch)
    eb = EpisodeBatch(scheme, groups, B, T, preprocess=pre, device=device)
    for k, v in b.items():
        eb.data.transition_data[k].copy_(v)
    return eb


class _Log:
    def log_stat(self, *a):
        pass

    def info(self, *a):
        pass


def _loop_setup(device, seed=3, B=LOOP_B, T=LOOP_T):
    from maleague.controllers import EntityMAC
    args = refil_args(device=str(device))
    g = torch.Generator().manual_seed(seed)
    D0 = ED + args.n_actions
    p = agent_params(g, D0, args.n_actions)
    mp = {}
    for h in HYPERS:
        mp.update(hyper_params(g, D0, h + "."))
    b = loop_batch(args, seed, B, T)
    groupA = torch.bernoulli(torch.rand(B, 1, 1, generator=g).repeat(1, 1, args.n_entities),
                             generator=g).to(torch.uint8)
    eb = _episode_batch(b, args, device)
    mac = EntityMAC(eb.scheme, eb.groups, args)
    sd = mac.agent.state_dict()
    sd.update({k: v.to(device) for k, v in p.items()})
    mac.agent.load_state_dict(sd)
    mac.enable_autograd()
    mx = _make_mixer(mp, args, device)
    return args, b, eb, p, mp, groupA, mac, copy.deepcopy(mac), mx, copy.deepcopy(mx)


def _gpu_loss(args, eb, groupA, mac, target_mac, mx, target_mx):
    def unroll(online, imagine):
        m = mac if online else target_mac
        m.init_hidden(eb.batch_size)
        if imagine:
            return m.forward(eb, None, imagine=True, groupA=groupA.to(eb["entities"].device))
        return m.forward(eb, None), None

    def mix(online, qs, ins, groups):
        return (mx if online else target_mx)(qs, ins, imagine_groups=groups)

    keys = ("reward", "actions", "terminated", "filled", "avail_actions", "entities", "entity_mask", "actions_onehot")
    return refil_loss(unroll, mix, {k: eb[k] for k in keys}, args)


def _ref_loss_fn(args, bb, pp, mpp, groupA):
    """The oracle's side of refil_loss over parameters pp / mpp and a batch bb of one dtype and device."""
    NA = args.n_agents

    def unroll(online, imagine):
        ent, em, om = entity_inputs(bb, args), bb["entity_mask"], bb["obs_mask"]
        h0 = torch.zeros(ent.shape[0], NA, args.rnn_hidden_dim, dtype=ent.dtype, device=ent.device)
        if not imagine:
            return RR.entity_agent(pp, ent, om, em, h0, args)[0], None
        within, interact, Wn, In = RR.imagine_masks(groupA, em, om)
        T = ent.shape[1]
        q, _ = RR.entity_agent(pp, ent.repeat(3, 1, 1, 1), torch.cat([om.to(torch.uint8), within, interact], dim=0),
                               em.repeat(3, 1, 1), h0.repeat(3, 1, 1), args)
        return q, (Wn.repeat(1, T, 1, 1), In.repeat(1, T, 1, 1))

    def mix(online, qs, ins, groups):
        return RR.flex_qmix(mpp, qs, ins[0], ins[1], args, imagine_groups=groups)

    return refil_loss(unroll, mix, bb, args)


def _ref_loss(args, b, p, mp, groupA, dtype):
    pp, mpp = _to(p, dtype), _to(mp, dtype)
    bb = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in b.items()}
    assert torch.equal(entity_inputs(bb, args), RR.build_entity_inputs(bb, args.n_agents, args.n_actions)[0])
    loss = _ref_loss_fn(args, bb, pp, mpp, groupA)
    loss.backward()
    return loss.detach(), pp, mpp


def test_reference_style_refil_loop(device):
    """EntityMAC.forward(batch, None, imagine=True, groupA), gather, FlexQMixer plain and with groups, the
    lambda-mixed TD loss, loss.backward(): the loss and every agent and mixer gradient equal autograd over the oracle."""
    args, b, eb, p, mp, groupA, mac, target_mac, mx, target_mx = _loop_setup(device)
    loss = _gpu_loss(args, eb, groupA, mac, target_mac, mx, target_mx)
    loss.backward()
    ref_loss, pp, mpp = _ref_loss(args, b, p, mp, groupA, f64)
    loss32, pp32, mpp32 = _ref_loss(args, b, p, mp, groupA, torch.float32)
    print("REFIL loop")
    _check("loss", loss, ref_loss, loss32)
    for k, v in mac.agent.named_parameters():
        _check(k, v.grad, pp[k].grad, pp32[k].grad)
    for k, v in mx.named_parameters():
        _check(k, v.grad, mpp[k].grad, mpp32[k].grad)


def test_gradients_match_fused_learner(device):
    """Two independent HIP paths: the autograd gradients of the reference-style loss, clipped, against the clipped
    gradients mlg_refil_train leaves in REFILLearner._grads (same batch, weights and groupA, targets equal to online)."""
    from maleague.controllers import EntityMAC
    from maleague.learners import REFILLearner
    args, b, eb, p, mp, groupA, mac, target_mac, mx, target_mx = _loop_setup(device)
    _gpu_loss(args, eb, groupA, mac, target_mac, mx, target_mx).backward()
    params = list(mac.parameters()) + list(mx.parameters())
    torch.nn.utils.clip_grad_norm_(params, args.grad_norm_clip)
    mac2 = EntityMAC(eb.scheme, eb.groups, args)
    mac2.agent.load_state_dict(mac.agent.state_dict())
    learner = REFILLearner(mac2, eb.scheme, _Log(), args, name="home")
    learner.mixer.load_state_dict(mx.state_dict())
    learner.target_mixer.load_state_dict(mx.state_dict())
    learner.target_mac.load_state(mac2)
    learner.build_optimizer()
    learner.train(eb, 0, 0, groupA=groupA.to(device))
    print("autograd vs fused REFIL learner")
    for (q, off, k), mine in zip(learner._flat.views, params):
        _check(f"param {off}", mine.grad, learner._grads[off:off + k].view_as(q).cpu().to(f64))


# ---- determinism, empty batches, optimizer steps, errors, opcheck, compile -----------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_cases():
    return (attn_case(257, 16, 16), mixer_case(130, 8, 16, False, True, 1), agent_case(67, 8, 16, 21, 1))


def _attn_op_args(device, bs=257, requires_grad=False):
    p, x, pre, post, gy = attn_case(bs, 16, 16) if bs != 257 else _cpu_cases()[0]
    ws = [p[k].to(device).requires_grad_(requires_grad) for k in ("in_trans.weight", "out_trans.weight",
                                                                   "out_trans.bias")]
    return ws, [t.to(device) for t in (x, pre, post, gy)]


def _mixer_op_args(device, R=130, requires_grad=False):
    from maleague.ops import struct_fields
    mp, qs, ent, em, groups, g_out = mixer_case(R, 8, 16, False, True, 1) if R != 130 else _cpu_cases()[1]
    args = _margs(8, 16)
    mx = _make_mixer(mp, args, device)
    d = mx._dims()
    flat = torch.cat([q.detach().reshape(-1) for q in mx.parameters()])
    from maleague import _native
    packed = torch.empty(_native.load().mlg_refil_packed_mixer_size(_native.byref(d)), device=device)
    _native.call("mlg_refil_pack_mixer", _native.byref(d), _native.ptr(flat), _native.ptr(packed), _native.stream_ptr())
    params = [q.detach().clone().requires_grad_(requires_grad) for q in mx.parameters()]
    data = [qs.reshape(R, -1).to(device), ent.reshape(R, 16, -1).to(device), em.reshape(R, 16).to(device),
            groups[0].reshape(R, 16, 16).to(device), groups[1].reshape(R, 16, 16).to(device),
            g_out.reshape(R).to(device)]
    return params, packed, data, struct_fields(d)


def _agent_op_args(device, R=67, requires_grad=False):
    from maleague.ops import struct_fields
    p, ent, om, em, h, gq, gh = agent_case(R, 8, 16, 21, 1) if R != 67 else _cpu_cases()[2]
    ag = _make_agent(p, _margs(8, 16), device)
    params = [v.detach().clone().requires_grad_(requires_grad) for v in ag.parameters()]
    data = [ent.reshape(R, 16, -1).to(device), om.reshape(R, 16, 16).to(device), em.reshape(R, 16).to(device),
            h.to(device), gq.reshape(R, 8, 21).to(device), gh.reshape(R, 8, 64).to(device)]
    return ag, params, data, struct_fields(ag.dims())


def test_backward_is_deterministic(device):
    ops = torch.ops.maleague
    ws, (x, pre, post, gy) = _attn_op_args(device)
    a, b = (ops.refil_attention_backward(*ws, x, pre, post, gy, 4) for _ in range(2))
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    params, packed, (qs, ent, em, wm, im, g_out), dims = _mixer_op_args(device)
    a, b = (ops.flex_qmix_backward(params, packed, qs, ent, em, wm, im, g_out, 0, dims) for _ in range(2))
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    ag, params, (ent, om, em, h, gq, gh), dims = _agent_op_args(device)
    a, b = (ops.entity_agent_backward(params, ag.packed(), ent, om, em, h, gq, gh, dims) for _ in range(2))
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_empty_batch_zeroes_parameter_gradients(device):
    ops = torch.ops.maleague
    ws, (x, pre, post, gy) = _attn_op_args(device, bs=3)
    dx, dflat = ops.refil_attention_backward(*ws, x[:0], pre[:0], post[:0], gy[:0], 4)
    assert dx.shape == (0, 16, 64) and dflat.numel() == 192 * 64 + 64 * 64 + 64 and float(dflat.abs().max()) == 0.0
    params, packed, (qs, ent, em, wm, im, g_out), dims = _mixer_op_args(device, R=5)
    dq, mflat = ops.flex_qmix_backward(params, packed, qs[:0], ent[:0], em[:0], wm[:0], im[:0], g_out[:0], 0, dims)
    assert dq.shape == (0, 16) and float(mflat.abs().max()) == 0.0
    ag, params, (ent, om, em, h, gq, gh), dims = _agent_op_args(device, R=3)
    dh, aflat = ops.entity_agent_backward(params, ag.packed(), ent[:0], om[:0], em[:0], h[:0], gq[:0], gh[:0], dims)
    assert dh.shape == (0, 8, 64) and float(aflat.abs().max()) == 0.0


def test_no_grad_ignores_the_switch(device):
    p, ent, om, em, h, _, _ = agent_case(3, 8, 16, 21, 1)
    ag = _make_agent(p, _margs(8, 16), device)
    with torch.no_grad():
        q, hs = ag((ent.to(device), om.to(device), em.to(device)), h.to(device))
    assert not q.requires_grad and not hs.requires_grad


@pytest.mark.parametrize("flat", [False, True], ids=["module_params", "flat_param_views"])
def test_torch_optimizer_step_reaches_the_kernels(device, flat):
    """Parameters stepped by torch.optim.RMSprop (also as the learner's FlatParams views): the next forward differs
    and equals a fresh module loaded with the stepped state dict (the packed blocks follow the parameters)."""
    from maleague.learners.q_learner import FlatParams
    args = _margs(8, 16)
    R = 6
    p, ent, om, em, h, gq, _ = agent_case(R, 8, 16, 21, 4)
    mp = mixer_case(R, 8, 16, False, False, 4)[0]
    ag, mx = _make_agent(p, args, device), _make_mixer(mp, args, device)
    params = list(ag.parameters()) + list(mx.parameters())
    if flat:
        keep = FlatParams(params, device)  # noqa: F841
        ag.mark_dirty()
    inputs = (ent.to(device), om.to(device), em.to(device))
    h = h.to(device)

    def forward(a, m):
        q, _ = a(inputs, h)
        return q, m(q[..., 0], (inputs[0], inputs[2]))

    opt = torch.optim.RMSprop(params, lr=1e-2)
    q0, y0 = forward(ag, mx)
    (y0.sum() + (q0 * gq.to(device)).sum()).backward()
    assert all(t.grad is not None for t in params)
    opt.step()
    q1, y1 = forward(ag, mx)
    assert not torch.equal(q0, q1) and not torch.equal(y0, y1)
    fresh_a = _make_agent({k: v.detach() for k, v in ag.state_dict().items()}, args, device, enable=False)
    fresh_m = _make_mixer({k: v.detach() for k, v in mx.state_dict().items()}, args, device, enable=False)
    q2, y2 = forward(fresh_a, fresh_m)
    assert torch.equal(q1.detach(), q2) and torch.equal(y1.detach(), y2)


def test_documented_errors(device):
    from maleague._native import NativeError
    args = _margs(8, 16)
    R = 4
    p, ent, om, em, h, _, _ = agent_case(R, 8, 16, 21, 2)
    mp, qs, ment, mem, _, _ = mixer_case(R, 8, 16, False, False, 2)
    ag, mx = _make_agent(p, args, device), _make_mixer(mp, args, device)
    inputs = (ent.to(device), om.to(device), em.to(device))
    with pytest.raises(NativeError, match="entity_agent_forward: gradients with respect to the entities"):
        ag((inputs[0].clone().requires_grad_(), inputs[1], inputs[2]), h.to(device))
    with pytest.raises(NativeError, match="flex_qmix_forward: gradients with respect to the entities"):
        mx(qs.to(device), (ment.to(device).requires_grad_(), mem.to(device)))
    q, _ = ag(inputs, h.to(device))
    (g,) = torch.autograd.grad(q.sum(), ag.fc1.weight, create_graph=True)
    with pytest.raises(RuntimeError, match="entity_agent_backward"):
        g.sum().backward()
    y = mx(qs.to(device), (ment.to(device), mem.to(device)))
    (g,) = torch.autograd.grad(y.sum(), mx.V.fc2.bias, create_graph=True)
    with pytest.raises(RuntimeError, match="flex_qmix_backward"):
        g.sum().backward()
    ap, x, pre, post, _ = attn_case(R, 16, 8)
    layer = _make_attn(ap, device)
    y = layer(x.to(device), pre.to(device), post.to(device))
    (g,) = torch.autograd.grad(y.sum(), layer.out_trans.bias, create_graph=True)
    with pytest.raises(RuntimeError, match="refil_attention_backward"):
        g.sum().backward()


def test_opcheck(device):
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    ops = torch.ops.maleague
    ws, (x, pre, post, _) = _attn_op_args(device, bs=3, requires_grad=True)
    torch.library.opcheck(ops.refil_attention.default, (*ws, x, pre, post, 4), test_utils=utils)
    params, packed, (qs, ent, em, wm, im, _), dims = _mixer_op_args(device, R=5, requires_grad=True)
    torch.library.opcheck(ops.flex_qmix_forward.default, (params, packed, qs, ent, em, wm, im, 0, dims),
                          test_utils=utils)
    torch.library.opcheck(ops.flex_qmix_forward.default, (params, packed, qs[:, :8].contiguous(), ent, em, None, None,
                                                          1, dims), test_utils=utils)
    ag, params, (ent, om, em, h, _, _), dims = _agent_op_args(device, R=3, requires_grad=True)
    torch.library.opcheck(ops.entity_agent_forward.default, (params, ag.packed(), ent, om, em, h, dims),
                          test_utils=utils)


def test_compiled_loss_gradients_match_eager(device):
    """A scalar loss of entity_agent_forward under torch.compile(backend="aot_eager", fullgraph=True): AOT autograd
    traces the backward through the fake implementations; the parameter gradients equal eager's bit for bit."""
    ag, params, (ent, om, em, h, gq, gh), dims = _agent_op_args(device, R=3, requires_grad=True)
    packed = ag.packed()

    def loss_fn(ps, hh):
        q, hn = torch.ops.maleague.entity_agent_forward(ps, packed, ent, om, em, hh, dims)
        return (q * gq).sum() + (hn * gh).sum()

    def grads(fn):
        for t in params:
            t.grad = None
        loss = fn(params, h)
        loss.backward()
        return loss.detach(), [t.grad.clone() for t in params]

    l0, g0 = grads(loss_fn)
    l1, g1 = grads(torch.compile(loss_fn, backend="aot_eager", fullgraph=True))
    assert torch.allclose(l0, l1, rtol=1e-6, atol=0)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
