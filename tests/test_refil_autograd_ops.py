"""Autograd of the REFIL ops (EntityAttentionLayer, FlexQMixer, EntityAttentionRNNAgent step), the parts that need
no GPU: the six new C entry points are declared, their host-only workspace queries answer (and reject bad dims with a
message), the new ops have fake implementations with the documented shapes, autograd is registered on the three
differentiable ops (checked under FakeTensorMode), entities that require grad are refused, the ops raise on host
tensors like every product path, and the modules' opt-in switch behaves like the QMIX side's."""
import pytest
import torch

from helpers import refil_args
from test_native_abi import declared_symbols

NA, NE, ED, A = 8, 16, 8, 21
D0 = ED + A
DIMS = [NA, NE, ED, A, 1, 64, 4, 64]  # MlgRefilDims: ..., entity_last_action, attn_embed_dim, attn_n_heads, rnn_hidden_dim
NEW = ["mlg_refil_attention_backward", "mlg_refil_attention_backward_workspace_floats", "mlg_refil_mixer_backward",
       "mlg_refil_mixer_backward_workspace_floats", "mlg_refil_agent_backward",
       "mlg_refil_agent_backward_workspace_floats"]
ROWS = (1, 130, 4112)


def _attn_params(requires_grad=False):
    return [torch.empty(*s, requires_grad=requires_grad) for s in ((192, 64), (64, 64), (64,))]


def _hyper_shapes():
    return [(64, D0), (64,), (192, 64), (64, 64), (64,), (32, 64), (32,)]


def _mixer_params(requires_grad=False):
    return [torch.empty(*s, requires_grad=requires_grad) for _ in range(4) for s in _hyper_shapes()]


def _agent_params(requires_grad=False):
    shapes = [(64, D0), (64,), (192, 64), (64, 64), (64,), (64, 64), (64,), (192, 64), (192, 64), (192,), (192,),
              (A, 64), (A,)]
    return [torch.empty(*s, requires_grad=requires_grad) for s in shapes]


def _u8(*s):
    return torch.empty(*s, dtype=torch.uint8)


def test_new_entry_points_declared():
    from maleague import _native
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s
        assert s in _native.SIGNATURES, s


def _dims(**kw):
    from maleague import _native
    d = dict(zip(["n_agents", "n_entities", "entity_shape", "n_actions", "entity_last_action", "attn_embed_dim",
                  "attn_n_heads", "rnn_hidden_dim"], DIMS))
    d.update(kw)
    return _native.MlgRefilDims(**d)


def test_attention_backward_workspace_floats():
    from maleague import _native
    lib = _native.load()
    q = lib.mlg_refil_attention_backward_workspace_floats
    sizes = [q(bs, 16, 8, 4) for bs in ROWS]
    assert 0 < sizes[0] < sizes[1] < sizes[2], sizes
    assert sizes[2] >= 4112 * (16 * 192 + 2 * 8 * 64)  # dqkv rows, o and dout rows
    assert q(4, 17, 8, 4) == -1 and b"n_entities=17" in lib.mlg_last_error()
    assert q(4, 16, 8, 2) == -1 and b"attn_n_heads=2" in lib.mlg_last_error()


@pytest.mark.parametrize("imagine", [0, 1])
def test_mixer_backward_workspace_floats(imagine):
    from maleague import _native
    lib = _native.load()
    q = lib.mlg_refil_mixer_backward_workspace_floats
    sizes = [q(_native.byref(_dims()), R, imagine) for R in ROWS]
    assert 0 < sizes[0] < sizes[1] < sizes[2], sizes
    per_hyper = NE * (192 + 64) + NA * (64 + 32)  # dqkv, dx1; dout, dx3
    assert sizes[2] >= 4112 * (4 * per_hyper + imagine * NA * (64 + 32) + 5 * 8 * 32)
    assert q(_native.byref(_dims()), 16, 1) > q(_native.byref(_dims()), 16, 0)
    assert q(_native.byref(_dims(n_entities=17)), 16, imagine) == -1 and b"n_entities=17" in lib.mlg_last_error()
    assert q(_native.byref(_dims(attn_n_heads=2)), 16, imagine) == -1 and b"heads 2" in lib.mlg_last_error()
    assert q(_native.byref(_dims()), -1, imagine) == -1 and b"R=-1" in lib.mlg_last_error()


def test_agent_backward_workspace_floats():
    from maleague import _native
    lib = _native.load()
    q = lib.mlg_refil_agent_backward_workspace_floats
    sizes = [q(_native.byref(_dims()), R) for R in ROWS]
    assert 0 < sizes[0] < sizes[1] < sizes[2], sizes
    assert sizes[2] >= 4112 * (NE * (192 + 64) + NA * (2 * 64 + 2 * 192 + A))  # the row deltas alone
    assert q(_native.byref(_dims(n_entities=17)), 16) == -1 and b"n_entities=17" in lib.mlg_last_error()
    assert q(_native.byref(_dims(attn_n_heads=2)), 16) == -1 and b"attn_n_heads=2" in lib.mlg_last_error()
    assert q(_native.byref(_dims()), -1) == -1 and b"R=-1" in lib.mlg_last_error()


def test_new_ops_fake_shapes():
    import maleague  # noqa: F401  (registers the ops)
    from torch._subclasses.fake_tensor import FakeTensorMode
    from maleague.ops import OPS
    for name in ("refil_attention_backward", "flex_qmix_forward", "flex_qmix_backward", "entity_agent_forward",
                 "entity_agent_backward"):
        assert name in OPS and hasattr(torch.ops.maleague, name), name
    R, ops = 40, torch.ops.maleague
    with FakeTensorMode():
        ap = _attn_params()
        dx, dflat = ops.refil_attention_backward(*ap, torch.empty(R, 11, 64), _u8(R, 5, 11), _u8(R, 5),
                                                 torch.empty(R, 5, 64), 4)
        assert dx.shape == (R, 11, 64) and dflat.shape == (192 * 64 + 64 * 64 + 64,)
        mp = _mixer_params()
        ent, em = torch.empty(R, NE, D0), _u8(R, NE)
        for nq, masks in ((NA, (None, None)), (2 * NA, (_u8(R, NE, NE), _u8(R, NE, NE)))):
            out = ops.flex_qmix_forward(mp, torch.empty(10), torch.empty(R, nq), ent, em, *masks, 0, DIMS)
            assert out.shape == (R,)
            dq, mflat = ops.flex_qmix_backward(mp, torch.empty(10), torch.empty(R, nq), ent, em, *masks,
                                               torch.empty(R), 1, DIMS)
            assert dq.shape == (R, nq) and mflat.shape == (sum(p.numel() for p in mp),)
        ps = _agent_params()
        q, h = ops.entity_agent_forward(ps, torch.empty(10), ent, _u8(R, NE, NE), em, torch.empty(R, NA, 64), DIMS)
        assert q.shape == (R, NA, A) and h.shape == (R, NA, 64)
        dh, aflat = ops.entity_agent_backward(ps, torch.empty(10), ent, _u8(R, NE, NE), em, torch.empty(R, NA, 64),
                                              torch.empty(R, NA, A), None, DIMS)
        assert dh.shape == (R, NA, 64) and aflat.shape == (sum(p.numel() for p in ps),)


def test_autograd_registered_on_differentiable_ops():
    import maleague  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    R, ops = 24, torch.ops.maleague
    with FakeTensorMode():
        ent, em, om = torch.empty(R, NE, D0), _u8(R, NE), _u8(R, NE, NE)
        # attention: parameters or x
        for pg, xg in ((True, False), (False, True), (False, False)):
            ap = _attn_params(pg)
            x = torch.empty(R, 16, 64, requires_grad=xg)
            y = ops.refil_attention(*ap, x, _u8(R, 8, 16), _u8(R, 8), 4)
            assert y.shape == (R, 8, 64) and y.requires_grad == (pg or xg)
        ap, x = _attn_params(True), torch.empty(R, 16, 64, requires_grad=True)
        y = ops.refil_attention(*ap, x, _u8(R, 8, 16), _u8(R, 8), 4)
        grads = torch.autograd.grad(y.sum(), [x] + ap)
        assert [g.shape for g in grads] == [x.shape] + [p.shape for p in ap]
        # mixer: parameters or agent_qs
        for pg, qg in ((True, False), (False, True), (False, False)):
            out = ops.flex_qmix_forward(_mixer_params(pg), torch.empty(10), torch.empty(R, NA, requires_grad=qg), ent,
                                        em, None, None, 0, DIMS)
            assert out.requires_grad == (pg or qg)
        for nq, masks in ((NA, (None, None)), (2 * NA, (_u8(R, NE, NE), _u8(R, NE, NE)))):
            mp, qs = _mixer_params(True), torch.empty(R, nq, requires_grad=True)
            out = ops.flex_qmix_forward(mp, torch.empty(10), qs, ent, em, *masks, 1, DIMS)
            grads = torch.autograd.grad(out.sum(), [qs] + mp)
            assert [g.shape for g in grads] == [qs.shape] + [p.shape for p in mp]
        # agent step: parameters or h_in
        for pg, hg in ((True, False), (False, True), (False, False)):
            q, h = ops.entity_agent_forward(_agent_params(pg), torch.empty(10), ent, om, em,
                                            torch.empty(R, NA, 64, requires_grad=hg), DIMS)
            assert q.requires_grad == (pg or hg) and h.requires_grad == (pg or hg)
        ps, h0 = _agent_params(True), torch.empty(R, NA, 64, requires_grad=True)
        q, h = ops.entity_agent_forward(ps, torch.empty(10), ent, om, em, h0, DIMS)
        grads = torch.autograd.grad(q.sum(), [h0] + ps)  # only q used: h_out's gradient stays None
        assert [g.shape for g in grads] == [h0.shape] + [p.shape for p in ps]


def test_entity_gradients_refused():
    import maleague  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    from maleague._native import NativeError
    R, ops = 8, torch.ops.maleague
    with FakeTensorMode():
        ent = torch.empty(R, NE, D0, requires_grad=True)
        with pytest.raises(NativeError, match="flex_qmix_forward: gradients with respect to the entities"):
            ops.flex_qmix_forward(_mixer_params(True), torch.empty(10), torch.empty(R, NA), ent, _u8(R, NE), None,
                                  None, 0, DIMS)
        with pytest.raises(NativeError, match="entity_agent_forward: gradients with respect to the entities"):
            ops.entity_agent_forward(_agent_params(True), torch.empty(10), ent, _u8(R, NE, NE), _u8(R, NE),
                                     torch.empty(R, NA, 64), DIMS)


def test_new_ops_refuse_host_tensors():
    import maleague  # noqa: F401
    from maleague._native import NativeError
    R, ops = 4, torch.ops.maleague
    z8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    ent, em, om = torch.zeros(R, NE, D0), z8(R, NE), z8(R, NE, NE)
    with pytest.raises((NativeError, RuntimeError)):
        ops.refil_attention_backward(*[torch.zeros_like(p) for p in _attn_params()], torch.zeros(R, 16, 64),
                                     z8(R, 8, 16), z8(R, 8), torch.zeros(R, 8, 64), 4)
    mp = [torch.zeros_like(p) for p in _mixer_params()]
    with pytest.raises((NativeError, RuntimeError)):
        ops.flex_qmix_forward(mp, torch.zeros(10), torch.zeros(R, NA), ent, em, None, None, 0, DIMS)
    with pytest.raises((NativeError, RuntimeError)):
        ops.flex_qmix_backward(mp, torch.zeros(10), torch.zeros(R, NA), ent, em, None, None, torch.zeros(R), 0, DIMS)
    ps = [torch.zeros_like(p) for p in _agent_params()]
    with pytest.raises((NativeError, RuntimeError)):
        ops.entity_agent_forward(ps, torch.zeros(10), ent, om, em, torch.zeros(R, NA, 64), DIMS)
    with pytest.raises((NativeError, RuntimeError)):
        ops.entity_agent_backward(ps, torch.zeros(10), ent, om, em, torch.zeros(R, NA, 64), torch.zeros(R, NA, A),
                                  torch.zeros(R, NA, 64), DIMS)


def test_opt_in_switch_defaults_off_and_follows_args():
    from maleague.modules.agents.entity_agent import EntityAttentionRNNAgent, ImagineEntityAttentionRNNAgent
    from maleague.modules.layers.attention import EntityAttentionLayer
    from maleague.modules.mixers.flex_qmix import FlexQMixer
    makers = ((EntityAttentionLayer, lambda a: EntityAttentionLayer(64, 64, 64, a)), (FlexQMixer, FlexQMixer),
              (EntityAttentionRNNAgent, lambda a: EntityAttentionRNNAgent(D0, a)),
              (ImagineEntityAttentionRNNAgent, lambda a: ImagineEntityAttentionRNNAgent(D0, a)))
    for cls, make in makers:
        off = make(refil_args(device="cpu"))
        assert off._autograd is False, cls
        assert off.enable_autograd() is off and off._autograd is True
        assert off.enable_autograd(False)._autograd is False
        on = make(refil_args(device="cpu", native_autograd=True))
        assert on._autograd is True, cls
        x = torch.zeros(2, NA, 64)
        assert on.wants_grad(x) and not on.enable_autograd(False).wants_grad(x)
        with torch.no_grad():
            assert not on.enable_autograd().wants_grad(x)
        for p in on.parameters():
            p.requires_grad_(False)
        assert not on.wants_grad(x) and on.wants_grad(x.clone().requires_grad_())


def test_entity_mac_forwards_the_switch():
    from helpers import entity_scheme_for
    from maleague.controllers.entity_controller import EntityMAC
    info = {"n_entities": NE, "entity_shape": ED, "n_actions": A, "n_agents": NA}
    scheme, groups, _ = entity_scheme_for(info, torch)
    scheme["actions_onehot"] = {"vshape": (A,), "group": "agents"}
    mac = EntityMAC(scheme, groups, refil_args(device="cpu"))
    assert mac.agent._autograd is False
    assert mac.enable_autograd() is mac and mac.agent._autograd is True
    assert mac.enable_autograd(False).agent._autograd is False
