"""Autograd of the agent and mixer ops, the parts that need no GPU: the C ABI's new entry points are declared, their
host-only workspace queries answer (and reject bad dims with a message), the new ops have fake implementations with
the documented shapes, autograd is registered on the differentiable ops (outputs of parameters that require grad
require grad under FakeTensorMode), and the ops raise on host tensors like every product path."""
import pytest
import torch

from test_native_abi import declared_symbols

DIMS = [80, 15, 5, 64, 100, 1, 1]  # 5v5: d_obs, n_actions, n_agents, hidden, d_in, obs_last_action, obs_agent_id
N, S, E, HE = 5, 60, 32, 64
NEW = ["mlg_agent_backward", "mlg_agent_backward_workspace_floats", "mlg_qmix_backward",
       "mlg_qmix_backward_workspace_floats"]


def _agent_params(requires_grad=False, H=64, A=15, d_in=100):
    shapes = [(H, d_in), (H,), (3 * H, H), (3 * H, H), (3 * H,), (3 * H,), (A, H), (A,)]
    return [torch.empty(*s, requires_grad=requires_grad) for s in shapes]


def _mixer_params(layers, requires_grad=False):
    if layers == 2:
        shapes = [(HE, S), (HE,), (N * E, HE), (N * E,), (HE, S), (HE,), (E, HE), (E,)]
    else:
        shapes = [(N * E, S), (N * E,), (0,), (0,), (E, S), (E,), (0,), (0,)]
    shapes += [(E, S), (E,), (E, S), (E,), (1, E), (1,)]
    return [torch.empty(*s, requires_grad=requires_grad and s != (0,)) for s in shapes]


def test_new_entry_points_declared():
    from maleague import _native
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s
        assert s in _native.SIGNATURES, s


def test_agent_backward_workspace_floats():
    from maleague import _native
    lib = _native.load()
    d = _native.MlgAgentDims(*DIMS)
    sizes = [lib.mlg_agent_backward_workspace_floats(_native.byref(d), R) for R in (1, 160, 20480)]
    assert sizes[0] > 0 and sizes[0] < sizes[1] < sizes[2], sizes
    assert sizes[2] >= 20480 * (3 * 64 + 2 * 3 * 64 + 15)  # the row deltas alone
    bad = _native.MlgAgentDims(80, 15, 5, 48, 100, 1, 1)
    assert lib.mlg_agent_backward_workspace_floats(_native.byref(bad), 16) == -1
    assert b"48" in lib.mlg_last_error()


@pytest.mark.parametrize("layers", [1, 2])
def test_qmix_backward_workspace_floats(layers):
    from maleague import _native
    lib = _native.load()
    p = _native.MlgQMixParams(*([None] * 14), N, S, E, HE if layers == 2 else 0, layers)
    sizes = [lib.mlg_qmix_backward_workspace_floats(_native.byref(p), R) for R in (1, 129, 3200)]
    assert sizes[0] > 0 and sizes[0] < sizes[1] < sizes[2], sizes
    bad = _native.MlgQMixParams(*([None] * 14), N, S, E, HE, 3)
    assert lib.mlg_qmix_backward_workspace_floats(_native.byref(bad), 16) == -1
    assert b"hypernet_layers" in lib.mlg_last_error()


def test_new_ops_fake_shapes():
    import maleague  # noqa: F401  (registers the ops)
    from torch._subclasses.fake_tensor import FakeTensorMode
    from maleague.ops import OPS
    for name in ("drqn_forward", "drqn_backward", "qmix_backward"):
        assert name in OPS and hasattr(torch.ops.maleague, name), name
    R = 40
    with FakeTensorMode():
        ps = _agent_params()
        q, h = torch.ops.maleague.drqn_forward(ps, torch.empty(10), torch.empty(R, 100), torch.empty(R, 64), DIMS)
        assert q.shape == (R, 15) and h.shape == (R, 64)
        dx, dh, dflat = torch.ops.maleague.drqn_backward(ps, torch.empty(10), torch.empty(R, 100), torch.empty(R, 64),
                                                         torch.empty(R, 15), None, DIMS)
        assert dx.shape == (R, 100) and dh.shape == (R, 64)
        assert dflat.shape == (sum(p.numel() for p in ps),)
        for layers in (1, 2):
            mp = _mixer_params(layers)
            dq, mflat = torch.ops.maleague.qmix_backward(mp, torch.empty(R, N), torch.empty(R, S), torch.empty(R),
                                                         [N, S, E, HE if layers == 2 else 0, layers])
            assert dq.shape == (R, N) and mflat.shape == (sum(p.numel() for p in mp),)


def test_autograd_registered_on_differentiable_ops():
    import maleague  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    R = 24
    with FakeTensorMode():
        q, h = torch.ops.maleague.drqn_forward(_agent_params(True), torch.empty(10), torch.empty(R, 100),
                                               torch.empty(R, 64), DIMS)
        assert q.requires_grad and h.requires_grad
        q, h = torch.ops.maleague.drqn_forward(_agent_params(False), torch.empty(10), torch.empty(R, 100),
                                               torch.empty(R, 64), DIMS)
        assert not q.requires_grad and not h.requires_grad
        for layers in (1, 2):
            dims = [N, S, E, HE if layers == 2 else 0, layers]
            out = torch.ops.maleague.qmix_forward(_mixer_params(layers, True), torch.empty(R, N), torch.empty(R, S),
                                                  dims)
            assert out.shape == (R,) and out.requires_grad
            # the gradient formula runs on fake tensors too and hands every live parameter its shape back
            mp = _mixer_params(layers, True)
            qs = torch.empty(R, N, requires_grad=True)
            out = torch.ops.maleague.qmix_forward(mp, qs, torch.empty(R, S), dims)
            grads = torch.autograd.grad(out.sum(), [qs] + [p for p in mp if p.numel()])
            assert [g.shape for g in grads] == [qs.shape] + [p.shape for p in mp if p.numel()]
        ps = _agent_params(True)
        x = torch.empty(R, 100, requires_grad=True)
        q, h = torch.ops.maleague.drqn_forward(ps, torch.empty(10), x, torch.empty(R, 64), DIMS)
        grads = torch.autograd.grad(q.sum(), [x] + ps)  # only q used: h_out's gradient stays None
        assert [g.shape for g in grads] == [x.shape] + [p.shape for p in ps]


def test_state_gradients_refused():
    import maleague  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    from maleague._native import NativeError
    with FakeTensorMode():
        with pytest.raises(NativeError, match="states are not implemented"):
            torch.ops.maleague.qmix_forward(_mixer_params(2, True), torch.empty(8, N),
                                            torch.empty(8, S, requires_grad=True), [N, S, E, HE, 2])


def test_new_ops_refuse_host_tensors():
    import maleague  # noqa: F401
    from maleague._native import NativeError
    R = 4
    ps = [torch.zeros_like(p) for p in _agent_params()]
    with pytest.raises((NativeError, RuntimeError)):
        torch.ops.maleague.drqn_forward(ps, torch.zeros(10), torch.zeros(R, 100), torch.zeros(R, 64), DIMS)
    with pytest.raises((NativeError, RuntimeError)):
        torch.ops.maleague.drqn_backward(ps, torch.zeros(10), torch.zeros(R, 100), torch.zeros(R, 64),
                                         torch.zeros(R, 15), torch.zeros(R, 64), DIMS)
    with pytest.raises((NativeError, RuntimeError)):
        torch.ops.maleague.qmix_backward([torch.zeros_like(p) for p in _mixer_params(2)], torch.zeros(R, N),
                                         torch.zeros(R, S), torch.zeros(R), [N, S, E, HE, 2])


def test_opt_in_switch_defaults_off_and_follows_args():
    from helpers import qmix_args
    from maleague.modules.agents.drqn_agent import DRQNAgentNetwork
    from maleague.modules.mixers import QMixer
    for cls, make in ((DRQNAgentNetwork, lambda a: DRQNAgentNetwork(100, a)), (QMixer, QMixer)):
        off = make(qmix_args(device="cpu"))
        assert off._autograd is False, cls
        assert off.enable_autograd() is off and off._autograd is True
        assert off.enable_autograd(False)._autograd is False
        assert make(qmix_args(device="cpu", native_autograd=True))._autograd is True, cls
    ag = DRQNAgentNetwork(100, qmix_args(device="cpu", native_autograd=True))
    x = torch.zeros(2, 100)
    assert ag.wants_grad(x) and not ag.enable_autograd(False).wants_grad(x)
    with torch.no_grad():
        assert not ag.enable_autograd().wants_grad(x)
    for p in ag.parameters():
        p.requires_grad_(False)
    assert not ag.wants_grad(x) and ag.wants_grad(x.clone().requires_grad_())
