"""COMA on the CPU: the float64 restatement (tests/coma_ref.py) against the golden fixtures recorded from the reference
(tests/golden/make_coma_golden.py), the config / registry surface, the fake (meta) implementations of the new ops and
the host-only checks of the critic entry points.

The noise floors measured here -- the largest |fp32 fixture - float64 restatement| per quantity over both fixtures and
all three train calls -- set the tolerances of the GPU tests (tests/test_gpu_coma.py: 4x the floor, absolute):

    quantity                         measured floor   GPU tolerance (4x)
    q_vals                           2.36e-07         9.5e-07
    TD(lambda) targets               1.65e-07         6.6e-07
    critic stats (5 keys)            8.03e-08         3.3e-07
    critic / target parameters       1.51e-07         6.1e-07    (every 16th element, after each call)
    actor stats (4 keys)             1.04e-08         4.2e-08
    agent parameters                 1.73e-08         7.0e-08    (every 16th element, after each call)
    critic parameters, all 56335     2.93e-07         1.2e-06    (after call 3; the larger population has the
    agent parameters, all 27535      1.94e-08         7.8e-08     larger maximum)

The assertions below hold the restatement to those floors (with 5 % headroom for another BLAS), so a drift of either
side shows here, on the CPU, first."""
import json

import numpy as np
import pytest
import torch

import coma_ref as CR
from conftest import GOLDEN

FLOORS = {"q_vals": 2.36e-7, "targets": 1.65e-7, "critic_stats": 8.03e-8, "critic_params": 1.51e-7,
          "actor_stats": 1.04e-8, "agent_params": 1.73e-8, "critic_params_full": 2.93e-7, "agent_params_full": 1.94e-8}
TOL = {k: 4.0 * v for k, v in FLOORS.items()}
CRITIC_STATS = ["critic_loss", "critic_grad_norm", "td_error_abs", "q_taken_mean", "target_mean"]
ACTOR_STATS = ["advantage_mean", "coma_loss", "agent_grad_norm", "pi_max"]


def load_learner(tag):
    d = np.load(f"{GOLDEN}/coma_learner_{tag}.npz")
    batch = {k[2:]: d[k] for k in d.files if k.startswith("b.")}
    pa = {k[len("p0.agent."):]: d[k] for k in d.files if k.startswith("p0.agent.")}
    pc = {k[len("p0.critic."):]: d[k] for k in d.files if k.startswith("p0.critic.")}
    return d, batch, pa, pc


@pytest.fixture(scope="module", params=["mask", "nomask"])
def ref_run(request):
    """The float64 learner restatement run for three calls next to the fixture: computed once per fixture."""
    import learner_ref as LR
    d, batch, pa, pc = load_learner(request.param)
    ref = CR.LearnerRef(pa, pc, 5, float(d["epsilon"]), bool(d["mask_before_softmax"]), target_update_interval=10)
    calls = []
    for i in range(3):
        stats, q, tg = ref.train(batch)
        calls.append(dict(stats=stats, q_vals=q, targets=tg, steps=ref.critic.steps, last=ref.critic.last_update,
                          critic=np.concatenate([ref.critic.p[k].reshape(-1) for k in CR.CRITIC_KEYS]),
                          target=np.concatenate([ref.critic.tp[k].reshape(-1) for k in CR.CRITIC_KEYS]),
                          agent=np.concatenate([ref.agent[k].detach().numpy().reshape(-1) for k in LR.AGENT_KEYS])))
    return d, calls


def test_restatement_matches_the_reference_within_the_floors(ref_run):
    d, calls = ref_run
    worst = {k: 0.0 for k in FLOORS}

    def upd(key, got, exp):
        worst[key] = max(worst[key], float(np.abs(np.asarray(got, np.float64) - np.asarray(exp, np.float64)).max()))

    for i, c in enumerate(calls):
        assert c["steps"] == int(d[f"steps{i}"]) == 6 * (i + 1)
        assert c["last"] == int(d[f"last_update{i}"]) == (0 if i == 0 else 12)  # the one update: after call 2
        upd("q_vals", c["q_vals"], d[f"q_vals{i}"])
        upd("targets", c["targets"], d[f"targets{i}"])
        for k in CRITIC_STATS:
            upd("critic_stats", c["stats"][k], d[f"stat{i}.{k}"])
        for k in ACTOR_STATS:
            upd("actor_stats", c["stats"][k], d[f"stat{i}.{k}"])
        upd("critic_params", c["critic"][::16], d[f"sub{i}.critic"])
        upd("critic_params", c["target"][::16], d[f"sub{i}.target_critic"])
        upd("agent_params", c["agent"][::16], d[f"sub{i}.agent"])
    upd("critic_params_full", calls[2]["critic"], np.concatenate([d[f"p3.critic.{k}"].reshape(-1) for k in CR.CRITIC_KEYS]))
    import learner_ref as LR
    upd("agent_params_full", calls[2]["agent"], np.concatenate([d[f"p3.agent.{k}"].reshape(-1) for k in LR.AGENT_KEYS]))
    print("measured floors:", {k: f"{v:.3g}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1.05 * FLOORS[k], (k, v, FLOORS[k])


def test_restated_critic_inputs_have_the_reference_layout():
    d, batch, _, pc = load_learner("mask")
    x = CR.critic_inputs(batch, 2)
    B, N, A, S, DO = 4, 5, 15, 60, 80
    assert x.shape == (B, N, S + DO + 2 * N * A + N) == (B, N, pc["fc1.weight"].shape[1])
    joint = x[:, :, S + DO:S + DO + N * A].reshape(B, N, N, A)
    for n in range(N):
        assert not joint[:, n, n].any()  # the agent's own block is zeroed
        others = [m for m in range(N) if m != n]
        assert np.array_equal(joint[:, n, others], batch["actions_onehot"][:, 2][:, others])
    assert np.array_equal(x[:, :, S + DO + N * A:S + DO + 2 * N * A].reshape(B, N, N, A)[:, 0],
                          batch["actions_onehot"][:, 1])
    assert not CR.critic_inputs(batch, 0)[:, :, S + DO + N * A:S + DO + 2 * N * A].any()
    assert np.array_equal(x[0, :, -N:], np.eye(N))


@pytest.mark.parametrize("A", [11, 15, 55])
def test_restated_softmax_matches_the_reference(A):
    d = np.load(f"{GOLDEN}/coma_policy.npz")
    eps = float(d["epsilon"])
    logits, avail = d[f"A{A}.logits"], d[f"A{A}.avail"]
    for mask in (0, 1):
        for test in (0, 1):
            exp = d[f"A{A}.probs.mask{mask}.test{test}"]
            got = CR.softmax_policy(logits, avail, eps, bool(mask), bool(test))
            assert np.isfinite(got).all()
            np.testing.assert_allclose(got, exp, rtol=2e-6, atol=1e-8)
    # the crafted rows: one available action takes everything that is not the floor's; none available is all zero
    p = CR.softmax_policy(logits, avail, eps, True, False)
    assert p[0, 0, A // 2] == pytest.approx(1.0) and p[0, 0].sum() == pytest.approx(1.0)
    assert not p[0, 1].any()


def test_restated_softmax_gradient_matches_autograd():
    rng = np.random.RandomState(3)
    logits = rng.randn(7, 11)
    avail = (rng.rand(7, 11) < 0.5).astype(np.int32)
    avail[0] = 0
    avail[1] = 0
    avail[1, 4] = 1
    g = rng.randn(7, 11)
    for mask in (False, True):
        for test in (False, True):
            x = torch.tensor(logits, requires_grad=True)
            p = CR.softmax_policy_torch(x, torch.tensor(avail), 0.3, mask, test)
            (p * torch.tensor(g)).sum().backward()
            got = CR.softmax_policy_grad(logits, avail, 0.3, mask, test, g)
            np.testing.assert_allclose(got, x.grad.numpy(), rtol=1e-10, atol=1e-14)
            np.testing.assert_allclose(p.detach().numpy(), CR.softmax_policy(logits, avail, 0.3, mask, test),
                                       rtol=1e-12, atol=1e-15)


def test_restated_multinomial_rule():
    import envref
    p = np.array([0.1, 0.5, 0.2, 0.2], dtype=np.float32)
    avail = np.array([1, 0, 1, 1])
    key = envref.env_key(3, 2)
    counts = np.zeros(4, dtype=np.int64)
    for ep in range(400):
        a = CR.select_multinomial(p, avail, key, ep, 7, 1)
        u = CR.policy_u(key, ep, 7, 1)
        cdf = np.cumsum(np.where(avail != 0, p, 0).astype(np.float32), dtype=np.float32)
        thr = np.float32(u * cdf[-1])
        assert avail[a] and cdf[a] > thr and (a == 0 or cdf[a - 1] <= thr or not avail[:a].any())
        counts[a] += 1
    assert counts[1] == 0 and counts[0] < counts[2] + counts[3]
    assert CR.select_multinomial(p, avail, key, 0, 0, 0, greedy=True) == 2  # the tie 0.2 / 0.2 takes the first index
    assert CR.select_multinomial(p, np.zeros(4, dtype=int), key, 0, 0, 0) == 0
    assert CR.policy_u(key, 1, 2, 3) == np.float32(envref.u01(envref.rng(key, envref.ctr(1, 2, 5, 3))))


# ---- the config / registry surface ---------------------------------------------------------------------------------
def test_builtin_coma_config_equals_the_recorded_yaml():
    from maleague.utils.config import BUILTIN, build_config
    want = json.loads(str(np.load(f"{GOLDEN}/coma_policy.npz")["coma_yaml"]))
    assert BUILTIN["algs/coma"] == want
    cfg = build_config(alg="coma", cuda_available=False)
    for k, v in want.items():
        if k == "env_args":
            assert cfg["env_args"]["state_last_action"] is False
            assert cfg["env_args"]["match_build_plan"] == "medium_1h_4t"  # the env layer's keys survive the merge
        else:
            assert cfg[k] == v, k
    assert cfg["buffer_size"] == cfg["batch_size"] == cfg["batch_size_run"] == 8


def test_registries_resolve_coma():
    from maleague.components.action_selectors import REGISTRY as selectors, MultinomialActionSelector
    from maleague.learners import REGISTRY as learners, COMALearner
    from maleague.modules.critics import REGISTRY as critics, COMACritic
    from helpers import qmix_args
    assert learners["coma"] is COMALearner and critics["coma"] is COMACritic
    sel = selectors["multinomial"](qmix_args(epsilon_start=0.5, epsilon_finish=0.01, epsilon_anneal_time=100000))
    assert isinstance(sel, MultinomialActionSelector) and sel.epsilon == 0.5 and sel.test_greedy is True


def test_critic_module_has_the_reference_state_dict():
    from maleague.modules.critics import COMACritic
    from helpers import qmix_args
    args = qmix_args(device="cpu")
    scheme = {"state": {"vshape": 60}, "obs": {"vshape": 80}, "actions_onehot": {"vshape": (15,)}}
    c = COMACritic(scheme, args)
    shapes = {k: tuple(v.shape) for k, v in c.state_dict().items()}
    assert shapes == {"fc1.weight": (128, 295), "fc1.bias": (128,), "fc2.weight": (128, 128), "fc2.bias": (128,),
                      "fc3.weight": (15, 128), "fc3.bias": (15,)}
    d, _, _, pc = load_learner("mask")
    c.load_state_dict({k: torch.from_numpy(v) for k, v in pc.items()})  # the reference's critic.th layout


def test_pi_logits_is_refused_where_it_is_out_of_scope():
    from helpers import qmix_args
    from maleague.league.evaluation import CrossPlayEvaluator
    with pytest.raises(NotImplementedError, match="agent_output_type"):
        CrossPlayEvaluator(qmix_args(agent_output_type="pi_logits", device="cpu"), "cpu")


def test_td_lambda_targets_python_surface():
    from maleague.learners.coma_learner import build_td_lambda_targets
    rng = np.random.RandomState(5)
    B, T, N = 3, 6, 2
    tq = rng.randn(B, T, N)
    r, m = rng.randn(B, T - 1), (rng.rand(B, T - 1) < 0.8).astype(np.float64)
    term = np.zeros((B, T - 1))
    term[0, 3] = 1
    got = build_td_lambda_targets(torch.tensor(r)[..., None], torch.tensor(term)[..., None], torch.tensor(m)[..., None],
                                  torch.tensor(tq), N, 0.99, 0.8)
    np.testing.assert_allclose(got.numpy(), CR.td_lambda_targets(r, term, m, tq, 0.99, 0.8), rtol=1e-12)


# ---- the ops' fake implementations and the host-only checks ---------------------------------------------------------
def test_new_ops_registered_with_fake_shapes():
    import maleague  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    from maleague.ops import OPS
    for name in ("policy_probs", "policy_probs_backward", "select_multinomial", "coma_policy_loss"):
        assert name in OPS and hasattr(torch.ops.maleague, name)
    with FakeTensorMode():
        x, av = torch.empty(8, 5, 15), torch.empty(8, 5, 15, dtype=torch.int32)
        p = torch.ops.maleague.policy_probs(x, av, 0.3, 1, 0)
        assert p.shape == (8, 5, 15) and p.dtype == torch.float32
        assert torch.ops.maleague.policy_probs_backward(x, av, x, 0.3, 1, 0).shape == (8, 5, 15)
        a = torch.ops.maleague.select_multinomial(x, av, torch.empty(8, dtype=torch.int64),
                                                  torch.empty(8, dtype=torch.int32), 0, 0)
        assert a.shape == (8, 5) and a.dtype == torch.int64
        pi, avail = torch.empty(4, 6, 5, 15), torch.empty(4, 6, 5, 15, dtype=torch.int32)
        st, dpi = torch.ops.maleague.coma_policy_loss(pi, avail, torch.empty(4, 6, 5, 1, dtype=torch.int64), pi,
                                                      torch.empty(4, 6, 1))
        assert st.shape == (4,) and dpi.shape == (4, 6, 5, 15)


def test_new_ops_refuse_host_tensors():
    import maleague  # noqa: F401
    from maleague._native import NativeError
    with pytest.raises((NativeError, RuntimeError)):
        torch.ops.maleague.policy_probs(torch.zeros(2, 3), torch.ones(2, 3, dtype=torch.int32), 0.1, 1, 0)


def _cfg(**kw):
    from maleague import _native
    base = dict(B=4, T=7, N=5, A=15, d_obs=80, S=60, hidden=128, lr=5e-4, optim_alpha=0.99, optim_eps=1e-5,
                grad_norm_clip=10.0, gamma=0.99, td_lambda=0.8)
    base.update(kw)
    return _native.MlgComaCfg(**base)


def test_critic_workspace_query_is_host_only_and_refuses_unsupported_shapes():
    from maleague import _native
    lib = _native.load()
    cfg = _cfg()
    assert lib.mlg_coma_param_count(_native.byref(cfg)) == 128 * 295 + 128 + 128 * 128 + 128 + 15 * 128 + 15
    assert lib.mlg_coma_workspace_floats(_native.byref(cfg)) > 0
    for kw, word in ((dict(hidden=64), b"hidden"), (dict(N=33), b"N=33"), (dict(A=97), b"A=97")):
        bad = _cfg(**kw)
        assert lib.mlg_coma_workspace_floats(_native.byref(bad)) == -1
        assert word in lib.mlg_last_error(), lib.mlg_last_error()
        assert lib.mlg_coma_param_count(_native.byref(bad)) == -1
    big = _cfg(B=64, N=32, A=96, T=101)
    assert lib.mlg_coma_workspace_floats(_native.byref(big)) > 0


def test_struct_layout_matches_the_header():
    """MlgComaCfg: seven int32, three floats, then three doubles on an 8-byte boundary (40); MlgComaBufs: the batch
    struct followed by nine pointers."""
    import ctypes
    from maleague import _native
    assert _native.MlgComaCfg.gamma.offset == 40 and ctypes.sizeof(_native.MlgComaCfg) == 64
    assert ctypes.sizeof(_native.MlgComaBufs) == ctypes.sizeof(_native.MlgBatch) + 9 * ctypes.sizeof(ctypes.c_void_p)
