"""GPU parity of the fused learner (mlg_qlearner_train) per dispatch arm: rnn_hidden_dim 32 / 64 / 128, teams of 1 to
32, the three bounds of the prefetching mixer forms crossed one at a time, A = 96, VDN and IQL off the default shape.
The cases, their batches and weights are tests/learner_arm_shapes.py's; tests/test_learner_dispatch.py pins on the CPU
the arm every test here first asserts.

Yardsticks. Three-call trajectories: the fp32 CPU oracle (oracle/learner_ref.py), statistics rtol 2e-4 / atol 1e-6 and
parameters atol 5e-5, the project's bounds against the oracle. First-call gradients: the same oracle in float64 before
its clip, per tensor max|g - g_ref| <= 1e-4 max(1, max|g_ref|), test_gpu_autograd.py's bound. Either would be ten times
the fp32 oracle's own distance from float64 (learner_arm_shapes.ORACLE_F64, measured on the CPU) where that were
larger; it is not for any case. Parameters after RMSprop compress an error of single gradient elements (the first
step is lr g / (0.1 |g| + eps)), which is why the gradients are compared directly as well.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import learner_arm_shapes as LA
import learner_ref as LR
from helpers import Q_TOL, build_stepper, shape_plan
from test_gpu_learner_shapes import STAT_KEYS, _episode_batch, _learner

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = LA.case(cid)
    args = LA.case_args(c)
    agent0, mixer0 = LA.case_weights(c, args)
    tb = LA.case_batch(c)
    assert tb["filled"].sum(dim=(1, 2)).tolist() == list(LA.LENS)
    n_av = tb["avail_actions"].sum(-1)
    assert bool((n_av > 0).all()) and 0.1 < float((n_av == 1).float().mean()) < 0.35
    assert bool((torch.gather(tb["avail_actions"], 3, tb["actions"]) == 1).all())
    return c, args, agent0, mixer0, tb


@functools.lru_cache(maxsize=None)
def _oracle(cid):
    """Computed once per case: the fp32 oracle's three calls (statistics per call, the oracle after them) and the
    float64 oracle's first-call gradients before the clip, in flat parameter order."""
    c, args, agent0, mixer0, tb = _inputs(cid)
    ob = LA.oracle_batch(tb)
    ref = LR.QLearnerRef(agent0, mixer0, LR.clone_args(args, device="cpu"))
    stats = [ref.train({k: v.clone() for k, v in ob.items()}, t_env, ep) for t_env, ep in LA.CALLS]
    ref64 = LR.QLearnerRef(agent0, mixer0, LR.clone_args(args, device="cpu"), dtype=torch.float64)
    s64 = ref64.train({k: v.clone() for k, v in ob.items()}, *LA.CALLS[0])
    return stats, ref, [g.clone() for g in ref64.last_grads], s64


def _fresh(cid, device):
    c, args, agent0, mixer0, tb = _inputs(cid)
    eb = _episode_batch(tb, device)
    learner, _ = _learner(eb, agent0, mixer0, args)
    assert eb.max_seq_length == LA.T_STORED and int(eb.max_t_filled()) == LA.T_FILLED
    return learner, eb


def _run(cid, device):
    """A fresh learner's three calls: statistics per call, the first call's raw stats and gradients."""
    learner, eb = _fresh(cid, device)
    out = {"stats": [], "learner": learner}
    for i, (t_env, ep) in enumerate(LA.CALLS):
        learner.train(eb, t_env, ep)
        out["stats"].append(dict(learner.last_stats))
        if i == 0:
            out["stats0"] = learner._stats.cpu().numpy().copy()
            out["grads0"] = learner._grads.cpu().clone()
    out["grads"] = learner._grads.cpu().numpy().copy()
    out["params"] = learner._flat.flat.cpu().numpy().copy()
    out["tparams"] = learner._tflat.flat.cpu().numpy().copy()
    return out


_RUNS = {}


def _shared_run(cid, device):
    if cid not in _RUNS:
        _RUNS[cid] = _run(cid, device)
    return _RUNS[cid]


def _assert_arm(cid):
    c = LA.case(cid)
    assert LA.describe(c) == c.arm
    return c


# ---- a. three-call trajectory against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("cid", LA.IDS)
def test_three_call_trajectory_vs_oracle(device, cid):
    c = _assert_arm(cid)
    _, args, _, _, tb = _inputs(cid)
    want, ref, _, _ = _oracle(cid)
    got = _shared_run(cid, device)
    learner = got["learner"]
    rtol, atol, _ = LA.bounds(cid)
    for i in range(len(LA.CALLS)):
        print(f"  {cid} call {i}: " + ", ".join(f"{k} {got['stats'][i][k]:.7g}/{want[i][k]:.7g}" for k in STAT_KEYS))
    for i in range(len(LA.CALLS)):
        for k in STAT_KEYS:
            assert np.isfinite(got["stats"][i][k]), f"{cid} call {i} {k}"
            np.testing.assert_allclose(got["stats"][i][k], want[i][k], rtol=rtol, atol=LA.STAT_ATOL,
                                       err_msg=f"{cid} call {i} {k}")
    assert learner.last_target_update_episode == ref.last_target_update_episode == 200
    pairs = [("agent", learner.mac.agent.state_dict(), ref.agent_state()),
             ("target agent", learner.target_mac.agent.state_dict(), ref.tp)]
    if args.mixer == "qmix":
        pairs += [("mixer", learner.mixer.state_dict(), ref.mixer_state()),
                  ("target mixer", learner.target_mixer.state_dict(), ref.tmp)]
    errs = {}
    for name, g, w in pairs:
        assert list(g.keys()) == list(w.keys())
        for k, v in g.items():
            errs[f"{name} {k}"] = float(np.abs(v.cpu().numpy() - w[k].detach().numpy()).max())
    worst = max(errs, key=errs.get)
    print(f"  {cid}: max parameter error {errs[worst]:.3e} at {worst} (bound {atol:.1e})")
    for k, e in errs.items():
        assert e <= atol, f"{cid} {k}: {e:.3e} > {atol:.1e}"
    assert np.array_equal(got["params"], got["tparams"])  # the third call ended with the sync
    n = LA.mask_sum(tb) * (args.n_agents if args.mixer is None else 1)  # IQL expands the mask over the agents
    assert float(learner._stats[5]) == n and float(learner._stats[6]) == n
    assert learner.mac.agent.trained_steps == ref.trained_steps == len(LA.CALLS) * int(n)


# ---- b. first-call gradients against the float64 oracle --------------------------------------------------------------
@pytest.mark.parametrize("cid", LA.IDS)
def test_first_call_gradients_vs_float64_oracle(device, cid):
    """learner._grads after the first call, scaled back by the clip factor clip_grad_norm_ applied (from the call's
    own grad_norm, stats[1]), per tensor of the flat vector against the float64 oracle's .grad before its clip."""
    _assert_arm(cid)
    _, args, _, _, _ = _inputs(cid)
    _, _, g64, s64 = _oracle(cid)
    got = _shared_run(cid, device)
    learner = got["learner"]
    norm = float(got["stats0"][1])
    np.testing.assert_allclose(norm, s64["grad_norm"], rtol=LA.bounds(cid)[0])
    assert (norm > args.grad_norm_clip) == LA.clips(cid, args.grad_norm_clip), norm
    coef = min(1.0, args.grad_norm_clip / (norm + 1e-6))  # clip_grad_norm_
    assert len(g64) == len(learner._flat.views)
    bound = LA.bounds(cid)[2]
    worst = 0.0
    for (q, off, k), ref in zip(learner._flat.views, g64):
        assert tuple(q.shape) == tuple(ref.shape)
        mine = got["grads0"][off:off + k].view_as(q).to(torch.float64) / coef
        err, scale = float((mine - ref).abs().max()), max(1.0, float(ref.abs().max()))
        worst = max(worst, err / scale)
        assert err <= bound * scale, f"{cid} tensor at {off} {tuple(q.shape)}: max error {err:.3e} > {bound * scale:.3e}"
    print(f"  {cid}: grad_norm {norm:.6g} (clip factor {coef:.4g}), largest gradient error / scale {worst:.3e}")


def test_some_cases_clip_and_some_do_not():
    assert LA.clips("generic-h64-32v32") and LA.clips("split-h32-2v2")
    assert not LA.clips("iql-h128-2v2") and not LA.clips("split-h128-4v4")


# ---- c. no stale reads, skip equals full ------------------------------------------------------------------------------
def _snapshots(cid, device, monkeypatch, full):
    if full:
        monkeypatch.setenv("MLG_LEARNER_FULL", "1")
    else:
        monkeypatch.delenv("MLG_LEARNER_FULL", raising=False)
    from maleague import _native
    learner, eb = _fresh(cid, device)
    if not full:  # the first call too starts from a NaN workspace (train() keeps a buffer that is large enough)
        need = _native.load().mlg_qlearner_workspace_floats(_native.byref(learner._cfg(eb.batch_size, eb.max_seq_length)))
        assert need > 0
        learner._ws = torch.empty(int(need) + 1024, dtype=torch.float32, device=device)
    out = []
    for i, ep in enumerate([0, 200, 200]):  # target a copy, stale (then synced), a copy again
        if not full:  # no kernel may read a workspace element the call did not write
            learner._ws.fill_(float("nan"))
        learner.train(eb, i, ep)
        torch.cuda.synchronize()
        out.append({"stats": learner._stats.cpu().numpy().copy(), "grads": learner._grads.cpu().numpy().copy(),
                    "params": learner._flat.flat.cpu().numpy().copy(), "sq": learner._sq.cpu().numpy().copy()})
    monkeypatch.delenv("MLG_LEARNER_FULL", raising=False)
    return out


@pytest.mark.parametrize("cid", ["split-h32-2v2", "split-h128-4v4", "split-at-bounds", "generic-h128-9v9",
                                 "vdn-h64-7v7", "iql-h128-2v2"])
def test_skip_path_equals_full_path(device, monkeypatch, cid):
    _assert_arm(cid)
    got = _snapshots(cid, device, monkeypatch, False)
    want = _snapshots(cid, device, monkeypatch, True)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ("stats", "grads", "params", "sq"):
            assert np.all(np.isfinite(g[k])), f"call {i}: {k} not finite"
        assert np.array_equal(g["stats"][:7], w["stats"][:7]), f"call {i}: {g['stats']} vs {w['stats']}"
        for k in ("grads", "params", "sq"):
            assert np.array_equal(g[k], w[k]), f"call {i}: {k} differ at {np.flatnonzero(g[k] != w[k])[:8]}"
    assert got[0]["stats"][7] < want[0]["stats"][7]  # the default path planned fewer forward blocks


# ---- d. trained on the HIP rollout of the same shape -----------------------------------------------------------------
@pytest.mark.parametrize("cid", ["split-h32-2v2", "generic-h128-9v9"])
def test_qlearner_vs_oracle_on_rollout_of_the_shape(device, cid):
    """test_qlearner_vs_oracle_on_rollout at 2v2 / H = 32 and 9v9 / H = 128: one QLearner.train on the untruncated
    train-mode batch of ParallelStepper (B = 8, episode_limit 20: real availability masks) against the oracle on the
    copy truncated to max_t_filled, and the trained agent's Q within 1e-4 of the oracle's forward."""
    from maleague import _native
    from maleague.learners import QLearner
    from test_gpu_learner_shapes import _Log
    c = LA.case(cid)
    stepper, mac, args = build_stepper(device, plan=shape_plan(c.dims), B=8, episode_limit=20, seed=c.seed,
                                       rnn_hidden_dim=c.H)
    assert (args.n_agents, args.n_actions, args.state_shape) == LA.dims(c)[:3]
    learner = QLearner(mac, None, _Log(), args, name="home")  # the scheme is kept, not read
    agent0 = {k: v.detach().cpu().clone() for k, v in mac.agent.state_dict().items()}
    mixer0 = {k: v.detach().cpu().clone() for k, v in learner.mixer.state_dict().items()}
    learner.build_optimizer()
    stepper.t_env = 30000
    batch, _ = stepper.run(test_mode=False)
    T = int(batch.max_t_filled())
    assert batch.batch_size == 8 and batch.max_seq_length == 21 and 2 <= T <= 21
    assert _native.qlearner_describe(learner._cfg(8, T)) == c.arm
    tb = {k: v[:, :T].detach().cpu().clone() for k, v in batch.data.transition_data.items()}
    ref = LR.QLearnerRef(agent0, mixer0, copy.copy(args))
    want = ref.train({k: v.clone() for k, v in tb.items()}, 30000, 0)
    learner.train(batch, 30000, 0)
    print(f"  {cid} T={T}: " + ", ".join(f"{k} {learner.last_stats[k]:.7g}/{want[k]:.7g}" for k in STAT_KEYS))
    for k in STAT_KEYS:
        np.testing.assert_allclose(learner.last_stats[k], want[k], rtol=LA.STAT_RTOL, atol=LA.STAT_ATOL, err_msg=k)
    for k, v in learner.mac.agent.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), ref.agent_state()[k].numpy(), atol=LA.PARAM_ATOL, rtol=0, err_msg=k)
    for k, v in learner.mixer.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), ref.mixer_state()[k].numpy(), atol=LA.PARAM_ATOL, rtol=0, err_msg=k)
    q_ref, _ = LR.mac_unroll({k: v.detach().cpu() for k, v in learner.mac.agent.state_dict().items()}, tb,
                             args.n_agents, T=T)
    learner.mac.init_hidden(batch.batch_size)
    for t in range(T):
        q = learner.mac.forward(batch, t)
        np.testing.assert_allclose(q.cpu().numpy(), q_ref[:, t].numpy(), atol=Q_TOL, rtol=0)
    stepper.close_env()


# ---- e. determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["generic-h64-32v32", "split-h128-4v4"])
def test_two_fresh_learners_agree_bitwise(device, cid):
    _assert_arm(cid)
    a, b = _run(cid, device), _run(cid, device)
    for k in ("grads", "params", "tparams"):
        assert np.array_equal(a[k], b[k]), f"{k} differ at {np.flatnonzero(a[k] != b[k])[:8]}"
    assert torch.equal(a["grads0"], b["grads0"]) and np.array_equal(a["stats0"], b["stats0"])


# ---- f. the reference's golden off the default agent shape -----------------------------------------------------------
def test_qlearner_9v9_h128_golden(device, golden):
    """The learner against the reference QLearner's own three calls at N = 9, A = 23, S = 108, d_obs = 144, H = 128
    (h128/bwd-split/q2 + qmix-generic), with the golden bounds of test_gpu_learner.py: statistics rtol 1e-4 / atol
    1e-6, parameters atol 2e-5."""
    from maleague import _native
    from helpers import qmix_args
    from test_gpu_learner_shapes import _golden_agent
    d = LA.SplitGolden(golden)
    args = qmix_args(**LA.GOLDEN_9V9_KW)
    mixer0 = {k[len("p0.mixer."):]: np.array(d[k]) for k in d.files if k.startswith("p0.mixer.")}
    eb = _episode_batch(LR.batch_from_npz(d), device)
    learner, log = _learner(eb, _golden_agent(d), mixer0, args)
    assert _native.qlearner_describe(learner._cfg(eb.batch_size, eb.max_seq_length)) == LA.case("generic-h128-9v9").arm
    for i, (t_env, ep) in enumerate(d["calls"]):
        learner.train(eb, int(t_env), int(ep))
        want = {k: float(d[f"stat{i}.{k}"]) for k in STAT_KEYS}
        print(f"  call {i}: " + ", ".join(f"{k} {learner.last_stats[k]:.7g}/{want[k]:.7g}" for k in STAT_KEYS))
        for k in STAT_KEYS:
            np.testing.assert_allclose(learner.last_stats[k], want[k], rtol=1e-4, atol=1e-6, err_msg=f"call {i} {k}")
        assert log.stats["home_qlearner_loss"] == learner.last_stats["loss"]
    last = len(d["calls"])
    for name, sd in (("agent", learner.mac.agent.state_dict()), ("target_agent", learner.target_mac.agent.state_dict()),
                     ("mixer", learner.mixer.state_dict())):
        for k, v in sd.items():
            np.testing.assert_allclose(v.cpu().numpy(), d[f"p{last}.{name}.{k}"], atol=2e-5, rtol=0,
                                       err_msg=f"{name} {k}")
    assert learner.mac.agent.trained_steps == int(d["trained_steps"])
