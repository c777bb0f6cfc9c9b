"""GPU parity of the fused learner with a feed-forward agent (mlg_qlearner_train, MlgLearnerCfg.agent = 1) per
dispatch name of tests/dqn_shapes.py (tests/test_dqn.py pins the names on the CPU), by the method and with the bounds
of tests/test_gpu_learner_arms.py and tests/test_gpu_learner.py:

  three-call trajectories against the fp32 oracle (tests/dqn_ref.DQNLearnerRef): statistics rtol 2e-4 / atol 1e-6,
  parameters atol 5e-5; first-call gradients per tensor against the float64 oracle before the clip:
  max|g - g_ref| <= 1e-4 max(1, max|g_ref|); the reference's goldens: statistics rtol 1e-4 / atol 1e-6, parameters
  atol 2e-5; MLG_LEARNER_FULL=1 from a NaN-filled workspace, a garbage-filled workspace and a second fresh learner:
  identical bits.
"""
import functools
import os

import numpy as np
import pytest
import torch

import dqn_ref
import dqn_shapes as DS
import learner_arm_shapes as LA
import learner_ref as LR
from helpers import Q_TOL, qmix_args
from test_gpu_learner_shapes import STAT_KEYS, _episode_batch, _golden_agent, _learner, mixer_state

pytestmark = pytest.mark.gpu

F64 = torch.float64


@functools.lru_cache(maxsize=None)
def _inputs(cid, reward_scale=1.0):
    c = DS.learner_case(cid)
    args = DS.learner_args(c)
    agent0 = dqn_ref.agent_state(args, LA.dims(c)[3], seed=c.seed)
    mixer0 = mixer_state(args, seed=c.seed + 8) if args.mixer == "qmix" else None
    tb = LA.case_batch(c)
    tb["reward"] = tb["reward"] * reward_scale
    assert tb["filled"].sum(dim=(1, 2)).tolist() == list(LA.LENS)
    return c, args, agent0, mixer0, tb


@functools.lru_cache(maxsize=None)
def _oracle(cid, reward_scale=1.0):
    """Once per case: the fp32 oracle's three calls and the float64 oracle's first call (gradients before the clip)."""
    c, args, agent0, mixer0, tb = _inputs(cid, reward_scale)
    ob = LA.oracle_batch(tb)
    ref = dqn_ref.DQNLearnerRef(agent0, mixer0, LR.clone_args(args, device="cpu"))
    stats = [ref.train({k: v.clone() for k, v in ob.items()}, t_env, ep) for t_env, ep in LA.CALLS]
    ref64 = dqn_ref.DQNLearnerRef(agent0, mixer0, LR.clone_args(args, device="cpu"), dtype=F64)
    s64 = ref64.train({k: v.clone() for k, v in ob.items()}, *LA.CALLS[0])
    return stats, ref, [g.clone() for g in ref64.last_grads], s64


def _fresh(cid, device, reward_scale=1.0):
    from maleague import _native
    c, args, agent0, mixer0, tb = _inputs(cid, reward_scale)
    eb = _episode_batch(tb, device)
    learner, _ = _learner(eb, agent0, mixer0, args)
    assert eb.max_seq_length == LA.T_STORED and int(eb.max_t_filled()) == LA.T_FILLED
    cfg = learner._cfg(eb.batch_size, eb.max_seq_length)
    assert cfg.agent == 1 and _native.qlearner_describe(learner._cfg(LA.B, LA.T_FILLED)) == c.arm
    return learner, eb


def _run(cid, device, reward_scale=1.0, ws_fill=None):
    learner, eb = _fresh(cid, device, reward_scale)
    if ws_fill is not None:
        from maleague import _native
        need = _native.load().mlg_qlearner_workspace_floats(_native.byref(learner._cfg(eb.batch_size, eb.max_seq_length)))
        learner._ws = torch.empty(int(need) + 1024, dtype=torch.float32, device=device)
    out = {"stats": [], "learner": learner, "raw": []}
    for i, (t_env, ep) in enumerate(LA.CALLS):
        if ws_fill is not None:
            ws_fill(learner._ws, i)
        learner.train(eb, t_env, ep)
        out["stats"].append(dict(learner.last_stats))
        out["raw"].append((learner._stats.cpu().numpy().copy(), learner._grads.cpu().numpy().copy(),
                           learner._flat.flat.cpu().numpy().copy(), learner._sq.cpu().numpy().copy()))
        if i == 0:
            out["stats0"] = learner._stats.cpu().numpy().copy()
            out["grads0"] = learner._grads.cpu().clone()
    out["params"] = learner._flat.flat.cpu().numpy().copy()
    out["tparams"] = learner._tflat.flat.cpu().numpy().copy()
    return out


_RUNS = {}


def _shared_run(cid, device):
    if cid not in _RUNS:
        _RUNS[cid] = _run(cid, device)
    return _RUNS[cid]


def _check_trajectory(cid, got, want, ref, args, tb):
    learner = got["learner"]
    for i in range(len(LA.CALLS)):
        print(f"  {cid} call {i}: " + ", ".join(f"{k} {got['stats'][i][k]:.7g}/{want[i][k]:.7g}" for k in STAT_KEYS))
    for i in range(len(LA.CALLS)):
        for k in STAT_KEYS:
            assert np.isfinite(got["stats"][i][k]), f"{cid} call {i} {k}"
            np.testing.assert_allclose(got["stats"][i][k], want[i][k], rtol=LA.STAT_RTOL, atol=LA.STAT_ATOL,
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
    print(f"  {cid}: max parameter error {errs[worst]:.3e} at {worst} (bound {LA.PARAM_ATOL:.1e})")
    for k, e in errs.items():
        assert e <= LA.PARAM_ATOL, f"{cid} {k}: {e:.3e} > {LA.PARAM_ATOL:.1e}"
    assert np.array_equal(got["params"], got["tparams"])  # the third call ended with the sync
    n = LA.mask_sum(tb) * (args.n_agents if args.mixer is None else 1)  # IQL expands the mask over the agents
    assert float(learner._stats[5]) == n and float(learner._stats[6]) == n
    assert learner.mac.agent.trained_steps == ref.trained_steps == len(LA.CALLS) * int(n)


def _check_gradients(cid, got, g64, s64, args, expect_clip=None):
    learner = got["learner"]
    norm = float(got["stats0"][1])
    np.testing.assert_allclose(norm, s64["grad_norm"], rtol=LA.STAT_RTOL)
    coef = min(1.0, args.grad_norm_clip / (norm + 1e-6))  # clip_grad_norm_
    if expect_clip is not None:
        assert (coef < 1.0) == expect_clip, (norm, coef)
    assert len(g64) == len(learner._flat.views)
    worst = 0.0
    for (q, off, k), ref in zip(learner._flat.views, g64):
        assert tuple(q.shape) == tuple(ref.shape)
        mine = got["grads0"][off:off + k].view_as(q).to(F64) / coef
        err, scale = float((mine - ref).abs().max()), max(1.0, float(ref.abs().max()))
        worst = max(worst, err / scale)
        assert err <= LA.GRAD_RTOL * scale, f"{cid} tensor at {off} {tuple(q.shape)}: {err:.3e} > {LA.GRAD_RTOL * scale:.3e}"
    print(f"  {cid}: grad_norm {norm:.6g} (clip factor {coef:.4g}), largest gradient error / scale {worst:.3e}")
    return coef


# ---- a. three-call trajectory (target equal; stale; stale and synced by the call) ------------------------------------
@pytest.mark.parametrize("cid", DS.LEARNER_IDS)
def test_three_call_trajectory_vs_oracle(device, cid):
    _, args, _, _, tb = _inputs(cid)
    want, ref, _, _ = _oracle(cid)
    _check_trajectory(cid, _shared_run(cid, device), want, ref, args, tb)


# ---- b. first-call gradients against the float64 oracle, before the clip ------------------------------------------------
@pytest.mark.parametrize("cid", DS.LEARNER_IDS)
def test_first_call_gradients_vs_float64_oracle(device, cid):
    _, args, _, _, _ = _inputs(cid)
    _, _, g64, s64 = _oracle(cid)
    _check_gradients(cid, _shared_run(cid, device), g64, s64, args)


def test_scaled_rewards_clip_the_gradient(device):
    """The VDN case with rewards times 40: the float64 oracle's first-call norm is above grad_norm_clip (it is below
    for the unscaled case), so the clip coefficient falls below 1; trajectory and gradients hold as for the others."""
    cid, scale = "ff-vdn-h32-3v3", 40.0
    _, args, _, _, tb = _inputs(cid, scale)
    want, ref, g64, s64 = _oracle(cid, scale)
    assert _oracle(cid)[3]["grad_norm"] < args.grad_norm_clip < s64["grad_norm"]
    got = _run(cid, device, scale)
    assert _check_gradients(cid, got, g64, s64, args, expect_clip=True) < 1.0
    _check_trajectory(cid, got, want, ref, args, tb)


# ---- c. no stale reads: skip = full, garbage = zero, determinism -----------------------------------------------------
def _raw_equal(a, b, what, stats_upto=8):
    for i, (x, y) in enumerate(zip(a["raw"], b["raw"])):
        assert np.array_equal(x[0][:stats_upto], y[0][:stats_upto]), f"{what} call {i}: stats {x[0]} vs {y[0]}"
        for k, name in ((1, "grads"), (2, "params"), (3, "sq")):
            assert np.all(np.isfinite(x[k])), f"{what} call {i}: {name} not finite"
            assert np.array_equal(x[k], y[k]), f"{what} call {i}: {name} differ at {np.flatnonzero(x[k] != y[k])[:8]}"


@pytest.mark.parametrize("cid", ["ff-qmix-h64-5v5", "ff-qmix-h128-17v17", "ff-vdn-h32-3v3", "ff-iql-h128-2v2",
                                 "ff-h1-e32-h64-7v7"])
def test_skip_path_equals_full_path_from_nan_workspace(device, monkeypatch, cid):
    """Every call starts from a NaN-filled workspace, so no kernel reads a word the call did not write; the same calls
    under MLG_LEARNER_FULL=1 give the same bits (stats[7], the planned blocks, is larger there)."""
    nan_fill = lambda ws, i: ws.fill_(float("nan"))  # noqa: E731
    monkeypatch.delenv("MLG_LEARNER_FULL", raising=False)
    got = _run(cid, device, ws_fill=nan_fill)
    monkeypatch.setenv("MLG_LEARNER_FULL", "1")
    want = _run(cid, device, ws_fill=nan_fill)
    monkeypatch.delenv("MLG_LEARNER_FULL", raising=False)
    _raw_equal(got, want, cid, stats_upto=7)
    assert got["raw"][0][0][7] < want["raw"][0][0][7]


@pytest.mark.parametrize("cid", ["ff-qmix-h32-1v1", "ff-vdn-h64-17v17", "ff-he32-e16-h32-5v5"])
def test_garbage_workspace_equals_zeroed_and_two_learners_agree(device, cid):
    """A workspace refilled with finite garbage before every call equals a zeroed one, and both equal the shared run
    of a third fresh learner: bit for bit."""
    garbage = _run(cid, device, ws_fill=lambda ws, i: ws.copy_(torch.randn_like(ws) * 1e3))
    zeroed = _run(cid, device, ws_fill=lambda ws, i: ws.zero_())
    _raw_equal(garbage, zeroed, cid)
    _raw_equal(zeroed, _run(cid, device), cid)


# ---- d. the reference's goldens through QLearner itself --------------------------------------------------------------
@pytest.mark.parametrize("tag,kw,arm", [("dqn_qmix", {}, "ff-h64/q1 + qmix-generic"),
                                        ("dqn_vdn", {"mixer": "vdn"}, "ff-h64/q1 + vdn-fast")])
def test_reference_golden_trajectory(device, golden, tag, kw, arm):
    from maleague import _native
    d = golden(f"qlearner_{tag}.npz")
    args = qmix_args(agent="dqn", **kw)
    mixer0 = {k[len("p0.mixer."):]: np.array(d[k]) for k in d.files if k.startswith("p0.mixer.")} or None
    eb = _episode_batch(LR.batch_from_npz(d), device)
    learner, log = _learner(eb, _golden_agent(d), mixer0, args)
    assert list(_golden_agent(d)) == dqn_ref.AGENT_KEYS
    assert _native.qlearner_describe(learner._cfg(eb.batch_size, eb.max_seq_length)) == arm
    for i, (t_env, ep) in enumerate(d["calls"]):
        learner.train(eb, int(t_env), int(ep))
        want = {k: float(d[f"stat{i}.{k}"]) for k in STAT_KEYS}
        print(f"  {tag} call {i}: " + ", ".join(f"{k} {learner.last_stats[k]:.7g}/{want[k]:.7g}" for k in STAT_KEYS))
        for k in STAT_KEYS:
            np.testing.assert_allclose(learner.last_stats[k], want[k], rtol=1e-4, atol=1e-6, err_msg=f"call {i} {k}")
    last = len(d["calls"])
    sds = [("agent", learner.mac.agent.state_dict()), ("target_agent", learner.target_mac.agent.state_dict())]
    if mixer0 is not None:
        sds.append(("mixer", learner.mixer.state_dict()))
    worst = 0.0
    for name, sd in sds:
        for k, v in sd.items():
            worst = max(worst, float(np.abs(v.cpu().numpy() - d[f"p{last}.{name}.{k}"]).max()))
            np.testing.assert_allclose(v.cpu().numpy(), d[f"p{last}.{name}.{k}"], atol=2e-5, rtol=0, err_msg=f"{name} {k}")
    print(f"  {tag}: max parameter error {worst:.3e} (bound 2e-5)")
    assert learner.mac.agent.trained_steps == int(d["trained_steps"])


# ---- e. end to end ---------------------------------------------------------------------------------------------------
def test_qmix_dqn_end_to_end(device, tmp_path):
    """MultiAgentExperiment with --config=qmix --agent=dqn on the 3v3 plan, 8 envs, four iterations: it trains on its
    own rollout's batches, statistics are finite, every parameter moved, the trained MAC's Q are within 1e-4 of the
    oracle's forward, and save_models / load_models round-trips (agent.th in the reference's key order)."""
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.learners import QLearner
    from maleague.modules.agents import DQNAgentNetwork
    from maleague.runs import MultiAgentExperiment
    from maleague.utils.config import build_config, to_args
    cfg = build_config("qmix", "ma", overrides=["agent=dqn", "runner=parallel", "batch_size_run=8", "batch_size=8",
                                                "buffer_cpu_only=False", "buffer_size=16", "env_args.episode_limit=20",
                                                "env_args.match_build_plan=small", "seed=0",
                                                "show_exp_parameters=False", "t_max=1000000",
                                                "test_interval=100000000", f"local_results_path={tmp_path}"])
    np.random.seed(0)
    torch.manual_seed(0)
    exp = MultiAgentExperiment(to_args(cfg), MainLogger(log_interval=10 ** 12))
    learner = exp.home_learner
    assert type(learner) is QLearner and isinstance(learner.mac.agent, DQNAgentNetwork)
    before = learner._flat.flat.clone() if learner.optimiser is not None else None
    exp._init_stepper()
    assert exp.stepper.describe_rollout()[0] == "ff-lds/tpw1"
    if before is None:
        before = learner._flat.flat.clone()
    for i in range(4):
        exp._train_episode(i * 8)
    assert learner.train_calls == 4
    stats = learner.last_stats
    assert all(np.isfinite(stats[k]) for k in STAT_KEYS), stats
    assert learner.mac.agent.trained_steps > 0
    for p, off, k in learner._flat.views:
        assert not torch.equal(learner._flat.flat[off:off + k], before[off:off + k]), tuple(p.shape)
    batch, _ = exp.stepper.run(test_mode=True)
    T = int(batch.max_t_filled())
    tb = {k: batch[k][:, :T].detach().cpu() for k in ("obs", "actions_onehot")}
    q64 = dqn_ref.oracle_q(learner.mac, tb, exp.args.n_agents, T, F64)
    learner.mac.init_hidden(batch.batch_size)
    with torch.no_grad():
        q = torch.stack([learner.mac.forward(batch, t) for t in range(T)], dim=1).cpu().numpy()
    err = float(np.abs(q - q64).max())
    print(f"  trained MAC: max |q - q64| {err:.3e} (bound {Q_TOL:.1e})")
    assert err <= Q_TOL
    path = str(tmp_path / "ckpt")
    os.makedirs(path)
    learner.save_models(path, learner.name)
    assert sorted(os.listdir(path)) == ["home_qlearner_agent.th", "home_qlearner_mixer.th", "home_qlearner_opt.th"]
    sd = torch.load(os.path.join(path, "home_qlearner_agent.th"), weights_only=True)
    assert list(sd) == dqn_ref.AGENT_KEYS
    mac2 = BasicMAC(exp.home_buffer.scheme, exp.groups, exp.args)
    fresh = QLearner(mac2, exp.home_buffer.scheme, MainLogger(log_interval=10 ** 12), exp.args, name="home")
    fresh.build_optimizer()
    fresh.load_models(path)
    assert torch.equal(fresh._flat.flat, learner._flat.flat) and torch.equal(fresh._sq, learner._sq)
    exp.stepper.close_env()
