"""GPU parity of the fused learner (mlg_qlearner_train) for the mixer cases beyond the default shape: IQL (no mixer),
one-layer hypernetworks and the other QMixer widths, against the CPU oracle (oracle/learner_ref.py), goldens of the
reference QLearner, MLG_LEARNER_FULL=1 and the autograd ops.

Tolerances are those of tests/test_gpu_learner.py: against a reference golden statistics rtol 1e-4 / atol 1e-6 and
parameters atol 2e-5; against the oracle statistics rtol 2e-4 / atol 1e-6 and parameters atol 5e-5. ORACLE_F64 lists,
per oracle case, how far the fp32 oracle itself is from a float64 run of the same oracle (measured on the CPU, the
figures are also in profiles/learner_shapes/README.md); where ten times that distance exceeds the bound above, the
case's bound is ten times that distance.
"""
import copy
import os

import numpy as np
import pytest
import torch

import learner_ref as LR
from helpers import qmix_args, scheme_for

pytestmark = pytest.mark.gpu

STAT_KEYS = ["loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean"]
CALLS = [(0, 0), (0, 100), (0, 200)]  # target == online; stale target; stale target, ends with the sync
MIXER_SEED = 11

# kw on top of qmix_args() per case
TRAJ = {
    "iql-dq": dict(mixer=None),
    "iql-nodq": dict(mixer=None, double_q=False),
    "h1-e32": dict(hypernet_layers=1),
    "h1-e64": dict(hypernet_layers=1, mixing_embed_dim=64),
    "h2-e16-he32": dict(mixing_embed_dim=16, hypernet_embed=32),
    "h2-e64-he128": dict(mixing_embed_dim=64, hypernet_embed=128),
    "h2-e32-he128": dict(mixing_embed_dim=32, hypernet_embed=128),
    "h2-e16-he64": dict(mixing_embed_dim=16, hypernet_embed=64),
}
WIDE = dict(n_agents=9, n_actions=17, state_shape=50, rnn_hidden_dim=32)
WIDE_CASES = {
    "iql": dict(mixer=None, **WIDE),
    "h1-e16": dict(hypernet_layers=1, mixing_embed_dim=16, **WIDE),
    "h2-e64-he128": dict(mixing_embed_dim=64, hypernet_embed=128, **WIDE),
}
# case -> (largest relative distance of a statistic, largest absolute distance of a parameter) between the fp32
# oracle and the same oracle in float64, after the case's calls (scripts/oracle_f64_distance.py, on the CPU). Ten times
# any of them is below the usual bounds, so every case keeps those: the one-layer hypernets' large gradients (norms of
# 80 to 840 before clipping) do not loosen anything.
ORACLE_F64 = {
    "iql-dq": (5.57e-06, 1.87e-07),  # largest grad_norm 0.4475
    "iql-nodq": (3.94e-07, 2.08e-07),  # largest grad_norm 0.4475
    "h1-e32": (1.53e-06, 5.12e-07),  # largest grad_norm 268
    "h1-e64": (5.85e-07, 1.40e-06),  # largest grad_norm 841.6
    "h2-e16-he32": (2.49e-06, 1.14e-06),  # largest grad_norm 10.08
    "h2-e64-he128": (4.39e-07, 1.04e-06),  # largest grad_norm 73.75
    "h2-e32-he128": (5.96e-07, 8.91e-07),  # largest grad_norm 25
    "h2-e16-he64": (3.84e-07, 1.07e-06),  # largest grad_norm 8.794
    "wide-iql": (1.58e-07, 6.10e-08),  # largest grad_norm 0.3478
    "wide-h1-e16": (1.53e-07, 7.39e-07),  # largest grad_norm 80.37
    "wide-h2-e64-he128": (4.59e-08, 1.10e-06),  # largest grad_norm 90.81
}


def _bounds(case):
    """(stat rtol, param atol) against the oracle: the defaults, or ten times the oracle's own fp32 error."""
    s, p = ORACLE_F64.get(case, (0.0, 0.0))
    return max(2e-4, 10 * s), max(5e-5, 10 * p)


class _Log:
    def __init__(self):
        self.stats = {}

    def log_stat(self, k, v, t):
        self.stats[k] = v

    def info(self, *a):
        pass


def mixer_state(args, seed=MIXER_SEED):
    """QMixer weights under a fixed seed, built on the CPU (state_dict of CPU tensors)."""
    from maleague.modules.mixers import QMixer
    torch.manual_seed(seed)
    return {k: v.detach().clone() for k, v in QMixer(LR.clone_args(args, device="cpu")).state_dict().items()}


def agent_state(args, d_obs, seed=3):
    from maleague.modules.agents.drqn_agent import DRQNAgentNetwork
    torch.manual_seed(seed)
    d_in = d_obs + (args.n_actions if args.obs_last_action else 0) + (args.n_agents if args.obs_agent_id else 0)
    return {k: v.detach().clone() for k, v in DRQNAgentNetwork(d_in, LR.clone_args(args, device="cpu")).state_dict().items()}


def _episode_batch(tb, device):
    from maleague.components.episode_batch import EpisodeBatch
    B, T, N, _ = tb["obs"].shape
    info = {"state_shape": tb["state"].shape[-1], "obs_shape": tb["obs"].shape[-1],
            "n_actions": tb["avail_actions"].shape[-1], "n_agents": N}
    scheme, groups, preprocess = scheme_for(info, torch)
    eb = EpisodeBatch(scheme, groups, B, T, preprocess=preprocess, device=device)
    for k, v in tb.items():
        eb.data.transition_data[k].copy_(v)
    return eb


def _learner(eb, agent0, mixer0, args):
    from maleague.controllers import BasicMAC
    from maleague.learners import QLearner
    mac = BasicMAC(eb.scheme, eb.groups, args)
    mac.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in agent0.items()})
    log = _Log()
    learner = QLearner(mac, eb.scheme, log, args, name="home")
    if args.mixer == "qmix":
        msd = {k: torch.as_tensor(np.asarray(v)) for k, v in mixer0.items()}
        learner.mixer.load_state_dict(msd)
        learner.target_mixer.load_state_dict(msd)
    learner.build_optimizer()
    return learner, log


def _golden_agent(d):
    return {k[len("p0.agent."):]: np.array(d[k]) for k in d.files if k.startswith("p0.agent.")}


def wide_batch():
    """Test 6's synthetic batch (CPU tensors, scheme dtypes): B=3, T=6, N=9, A=17, S=50, d_obs=23; filled prefixes
    of 5, 3 and 2 steps, `terminated` on the last filled step of the first two episodes; every agent has an available
    action and takes one. The contents are random at every step, filled or not: nothing past an episode's end may
    reach a result. max_t_filled is 5, so the learner trains on transitions 0..3 (WIDE_T)."""
    rs = np.random.RandomState(21)
    B, T, N, A, S, d_obs = 3, 6, WIDE["n_agents"], WIDE["n_actions"], WIDE["state_shape"], 23
    lens = [5, 3, 2]
    filled = np.zeros((B, T, 1), np.int64)
    term = np.zeros((B, T, 1), np.uint8)
    for b, f in enumerate(lens):
        filled[b, :f] = 1
    term[0, lens[0] - 1] = 1
    term[1, lens[1] - 1] = 1
    avail = (rs.rand(B, T, N, A) < 0.5).astype(np.int32)
    avail[..., 3] = 1
    actions = np.zeros((B, T, N, 1), np.int64)
    for idx in np.ndindex(B, T, N):
        actions[idx][0] = rs.choice(np.flatnonzero(avail[idx]))
    onehot = np.zeros((B, T, N, A), np.float32)
    np.put_along_axis(onehot, actions, 1.0, axis=-1)
    out = {"state": rs.randn(B, T, S).astype(np.float32), "obs": rs.randn(B, T, N, d_obs).astype(np.float32),
           "actions": actions, "avail_actions": avail, "reward": rs.randn(B, T, 1).astype(np.float32),
           "terminated": term, "actions_onehot": onehot, "filled": filled}
    return {k: torch.from_numpy(v) for k, v in out.items()}


WIDE_T = 5  # max_t_filled of wide_batch(): the reference trains on sample[:, :max_t_filled] (ma_experiment.py:236-238)


def wide_oracle_batch(tb):
    return {k: v[:, :WIDE_T].clone() for k, v in tb.items()}


def _compare_to_oracle(case, learner, ref, args, what=""):
    rtol, atol = _bounds(case)
    pairs = [("agent", learner.mac.agent.state_dict(), ref.agent_state()),
             ("target agent", learner.target_mac.agent.state_dict(), ref.tp)]
    if args.mixer == "qmix":
        pairs += [("mixer", learner.mixer.state_dict(), ref.mixer_state()),
                  ("target mixer", learner.target_mixer.state_dict(), ref.tmp)]
    worst = 0.0
    for name, got, want in pairs:
        assert list(got.keys()) == list(want.keys())
        for k, v in got.items():
            worst = max(worst, float(np.abs(v.cpu().numpy() - want[k].detach().numpy()).max()))
    print(f"  {case}{what}: max parameter error {worst:.3e} (bound {atol:.1e})")
    for name, got, want in pairs:
        for k, v in got.items():
            np.testing.assert_allclose(v.cpu().numpy(), want[k].detach().numpy(), atol=atol, rtol=0,
                                       err_msg=f"{case} {name} {k}")


def _compare_stats(case, i, got, want):
    rtol, _ = _bounds(case)
    print(f"  {case} call {i}: " + ", ".join(f"{k} {got[k]:.7g}/{want[k]:.7g}" for k in STAT_KEYS))
    for k in STAT_KEYS:
        assert np.isfinite(got[k]), f"{case} call {i} {k}"
        np.testing.assert_allclose(got[k], want[k], rtol=rtol, atol=1e-6, err_msg=f"{case} call {i} {k}")


# ---- 4. three-call trajectories against the oracle on the committed batch ------------------------------------------
@pytest.mark.parametrize("case", list(TRAJ))
def test_three_call_trajectory_vs_oracle(device, golden, case):
    """B=4, T=7, N=5, A=15, S=60: 24 mixer rows, two 16-row tiles, the second partial."""
    d = golden("qlearner_qmix_dq.npz")
    args = qmix_args(**TRAJ[case])
    agent0 = _golden_agent(d)
    mixer0 = mixer_state(args) if args.mixer == "qmix" else None
    tb = LR.batch_from_npz(d)
    eb = _episode_batch(tb, device)
    learner, _ = _learner(eb, agent0, mixer0, args)
    ref = LR.QLearnerRef(agent0, mixer0, copy.copy(args))
    for i, (t_env, ep) in enumerate(CALLS):
        want = ref.train({k: v.clone() for k, v in tb.items()}, t_env, ep)
        learner.train(eb, t_env, ep)
        _compare_stats(case, i, learner.last_stats, want)
    assert learner.last_target_update_episode == ref.last_target_update_episode == 200
    _compare_to_oracle(case, learner, ref, args)
    assert learner.mac.agent.trained_steps == ref.trained_steps
    if args.mixer is None:  # the mask expanded over the agents
        m = tb["filled"][:, :-1].float()
        m[:, 1:] *= 1 - tb["terminated"][:, :-2].float()
        n = float(m.sum()) * args.n_agents
        assert float(learner._stats[5]) == n and float(learner._stats[6]) == n
        assert ref.trained_steps == len(CALLS) * int(n)


# ---- 5. goldens of the reference QLearner ------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("qlearner_qmix_h1.npz", {"hypernet_layers": 1}),
                                     ("qlearner_qmix_e64_he128.npz", {"mixing_embed_dim": 64, "hypernet_embed": 128})])
def test_qlearner_shapes_golden(device, golden, name, kw):
    d = golden(name)
    args = qmix_args(**kw)
    mixer0 = {k[len("p0.mixer."):]: np.array(d[k]) for k in d.files if k.startswith("p0.mixer.")}
    eb = _episode_batch(LR.batch_from_npz(d), device)
    learner, log = _learner(eb, _golden_agent(d), mixer0, args)
    for i, (t_env, ep) in enumerate(d["calls"]):
        learner.train(eb, int(t_env), int(ep))
        want = {k: float(d[f"stat{i}.{k}"]) for k in STAT_KEYS}
        print(f"  {name} call {i}: " + ", ".join(f"{k} {learner.last_stats[k]:.7g}/{want[k]:.7g}" for k in STAT_KEYS))
        for k in STAT_KEYS:
            np.testing.assert_allclose(learner.last_stats[k], float(d[f"stat{i}.{k}"]), rtol=1e-4, atol=1e-6,
                                       err_msg=f"{name} call {i} {k}")
        assert log.stats["home_qlearner_loss"] == learner.last_stats["loss"]
    last = len(d["calls"])
    for k, v in learner.mac.agent.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), d[f"p{last}.agent.{k}"], atol=2e-5, rtol=0, err_msg=k)
    for k, v in learner.target_mac.agent.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), d[f"p{last}.target_agent.{k}"], atol=2e-5, rtol=0, err_msg=k)
    for k, v in learner.mixer.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), d[f"p{last}.mixer.{k}"], atol=2e-5, rtol=0, err_msg=k)
    assert learner.mac.agent.trained_steps == int(d["trained_steps"])


# ---- 6. beyond the prefetching bounds -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    tb = wide_batch()
    assert tb["filled"].sum(dim=(1, 2)).tolist() == [5, 3, 2]
    assert bool((tb["avail_actions"].sum(-1) > 0).all())
    assert bool((torch.gather(tb["avail_actions"], 3, tb["actions"]) == 1).all())
    return tb


@pytest.mark.parametrize("case", list(WIDE_CASES))
def test_wide_shapes_vs_oracle(device, wide, case):
    """N = 9 > 8 and A = 17 > 16 (the generic gather, two action tiles), S = 50 (no multiple of 16), H = 32 (the
    non-fused backward launch), episodes of unequal length."""
    args = qmix_args(**WIDE_CASES[case])
    agent0 = agent_state(args, wide["obs"].shape[-1])
    mixer0 = mixer_state(args) if args.mixer == "qmix" else None
    eb = _episode_batch(wide, device)
    learner, _ = _learner(eb, agent0, mixer0, args)
    ref = LR.QLearnerRef(agent0, mixer0, copy.copy(args))
    assert int(eb.max_t_filled()) == WIDE_T
    want = ref.train(wide_oracle_batch(wide), 0, 0)
    learner.train(eb, 0, 0)
    _compare_stats("wide-" + case, 0, learner.last_stats, want)
    _compare_to_oracle("wide-" + case, learner, ref, args)
    assert learner.mac.agent.trained_steps == ref.trained_steps


# ---- 7. skip equivalence --------------------------------------------------------------------------------------------
def _snapshots(device, wide, args, monkeypatch, full):
    if full:
        monkeypatch.setenv("MLG_LEARNER_FULL", "1")
    else:
        monkeypatch.delenv("MLG_LEARNER_FULL", raising=False)
    agent0 = agent_state(args, wide["obs"].shape[-1])
    mixer0 = mixer_state(args) if args.mixer == "qmix" else None
    eb = _episode_batch(wide, device)
    learner, _ = _learner(eb, agent0, mixer0, args)
    out = []
    for i, ep in enumerate([0, 200, 200]):  # target a copy, stale (then synced), a copy again
        if not full:  # no kernel may read a workspace element that the call did not write
            if learner._ws is not None:
                learner._ws.fill_(float("nan"))
        learner.train(eb, i, ep)
        torch.cuda.synchronize()
        out.append({"stats": learner._stats.cpu().numpy().copy(), "grads": learner._grads.cpu().numpy().copy(),
                    "params": learner._flat.flat.cpu().numpy().copy(), "sq": learner._sq.cpu().numpy().copy()})
    monkeypatch.delenv("MLG_LEARNER_FULL", raising=False)
    return out


@pytest.mark.parametrize("case", ["iql", "h1-e16"])
def test_skip_path_equals_full_path(device, wide, monkeypatch, case):
    args = qmix_args(**WIDE_CASES[case])
    got = _snapshots(device, wide, args, monkeypatch, False)
    want = _snapshots(device, wide, args, monkeypatch, True)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.all(np.isfinite(g["stats"])), f"call {i}: stats {g['stats']}"
        assert np.array_equal(g["stats"][:7], w["stats"][:7]), f"call {i}: {g['stats']} vs {w['stats']}"
        for k in ("grads", "params", "sq"):
            assert np.array_equal(g[k], w[k]), f"call {i}: {k} differ at {np.flatnonzero(g[k] != w[k])[:8]}"
    assert got[0]["stats"][7] < want[0]["stats"][7]  # the default path planned fewer forward blocks


# ---- 8. two implementations agree -----------------------------------------------------------------------------------
def test_one_layer_gradients_match_autograd_ops(device, golden):
    """The fused learner's gradient for layers 1, E = 32 on the golden batch (learner._grads scaled back by the clip
    factor) against loss.backward() over mac.forward / QMixer.forward with enable_autograd(), targets under no_grad:
    per tensor within test_gpu_autograd.py's bound, max|g - g_ref| <= 1e-4 * max(1, max|g_ref|)."""
    from maleague.controllers import BasicMAC
    from maleague.modules.mixers import QMixer
    from test_gpu_autograd import _check, td_loss
    d = golden("qlearner_qmix_dq.npz")
    args = qmix_args(hypernet_layers=1)
    agent0, mixer0 = _golden_agent(d), mixer_state(args)
    tb = LR.batch_from_npz(d)
    eb = _episode_batch(tb, device)
    learner, _ = _learner(eb, agent0, mixer0, args)
    learner.train(eb, 0, 0)
    norm = float(learner._stats[1])
    coef = min(1.0, args.grad_norm_clip / (norm + 1e-6))  # clip_grad_norm_
    assert norm > args.grad_norm_clip, "the case is meant to clip"

    mac = BasicMAC(eb.scheme, eb.groups, args)
    mac.load_state_dict({k: torch.from_numpy(v) for k, v in agent0.items()})
    mac.enable_autograd()
    target_mac = copy.deepcopy(mac)
    mx = QMixer(args)
    mx.load_state_dict(mixer0)
    mx.enable_autograd()
    target_mx = copy.deepcopy(mx)

    def unroll(online):
        m = mac if online else target_mac
        m.init_hidden(eb.batch_size)
        return torch.stack([m.forward(eb, t) for t in range(eb.max_seq_length)], dim=1)

    def mix(online, qs, states):
        return (mx if online else target_mx)(qs, states)

    loss = td_loss(unroll, mix, {k: eb[k] for k in ("reward", "actions", "terminated", "filled", "avail_actions",
                                                    "state")}, args)
    loss.backward()
    np.testing.assert_allclose(float(loss.detach()), learner.last_stats["loss"], rtol=1e-4)
    params = list(mac.parameters()) + list(mx.parameters())
    assert len(params) == len(learner._flat.views)
    print("fused learner (unclipped) vs autograd ops, one-layer hypernets")
    for (q, off, k), mine in zip(learner._flat.views, params):
        fused = learner._grads[off:off + k].view_as(q).cpu().to(torch.float64) / coef
        _check(f"param {off}", fused, mine.grad.detach().cpu().to(torch.float64))


# ---- 9. end to end ----------------------------------------------------------------------------------------------------
def test_iql_end_to_end(device, tmp_path):
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.learners import QLearner
    from maleague.runs import MultiAgentExperiment
    from maleague.utils.config import build_config, to_args
    cfg = build_config("iql", "ma", overrides=["runner=parallel", "batch_size_run=8", "batch_size=8",
                                               "buffer_cpu_only=False", "buffer_size=16", "env_args.episode_limit=20",
                                               "seed=0", "show_exp_parameters=False", "t_max=1000000",
                                               "test_interval=100000000", f"local_results_path={tmp_path}"])
    np.random.seed(0)
    torch.manual_seed(0)
    exp = MultiAgentExperiment(to_args(cfg), MainLogger(log_interval=10 ** 12))
    learner = exp.home_learner
    assert type(learner) is QLearner and learner.mixer is None
    exp._init_stepper()
    for i in range(2):
        exp._train_episode(i * 8)
    assert learner.train_calls == 2
    stats = learner.last_stats
    assert np.isfinite(stats["loss"]) and np.isfinite(stats["grad_norm"])
    assert learner.mac.agent.trained_steps > 0
    path = str(tmp_path / "ckpt")
    os.makedirs(path)
    learner.save_models(path, learner.name)
    assert sorted(os.listdir(path)) == ["home_qlearner_agent.th", "home_qlearner_opt.th"]
    mac2 = BasicMAC(exp.home_buffer.scheme, exp.groups, exp.args)
    fresh = QLearner(mac2, exp.home_buffer.scheme, MainLogger(log_interval=10 ** 12), exp.args, name="home")
    fresh.build_optimizer()
    assert not torch.equal(fresh._flat.flat, learner._flat.flat)
    fresh.load_models(path)
    assert torch.equal(fresh._flat.flat, learner._flat.flat)
    assert torch.equal(fresh._tflat.flat, learner._flat.flat)  # target nets are not saved: they take the online file
    assert torch.equal(fresh._sq, learner._sq) and float(fresh._sq.abs().sum()) > 0
    assert float(fresh._step) == float(learner._step) == 2.0
    exp.stepper.close_env()
