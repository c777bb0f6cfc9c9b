"""GPU parity of QLearner with a DistinctMAC (the unrolled branch, learners/q_learner.py): first-call gradients per
agent and tensor against the float64 restatement, three-call trajectories against the fp32 one
(tests/distinct_ref.py's DistinctLearnerRef), rollout then training, and a MultiAgentExperiment end to end.

Batches are learner_arm_shapes.arm_batch's (B = 5, filled prefixes 6 / 5 / 3 / 2 / 2 of 8 stored steps, terminated
flags on three episodes); the learner unrolls over all 8 stored steps, the oracle trains on the copy truncated to
max_t_filled (the masked steps reach nothing). Tolerances are tests/learner_arm_shapes.py's, the ones
tests/test_gpu_learner_arms.py applies: statistics rtol 2e-4 / atol 1e-6, parameters atol 5e-5, gradients 1e-4 of the
float64 tensor's largest element.
"""
import functools
import os

import numpy as np
import pytest
import torch

import distinct_ref as DR
import helpers
import learner_arm_shapes as LA
import learner_ref as LR
from helpers import qmix_args, scheme_for
from test_gpu_learner_shapes import STAT_KEYS, _episode_batch, _Log, mixer_state

pytestmark = pytest.mark.gpu

F64 = torch.float64
D_OBS, A, S = 48, 11, 36
# (id, N, H, mixer kwargs)
CASES = [("qmix-n3-h64", 3, 64, LA.QMIX), ("qmix-n1-h32", 1, 32, LA.QMIX), ("qmix-n5-h32", 5, 32, LA.QMIX),
         ("vdn-n5-h64", 5, 64, LA.VDN), ("vdn-n3-h32", 3, 32, LA.VDN), ("iql-n3-h32", 3, 32, LA.IQL),
         ("iql-n1-h64", 1, 64, LA.IQL)]
IDS = [c[0] for c in CASES]
SEED = 11


def _args(N, H, mixer, device="cuda"):
    return qmix_args(n_agents=N, n_actions=A, state_shape=S, rnn_hidden_dim=H, obs_agent_id=False, mac="distinct",
                     device=device, **mixer)


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    _, N, H, mixer = next(c for c in CASES if c[0] == cid)
    args = _args(N, H, mixer)
    agents0 = DR.all_agent_params(N, D_OBS + A, H, A, SEED)
    mixer0 = mixer_state(args, seed=SEED + 8) if args.mixer == "qmix" else None
    tb = LA.arm_batch(N, A, S, D_OBS, seed=SEED + 100)
    return args, agents0, mixer0, tb


@functools.lru_cache(maxsize=None)
def _oracle(cid):
    """Once per case: the fp32 oracle's three calls and the float64 oracle's first call (gradients before the clip,
    agent 0's tensors first, then the mixer's)."""
    args, agents0, mixer0, tb = _inputs(cid)
    ob = LA.oracle_batch(tb)
    ref = DR.learner_ref(agents0, mixer0, LR.clone_args(args, device="cpu"))
    stats = [ref.train({k: v.clone() for k, v in ob.items()}, t_env, ep) for t_env, ep in LA.CALLS]
    ref64 = DR.learner_ref(agents0, mixer0, LR.clone_args(args, device="cpu"), dtype=F64)
    s64 = ref64.train({k: v.clone() for k, v in ob.items()}, *LA.CALLS[0])
    return stats, ref, [g.clone() for g in ref64.last_grads], s64


def _learner(device, args, agents0, mixer0):
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import DistinctMAC
    from maleague.learners import QLearner
    info = {"state_shape": S, "obs_shape": D_OBS, "n_actions": A, "n_agents": args.n_agents}
    scheme, groups, preprocess = scheme_for(info, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    mac = DistinctMAC(proto.scheme, groups, args)
    DR.load_agents(mac, agents0)
    log = _Log()
    learner = QLearner(mac, proto.scheme, log, args, name="home")
    if args.mixer == "qmix":
        msd = {k: torch.as_tensor(np.asarray(v)) for k, v in mixer0.items()}
        learner.mixer.load_state_dict(msd)
        learner.target_mixer.load_state_dict(msd)
    learner.build_optimizer()
    return learner, log


_RUNS = {}


def _run(cid, device):
    """A fresh learner's three calls, shared by the tests of a case: statistics per call, the first call's
    gradients (as left in .grad: after the clip) and grad_norm."""
    if cid in _RUNS:
        return _RUNS[cid]
    args, agents0, mixer0, tb = _inputs(cid)
    eb = _episode_batch(tb, device)
    assert eb.max_seq_length == LA.T_STORED and int(eb.max_t_filled()) == LA.T_FILLED
    learner, log = _learner(device, args, agents0, mixer0)
    out = {"stats": [], "learner": learner, "log": log}
    for i, (t_env, ep) in enumerate(LA.CALLS):
        learner.train(eb, t_env, ep)
        out["stats"].append(dict(learner.last_stats))
        if i == 0:
            out["grads0"] = [p.grad.detach().cpu().clone() for p in learner.parameters()]
    _RUNS[cid] = out
    return out


@pytest.mark.parametrize("cid", IDS)
def test_first_call_gradients_vs_float64_oracle(device, cid):
    """.grad after the first call, scaled back by the factor clip_grad_norm_ applied (from the call's own grad_norm),
    per agent and tensor against the float64 oracle's .grad before its clip."""
    args, _, _, _ = _inputs(cid)
    _, _, g64, s64 = _oracle(cid)
    got = _run(cid, device)
    norm = got["stats"][0]["grad_norm"]
    np.testing.assert_allclose(norm, s64["grad_norm"], rtol=LA.STAT_RTOL)
    coef = min(1.0, args.grad_norm_clip / (norm + 1e-6))  # clip_grad_norm_
    params = got["learner"].parameters()
    assert len(g64) == len(params) == len(got["grads0"]) and len(params) >= 8 * args.n_agents
    worst = 0.0
    for j, (p, mine, ref) in enumerate(zip(params, got["grads0"], g64)):
        assert tuple(p.shape) == tuple(ref.shape)
        err, scale = float((mine.to(F64) / coef - ref).abs().max()), float(ref.abs().max())
        worst = max(worst, err / scale)
        who = f"agent {j // 8} {DR.AGENT_KEYS[j % 8]}" if j < 8 * args.n_agents else f"mixer tensor {j - 8 * args.n_agents}"
        assert err <= LA.GRAD_RTOL * scale, f"{cid} {who}: max error {err:.3e} > {LA.GRAD_RTOL * scale:.3e}"
    print(f"  {cid}: grad_norm {norm:.6g} (clip factor {coef:.4g}), largest gradient error / bound "
          f"{100 * worst / LA.GRAD_RTOL:.2f} %")


@pytest.mark.parametrize("cid", IDS)
def test_three_call_trajectory_vs_oracle(device, cid):
    """Target equal to online, stale, then stale ending with the sync, against the fp32 oracle: statistics, the N
    networks, their targets, the mixer and its target; the logger received the reference's stat keys."""
    args, _, _, tb = _inputs(cid)
    want, ref, _, _ = _oracle(cid)
    got = _run(cid, device)
    learner = got["learner"]
    for i in range(len(LA.CALLS)):
        print(f"  {cid} call {i}: " + ", ".join(f"{k} {got['stats'][i][k]:.7g}/{want[i][k]:.7g}" for k in STAT_KEYS))
        for k in STAT_KEYS:
            assert np.isfinite(got["stats"][i][k]), f"{cid} call {i} {k}"
            np.testing.assert_allclose(got["stats"][i][k], want[i][k], rtol=LA.STAT_RTOL, atol=LA.STAT_ATOL,
                                       err_msg=f"{cid} call {i} {k}")
    assert set(got["log"].stats) == {"home_qlearner_" + k for k in STAT_KEYS}
    assert learner.last_target_update_episode == ref.last_target_update_episode == 200
    pairs = []
    for i in range(args.n_agents):
        pairs.append((f"agent {i}", learner.mac.agents[i].state_dict(), ref.agent_states()[i]))
        pairs.append((f"target agent {i}", learner.target_mac.agents[i].state_dict(), ref.target_states()[i]))
    if args.mixer == "qmix":
        pairs += [("mixer", learner.mixer.state_dict(), ref.mixer_state()),
                  ("target mixer", learner.target_mixer.state_dict(), ref.tmp)]
    errs = {}
    for name, g, w in pairs:
        assert list(g.keys()) == list(w.keys())
        for k, v in g.items():
            errs[f"{name} {k}"] = float(np.abs(v.cpu().numpy() - w[k].detach().numpy()).max())
    worst = max(errs, key=errs.get)
    print(f"  {cid}: max parameter error {errs[worst]:.3e} at {worst} (bound {LA.PARAM_ATOL:.1e}, "
          f"{100 * errs[worst] / LA.PARAM_ATOL:.2f} %)")
    for k, e in errs.items():
        assert e <= LA.PARAM_ATOL, f"{cid} {k}: {e:.3e} > {LA.PARAM_ATOL:.1e}"
    for a, t in zip(learner.mac.agents, learner.target_mac.agents):  # the third call ended with the sync
        assert all(torch.equal(v, t.state_dict()[k]) for k, v in a.state_dict().items())
    n = LA.mask_sum(tb) * (args.n_agents if args.mixer is None else 1)  # IQL expands the mask over the agents
    assert [a.trained_steps for a in learner.mac.agents] == [ref.trained_steps] * args.n_agents
    assert ref.trained_steps == len(LA.CALLS) * int(n)


@pytest.mark.parametrize("mixer", [LA.VDN, LA.QMIX, LA.IQL], ids=["vdn", "qmix", "iql"])
def test_dead_agent_slot_gradient(device, mixer):
    """An agent slot that is dead in every stored step (a zero observation, only the no-op available and taken) gets
    an exactly zero gradient in every tensor of its network, and the step leaves that network's parameters bit for
    bit where they were. The slot's chosen Q keeps its value in the mix: loss, td_error_abs, q_taken_mean and
    target_mean are the reference arithmetic's, and the other slots' gradients are the float64 restatement's within
    1e-4 of each tensor's largest element. (The reference's arithmetic itself would move the dead slot's network: at
    N = 3, H = 32, VDN, slot 1 dead, the float64 restatement gives its tensors max|grad| 4.3e-2 .. 5.2e-1; the learner
    cuts that path, DESIGN.md §7. grad_norm is therefore the norm without the dead slot's share.)"""
    N, H, dead = 3, 32, 1
    args = _args(N, H, mixer)
    agents0 = DR.all_agent_params(N, D_OBS + A, H, A, SEED)
    mixer0 = mixer_state(args, seed=SEED + 8) if args.mixer == "qmix" else None
    tb = LA.arm_batch(N, A, S, D_OBS, seed=SEED + 100)
    tb["obs"][:, :, dead] = 0
    tb["avail_actions"][:, :, dead] = 0
    tb["avail_actions"][:, :, dead, 0] = 1
    tb["actions"][:, :, dead] = 0
    tb["actions_onehot"][:, :, dead] = 0
    tb["actions_onehot"][:, :, dead, 0] = 1
    ref64 = DR.learner_ref(agents0, mixer0, LR.clone_args(args, device="cpu"), dtype=F64)
    want = ref64.train({k: v.clone() for k, v in LA.oracle_batch(tb).items()}, 0, 0)
    learner, _ = _learner(device, args, agents0, mixer0)
    before = [p.detach().clone() for p in learner.mac.agents[dead].parameters()]
    learner.train(_episode_batch(tb, device), 0, 0)
    for k in ("loss", "td_error_abs", "q_taken_mean", "target_mean"):
        np.testing.assert_allclose(learner.last_stats[k], want[k], rtol=LA.STAT_RTOL, atol=LA.STAT_ATOL, err_msg=k)
    g64 = ref64.last_grads
    print("  dead slot, float64 max|grad| per tensor:",
          [f"{float(g.abs().max()):.3e}" for g in g64[8 * dead:8 * dead + 8]])
    for p, p0 in zip(learner.mac.agents[dead].parameters(), before):
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0
        assert torch.equal(p.detach(), p0)
    live64 = [g for j, g in enumerate(g64) if j // 8 != dead]
    live = [p.grad for j, p in enumerate(learner.parameters()) if j // 8 != dead]
    norm64 = float(torch.sqrt(sum((g ** 2).sum() for g in live64)))
    np.testing.assert_allclose(learner.last_stats["grad_norm"], norm64, rtol=LA.STAT_RTOL)
    coef = min(1.0, args.grad_norm_clip / (norm64 + 1e-6))
    for mine, ref in zip(live, live64):
        err, scale = float((mine.detach().cpu().to(F64) / coef - ref).abs().max()), float(ref.abs().max())
        assert err <= LA.GRAD_RTOL * scale, (err, scale)
    for i in (0, 2):  # the live networks moved
        assert not torch.equal(learner.mac.agents[i].fc2.bias.detach().cpu(), torch.from_numpy(agents0[i]["fc2.bias"]))


# ---- rollout, then training, then the next rollout ------------------------------------------------------------------

def test_rollout_then_training_then_rollout(device, monkeypatch):
    """3v3, 8 envs: the learner trains on the rollout's own batch (statistics and stepped networks against the fp32
    oracle on the copy truncated to max_t_filled), and the trained weights drive the next rollout: the pool is
    repacked from the learner's flat buffer in one launch and the float64 oracle with the stepped parameters matches
    every pick again."""
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import DistinctMAC
    from maleague.custom_logging import MainLogger
    from maleague.learners import QLearner
    from maleague.steppers import ParallelStepper
    from maleague.utils.flat import flat_view
    monkeypatch.setattr(helpers, "oracle_q", DR.oracle_q)
    B, seed = 8, 3
    args = qmix_args(batch_size_run=B, seed=seed, obs_agent_id=False, mac="distinct",
                     env_args={"match_build_plan": "small", "grid_size": 20, "stochastic_spawns": True,
                               "episode_limit": 20})
    stepper = ParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"], info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(info, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    mac = DistinctMAC(proto.scheme, groups, args)
    agents0 = DR.all_agent_params(args.n_agents, mac.input_shape, 64, args.n_actions, seed)
    DR.load_agents(mac, agents0)
    learner = QLearner(mac, proto.scheme, _Log(), args, name="home")
    mixer0 = {k: v.detach().cpu().clone() for k, v in learner.mixer.state_dict().items()}
    learner.build_optimizer()
    assert flat_view(mac.parameters()) is not None  # back to back: one mlg_pack_agent_pool launch per repack
    stepper.initialize(scheme, groups, preprocess, mac)
    stepper.t_env = 30000
    batch, infos = stepper.run(test_mode=False)
    eps = mac.action_selector.epsilon
    helpers.check_run(stepper, mac, args, batch, infos, episode=0, test_mode=False, eps=eps, dtype=F64)
    T = int(batch.max_t_filled())
    tb = {k: v[:, :T].detach().cpu().clone() for k, v in batch.data.transition_data.items()}
    ref = DR.learner_ref(agents0, mixer0, LR.clone_args(args, device="cpu"))
    want = ref.train({k: v.clone() for k, v in tb.items()}, 30000, 0)
    pool_before = mac.packed().clone()
    learner.train(batch, 30000, 0)
    print(f"  T={T}: " + ", ".join(f"{k} {learner.last_stats[k]:.7g}/{want[k]:.7g}" for k in STAT_KEYS))
    for k in STAT_KEYS:
        np.testing.assert_allclose(learner.last_stats[k], want[k], rtol=LA.STAT_RTOL, atol=LA.STAT_ATOL, err_msg=k)
    for i, a in enumerate(mac.agents):
        for k, v in a.state_dict().items():
            np.testing.assert_allclose(v.cpu().numpy(), ref.agent_states()[i][k].numpy(), atol=LA.PARAM_ATOL, rtol=0,
                                       err_msg=f"agent {i} {k}")
    assert not torch.equal(mac.packed(), pool_before)
    batch, infos = stepper.run(test_mode=True)
    helpers.check_run(stepper, mac, args, batch, infos, episode=1, test_mode=True, eps=0.0, dtype=F64)


# ---- end to end ---------------------------------------------------------------------------------------------------

def test_experiment_end_to_end(device, tmp_path):
    """MultiAgentExperiment with mac=distinct on the small plan: a few iterations with training, a checkpoint with
    the per-agent file names, reloaded into a fresh MAC with equal Q."""
    from maleague.controllers import DistinctMAC
    from maleague.custom_logging import MainLogger
    from maleague.runs import MultiAgentExperiment
    from maleague.utils.config import build_config, to_args
    cfg = build_config("qmix", "ma", overrides=["mac=distinct", "obs_agent_id=False", "runner=parallel",
                                                "batch_size_run=8", "batch_size=8", "buffer_cpu_only=False",
                                                "buffer_size=16", "env_args.episode_limit=20",
                                                "env_args.match_build_plan=small", "seed=0",
                                                "show_exp_parameters=False", "t_max=1000000",
                                                "test_interval=100000000", f"local_results_path={tmp_path}"])
    np.random.seed(0)
    torch.manual_seed(0)
    exp = MultiAgentExperiment(to_args(cfg), MainLogger(log_interval=10 ** 12))
    assert isinstance(exp.home_mac, DistinctMAC) and exp.home_learner.mixer is not None
    exp._init_stepper()
    assert exp.stepper.describe_rollout()[0] == "dx-global/tpw1"
    for i in range(3):
        exp._train_episode(i * 8)
    exp.stepper.flush()
    assert exp.home_learner.train_calls == 3
    for v in exp.home_learner.last_stats.values():
        assert np.isfinite(v)
    assert exp.home_mac.agents[2].trained_steps > 0
    path = str(tmp_path / "ckpt")
    os.makedirs(path)
    exp.home_learner.save_models(path, exp.home_learner.name)
    names = sorted(os.listdir(path))
    assert names == sorted([f"home_qlearner_agent_{i}.th" for i in range(3)]
                           + ["home_qlearner_mixer.th", "home_qlearner_opt.th"]), names
    fresh = DistinctMAC(exp.home_buffer.scheme, exp.groups, exp.args)
    fresh.load_models(path, "home_qlearner_")
    batch, _ = exp.stepper.run(test_mode=True)
    exp.stepper.flush()
    T = int(batch.max_t_filled())
    qs = []
    for mac in (exp.home_mac, fresh):
        mac.init_hidden(batch.batch_size)
        with torch.no_grad():
            qs.append(torch.stack([mac.forward(batch, t) for t in range(T)], dim=1))
    assert torch.equal(qs[0], qs[1]) and bool(torch.isfinite(qs[0]).all())
    exp.home_learner.load_models(path)  # the learner's own reload: agents, targets, mixer, optimiser state
    for a, b in zip(exp.home_mac.agents, fresh.agents):
        assert all(torch.equal(v, b.state_dict()[k].to(v.device)) for k, v in a.state_dict().items())
