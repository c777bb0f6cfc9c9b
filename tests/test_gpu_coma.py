"""COMA on the GPU: the policy op, the multinomial draw, mlg_rollout_policy, the critic pipeline, the actor loss, the
learner and one MultiAgentExperiment run, against the float64 restatement (tests/coma_ref.py), the C env oracle and the
golden fixtures recorded from the reference (tests/golden/coma_*.npz).

Tolerances. policy_probs: rtol 2e-5, atol 1e-7 (the worst-case fp32 softmax bound is about (A + 4) 2^-24 at A = 96).
The draw is bit-identical to the fp32 restatement. Rollout: delta = 2e-4 on the cdf, twice the project's 1e-4 logit
tolerance, since sum |dp| <= 2 max |dlogit|. Critic, learner: 4x the fp32-vs-float64 noise floors measured on the CPU by
tests/test_coma_ref.py (its docstring lists the floors and these values); absolute."""
import os

import numpy as np
import pytest
import torch

import coma_ref as CR
import envref
import learner_ref as LR
import maleague  # noqa: F401  (registers torch.ops.maleague.*)
from conftest import GOLDEN
from helpers import (DELTA, NEAR_TIE_CAP, CriticHarness, _check_policy_run, _golden_batch, _policy_stepper,  # noqa: F401
                     _random_batch, _random_critic, coma_args, scheme_for)
from test_coma_ref import ACTOR_STATS, CRITIC_STATS, TOL, load_learner

pytestmark = pytest.mark.gpu

# ---- policy_probs ------------------------------------------------------------------------------------------------------
def _rows(R, A, seed):
    rng = np.random.RandomState(seed)
    logits = (rng.randn(R, A) * 2).astype(np.float32)
    avail = (rng.rand(R, A) < 0.6).astype(np.int32)
    avail[:, 0] = np.maximum(avail[:, 0], avail.sum(-1) == 0)
    avail[0] = 0
    avail[0, A // 2] = 1  # one available action
    if R > 1:
        avail[R - 1] = 0  # none
    return logits, avail, rng.randn(R, A).astype(np.float32)


@pytest.mark.parametrize("A", [11, 15, 55, 1, 16, 17, 64, 69])
@pytest.mark.parametrize("R", [1, 17, 130, 64, 65])
def test_policy_probs_forward_backward(device, A, R):
    logits, avail, g = _rows(R, A, 100 * A + R)
    for mask in (0, 1):
        for test in (0, 1):
            x = torch.tensor(logits, device=device, requires_grad=True)
            p = torch.ops.maleague.policy_probs(x, torch.tensor(avail, device=device), 0.3, mask, test)
            exp = CR.softmax_policy(logits, avail, 0.3, bool(mask), bool(test))
            got = p.detach().cpu().numpy()
            assert np.isfinite(got).all()
            np.testing.assert_allclose(got, exp, rtol=2e-5, atol=1e-7, err_msg=f"mask={mask} test={test}")
            if mask and not test:
                assert (got[avail == 0] == 0).all()
            (p * torch.tensor(g, device=device)).sum().backward()
            dexp = CR.softmax_policy_grad(logits, avail, 0.3, bool(mask), bool(test), g)
            np.testing.assert_allclose(x.grad.cpu().numpy(), dexp, rtol=2e-5, atol=1e-7,
                                       err_msg=f"backward mask={mask} test={test}")


def test_policy_probs_matches_the_reference_fixture_and_opcheck(device):
    d = np.load(f"{GOLDEN}/coma_policy.npz")
    for A in (11, 15, 55):
        x = torch.tensor(d[f"A{A}.logits"], device=device)
        av = torch.tensor(d[f"A{A}.avail"], device=device)
        for mask in (0, 1):
            for test in (0, 1):
                p = torch.ops.maleague.policy_probs(x, av, float(d["epsilon"]), mask, test)
                np.testing.assert_allclose(p.cpu().numpy(), d[f"A{A}.probs.mask{mask}.test{test}"], rtol=2e-5, atol=1e-7)
    x = torch.tensor(d["A15.logits"], device=device, requires_grad=True)
    av = torch.tensor(d["A15.avail"], device=device)
    torch.library.opcheck(torch.ops.maleague.policy_probs.default, (x, av, 0.3, 1, 0),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    keys = torch.arange(6, dtype=torch.int64, device=device)
    eps = torch.zeros(6, dtype=torch.int32, device=device)
    torch.library.opcheck(torch.ops.maleague.select_multinomial.default, (x.detach(), av, keys, eps, 0, 0),
                          test_utils=("test_schema", "test_faketensor"))


# ---- mlg_select_multinomial -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [11, 15, 55, 1, 16, 17, 64, 69])
@pytest.mark.parametrize("B", [1, 17, 130, 64, 65])
def test_select_multinomial_bit_identical(device, A, B):
    N = 3
    logits, avail, _ = _rows(B * N, A, 7 * A + B)
    p = torch.ops.maleague.policy_probs(torch.tensor(logits, device=device), torch.tensor(avail, device=device), 0.3,
                                        0, 0).view(B, N, A)
    av = torch.tensor(avail, device=device).view(B, N, A)
    keys_h = [envref.env_key(11, b) for b in range(B)]
    keys = torch.tensor(np.array(keys_h, dtype=np.uint64).view(np.int64), device=device)
    episodes_h = [(3 * b) % 5 for b in range(B)]
    episodes = torch.tensor(episodes_h, dtype=torch.int32, device=device)
    ph, avh = p.cpu().numpy(), av.cpu().numpy()
    for greedy in (0, 1):
        got = torch.ops.maleague.select_multinomial(p, av, keys, episodes, 4, greedy).cpu().numpy()
        for b in range(B):
            for n in range(N):
                exp = CR.select_multinomial(ph[b, n], avh[b, n], keys_h[b], episodes_h[b], 4, n, greedy=bool(greedy))
                assert got[b, n] == exp, (greedy, b, n)
                assert avh[b, n, got[b, n]] != 0 or not avh[b, n].any()


def test_select_multinomial_greedy_ties_and_selector(device):
    from maleague.components.action_selectors import MultinomialActionSelector
    p = torch.tensor([[[0.2, 0.3, 0.3, 0.2], [0.5, 0.5, 0.0, 0.0], [0.1, 0.2, 0.3, 0.4]]], device=device)
    av = torch.tensor([[[1, 1, 1, 1], [0, 1, 1, 1], [1, 1, 1, 0]]], dtype=torch.int32, device=device)
    sel = MultinomialActionSelector(coma_args())
    a, none = sel.select(p, av, 0, test_mode=True)
    assert none is None and a.dtype == torch.int64 and a.cpu().tolist() == [[1, 1, 2]]
    draws = torch.stack([sel.select(p, av, 0, test_mode=False)[0] for _ in range(64)])
    taken = torch.gather(av.expand(64, -1, -1, -1).reshape(64, 3, 4), 2, draws.reshape(64, 3, 1))
    assert bool((taken == 1).all()) and len(torch.unique(draws[:, 0, 0])) > 1


# ---- BasicMAC.forward with pi_logits ------------------------------------------------------------------------------------
def test_mac_forward_pi_logits_both_modes(device):
    """Fused (no_grad) and differentiable forward both give the float64 restatement's probabilities within the
    project's 1e-4 logit tolerance (the two read their inputs differently -- from the batch / from a dense row -- and
    are not bit-identical)."""
    from maleague.controllers import BasicMAC, EntityMAC  # noqa: F401
    d, batch, pa, _ = load_learner("mask")
    eb = _golden_batch(batch, device)
    for mask in (True, False):
        mac = BasicMAC(eb.scheme, eb.groups, coma_args(mask_before_softmax=mask))
        mac.load_state_dict({k: torch.from_numpy(v) for k, v in pa.items()})
        mac.cuda()
        p64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in pa.items()}
        tb = {k: torch.tensor(batch[k], dtype=torch.float64) for k in ("obs", "actions_onehot")}
        logits, _ = LR.mac_unroll(p64, tb, 5, h0=torch.zeros(20, 64, dtype=torch.float64))
        outs = {}
        for mode in ("fused", "grad"):
            mac.enable_autograd(mode == "grad")
            mac.init_hidden(4)
            with torch.enable_grad() if mode == "grad" else torch.no_grad():
                outs[mode] = torch.stack([mac.forward(eb, t) for t in range(7)], dim=1)
            assert outs[mode].requires_grad == (mode == "grad")
        exp = CR.softmax_policy(logits.numpy(), batch["avail_actions"], 0.5, mask, False)
        for mode, o in outs.items():
            np.testing.assert_allclose(o.detach().cpu().numpy(), exp, atol=1e-4, rtol=0, err_msg=mode)
        mac.enable_autograd(False)
        mac.init_hidden(4)
        test_p = mac.forward(eb, 0, test_mode=True).cpu().numpy()
        np.testing.assert_allclose(test_p, CR.softmax_policy(logits.numpy()[:, 0], batch["avail_actions"][:, 0], 0.5, mask,
                                                             True), atol=1e-4, rtol=0)


def test_self_play_stepper_refuses_pi_logits(device):
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.envs.plans import builtin_plan
    from maleague.steppers import SelfPlayParallelStepper
    args = coma_args(batch_size_run=2, env_args={"match_build_plan": builtin_plan("small", self_play=True),
                                                  "grid_size": 20, "stochastic_spawns": True, "episode_limit": 5})
    stepper = SelfPlayParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    from maleague.components.episode_batch import EpisodeBatch
    scheme, groups, preprocess = scheme_for({**info, "n_agents": args.n_agents}, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    mac = BasicMAC(proto.scheme, groups, args)
    with pytest.raises(NotImplementedError, match="agent_output_type"):
        stepper.initialize(scheme, groups, preprocess, mac, mac)


# ---- mlg_rollout_policy -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("plan", ["small", "medium_1h_4t"])
def test_rollout_policy(device, plan, H, mask):
    """One launch per run; train mode (eps 0.3) draws within delta of the restated cdf, test mode takes the first-index
    argmax; the ring's full-write output equals the plain-mode bytes."""
    from maleague.components.replay_buffer import ReplayBuffer
    from maleague.envs.teams_env import VecEnvState
    stepper, mac, args, (scheme, groups, preprocess) = _policy_stepper(device, plan, H, mask)
    batch, _ = stepper.run(test_mode=True)
    _check_policy_run(stepper, mac, args, batch, 0, True, mask)
    assert stepper.t_env == 0
    batch, _ = stepper.run(test_mode=False)
    _check_policy_run(stepper, mac, args, batch, 1, False, mask)
    assert stepper.t_env == int(stepper.last_run["ep_len"].sum())
    plain = {k: batch[k].clone() for k in batch.data.transition_data}
    # the same run (episode counter 1) written into ring slots that held other bytes
    ring = ReplayBuffer(scheme, groups, 40, stepper.episode_limit + 1, preprocess=preprocess, device=device)
    for v in ring.data.transition_data.values():
        v.fill_(7)
    ring.buffer_index = 30  # wraps: slots 30..39, 0..6
    st = VecEnvState(stepper.spec, stepper.batch_size, device)
    st.episode.fill_(1)
    stepper.envs = st
    assert stepper.attach_replay(ring)
    b_ring, _ = stepper.run(test_mode=False)
    for k, v in plain.items():
        assert torch.equal(v, b_ring[k]), k


def test_rollout_policy_refuses_nothing_silently(device):
    """H = 128 runs too (the generic kernel); an unsupported hidden width is refused with the key's name."""
    from maleague._native import NativeError
    stepper, mac, args, _ = _policy_stepper(device, "small", 128, False, B=3, episode_limit=6)
    batch, _ = stepper.run(test_mode=False)
    _check_policy_run(stepper, mac, args, batch, 0, False, False)
    bad = mac.agent.dims()
    bad.hidden = 48
    from maleague import _native
    with pytest.raises(NativeError, match="rnn_hidden_dim"):
        _native.call("mlg_rollout_policy", _native.byref(stepper._cspec), _native.byref(stepper.envs.to_c()),
                     _native.byref(bad), None, None, None, 0.0, 0, 0, 0, None)


# ---- mlg_coma_critic_train ----------------------------------------------------------------------------------------------
def test_critic_train_against_the_reference_fixture(device):
    d, batch, _, pc = load_learner("mask")
    eb = _golden_batch(batch, device)
    h = CriticHarness(pc, device, 4, 7, 5, 15, 80, 60, interval=10)
    for i in range(3):
        q, tg, st = h.train(eb)
        err = {"q_vals": np.abs(q - d[f"q_vals{i}"]).max(), "targets": np.abs(tg - d[f"targets{i}"]).max(),
               "critic_stats": max(abs(st[j] / st[5] - float(d[f"stat{i}.{k}"])) for j, k in enumerate(CRITIC_STATS)),
               "critic_params": max(np.abs(h.params.cpu().numpy()[::16] - d[f"sub{i}.critic"]).max(),
                                    np.abs(h.target.cpu().numpy()[::16] - d[f"sub{i}.target_critic"]).max())}
        print(f"call {i}: " + ", ".join(f"{k} {v:.3g} (tol {TOL[k]:.3g})" for k, v in err.items()))
        assert st[5] == 6 and h.counters.cpu().tolist() == [int(d[f"steps{i}"]), int(d[f"last_update{i}"])]
        for k, v in err.items():
            assert v <= TOL[k], (i, k, v, TOL[k])
    np.testing.assert_allclose(h.params.cpu().numpy(),
                               np.concatenate([d[f"p3.critic.{k}"].reshape(-1) for k in CR.CRITIC_KEYS]),
                               atol=TOL["critic_params_full"], rtol=0)


@pytest.mark.parametrize("case", ["B1", "B9_N3_A11", "tail_skips", "rows"])
def test_critic_train_against_the_restatement(device, case):
    """B = 1; B = 9, N = 3, A = 11 (a partly filled 16-row tile next to a full one); every episode ends three steps
    early (the tail steps are skipped on the device: q_vals zero, no optimizer step); a slot map."""
    shape = {"B1": (1, 6, 5, 15, 24, 12, [5]), "B9_N3_A11": (9, 5, 3, 11, 16, 10, [4, 2, 3, 4, 1, 4, 3, 2, 4]),
             "tail_skips": (3, 8, 2, 7, 8, 6, [4, 3, 4]), "rows": (3, 5, 2, 7, 8, 6, [4, 2, 3])}[case]
    B, T, N, A, d_obs, S, lengths = shape
    D = S + d_obs + 2 * N * A + N
    pc = _random_critic(D, A, 31)
    if case == "rows":  # three episodes read out of a five-slot buffer through rows = [3, 0, 4]
        store = _random_batch(5, T, N, A, d_obs, S, [1, 3, 4, 4, 2], 41)
        slots = [3, 0, 4]
        batch = {k: v[slots] for k, v in store.items()}
        eb = _golden_batch(store, device)
        rows = torch.tensor(slots, dtype=torch.int32, device=device)
    else:
        batch = _random_batch(B, T, N, A, d_obs, S, lengths, 41)
        eb, rows = _golden_batch(batch, device), None
    ref = CR.CriticRef(pc)
    h = CriticHarness(pc, device, B, T, N, A, d_obs, S)
    for i in range(2):
        eq, etg, esums, taken = ref.train(batch)
        q, tg, st = h.train(eb, rows)
        assert st[5] == taken and int(h.counters[0]) == ref.steps
        flat = np.concatenate([ref.p[k].reshape(-1) for k in CR.CRITIC_KEYS])
        err = {"q_vals": np.abs(q - eq).max(), "targets": np.abs(tg - etg).max(),
               "critic_stats": np.abs(st[:5] / max(taken, 1) - esums / max(taken, 1)).max(),
               "critic_params": np.abs(h.params.cpu().numpy() - flat).max()}
        print(f"{case} call {i}: " + ", ".join(f"{k} {v:.3g} (tol {TOL[k]:.3g})" for k, v in err.items()))
        for k, v in err.items():
            assert v <= TOL[k], (case, i, k, v, TOL[k])
    if case == "tail_skips":
        assert taken == 4 and not q[:, 4:].any() and q[:, :4].any()


def test_critic_train_is_bitwise_reproducible(device):
    d, batch, _, pc = load_learner("nomask")
    eb = _golden_batch(batch, device)
    outs = []
    for _ in range(2):
        h = CriticHarness(pc, device, 4, 7, 5, 15, 80, 60)
        q, tg, st = h.train(eb)
        outs.append((q, tg, st, h.params.cpu().numpy(), h.sq.cpu().numpy(), h.grads.cpu().numpy()))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


def test_critic_train_refuses_unsupported_shapes(device):
    from maleague import _native
    cfg = _native.MlgComaCfg(B=4, T=7, N=5, A=15, d_obs=80, S=60, hidden=64)
    with pytest.raises(_native.NativeError, match="hidden"):
        _native.call("mlg_coma_critic_train", _native.byref(cfg), None, None)


# ---- the actor loss ---------------------------------------------------------------------------------------------------
def test_coma_policy_loss_against_autograd(device):
    rng = np.random.RandomState(9)
    B, Tm, N, A = 3, 5, 4, 11
    pi = rng.dirichlet(np.ones(A), size=(B, Tm, N))
    avail = (rng.rand(B, Tm, N, A) < 0.6).astype(np.int32)
    actions = np.zeros((B, Tm, N, 1), np.int64)
    for idx in np.ndindex(B, Tm, N):
        if not avail[idx].any():
            avail[idx][rng.randint(A)] = 1
        actions[idx][0] = rng.choice(np.nonzero(avail[idx])[0])
    mask = (rng.rand(B, Tm, 1) < 0.7).astype(np.float64)
    mask[0, 0] = 1
    avail[B - 1, Tm - 1] = 0  # a padding row: avail all zero (its mask is zero as well)
    mask[B - 1, Tm - 1] = 0
    q = rng.randn(B, Tm, N, A)
    x = torch.tensor(pi, requires_grad=True)
    exp = CR.actor_loss_torch(x, torch.tensor(avail), torch.tensor(actions), torch.tensor(q), torch.tensor(mask))
    exp[0].backward()
    xg = torch.tensor(pi, dtype=torch.float32, device=device, requires_grad=True)
    args = (xg, torch.tensor(avail, device=device), torch.tensor(actions, device=device),
            torch.tensor(q, dtype=torch.float32, device=device), torch.tensor(mask, dtype=torch.float32, device=device))
    stats, _ = torch.ops.maleague.coma_policy_loss(*args)
    (2.0 * stats[0]).backward()
    got = stats.detach().cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(xg.grad.cpu().numpy()).all()
    np.testing.assert_allclose(got, [float(v.detach()) for v in exp], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(xg.grad.cpu().numpy(), 2.0 * x.grad.numpy(), rtol=2e-5, atol=1e-7)
    assert not xg.grad[B - 1, Tm - 1].any()
    torch.library.opcheck(torch.ops.maleague.coma_policy_loss.default, args,
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))


# ---- COMALearner and the experiment -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["mask", "nomask"])
def test_coma_learner_against_the_reference_fixture(device, tag):
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.learners import COMALearner
    d, batch, pa, pc = load_learner(tag)
    eb = _golden_batch(batch, device)
    args = coma_args(mask_before_softmax=bool(d["mask_before_softmax"]), target_update_interval=10)
    mac = BasicMAC(eb.scheme, eb.groups, args)
    mac.load_state_dict({k: torch.from_numpy(v) for k, v in pa.items()})
    learner = COMALearner(mac, eb.scheme, MainLogger(), args, name="home")
    assert learner.name == "home_comalearner_"
    learner.critic.load_state_dict({k: torch.from_numpy(v) for k, v in pc.items()})
    learner.target_critic.load_state_dict({k: torch.from_numpy(v) for k, v in pc.items()})
    learner.build_optimizer()
    for i, (t_env, ep) in enumerate(d["calls"]):
        learner.train(eb, int(t_env), int(ep))
        st = learner.last_stats
        assert set(st) == set(CRITIC_STATS) | {"home_comalearner_" + k for k in ACTOR_STATS}
        flat = lambda m: torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()  # noqa: E731
        err = {"q_vals": np.abs(learner.q_vals.cpu().numpy() - d[f"q_vals{i}"]).max(),
               "targets": np.abs(learner.targets.cpu().numpy() - d[f"targets{i}"]).max(),
               "critic_stats": max(abs(st[k] - float(d[f"stat{i}.{k}"])) for k in CRITIC_STATS),
               "actor_stats": max(abs(st["home_comalearner_" + k] - float(d[f"stat{i}.{k}"])) for k in ACTOR_STATS),
               **{"actor." + k: abs(st["home_comalearner_" + k] - float(d[f"stat{i}.{k}"])) for k in ACTOR_STATS},
               "critic_params": max(np.abs(flat(learner.critic)[::16] - d[f"sub{i}.critic"]).max(),
                                    np.abs(flat(learner.target_critic)[::16] - d[f"sub{i}.target_critic"]).max()),
               "agent_params": np.abs(flat(mac.agent)[::16] - d[f"sub{i}.agent"]).max()}
        per_stat = {k: err.pop(k) for k in list(err) if k.startswith("actor.")}
        print(f"{tag} call {i}: " + ", ".join(f"{k} {v:.3g} (tol {TOL[k]:.3g})" for k, v in err.items())
              + " | " + ", ".join(f"{k} {v:.3g}" for k, v in per_stat.items()))
        assert learner.critic_training_steps == int(d[f"steps{i}"])
        assert learner.last_target_update_step == int(d[f"last_update{i}"])
        for k, v in err.items():
            assert v <= TOL[k], (tag, i, k, v, TOL[k])
    for name, module, keys in (("critic", learner.critic, CR.CRITIC_KEYS), ("agent", mac.agent, LR.AGENT_KEYS)):
        exp = np.concatenate([d[f"p3.{name}.{k}"].reshape(-1) for k in keys])
        np.testing.assert_allclose(flat(module), exp, atol=TOL[f"{name}_params_full"], rtol=0)


def test_coma_experiment_runs_and_checkpoints(device, tmp_path):
    from maleague.custom_logging import MainLogger
    from maleague.learners import COMALearner
    from maleague.runs import MultiAgentExperiment
    from maleague.utils.config import build_config, to_args
    cfg = build_config("coma", "ma", overrides=["buffer_cpu_only=False", "env_args.episode_limit=20",
                                                "env_args.match_build_plan=small", "seed=0",
                                                "show_exp_parameters=False", "t_max=1000000",
                                                "test_interval=100000000", "learner_log_interval=0",
                                                f"local_results_path={tmp_path}"])
    assert cfg["batch_size_run"] == cfg["batch_size"] == cfg["buffer_size"] == 8
    np.random.seed(0)
    torch.manual_seed(0)
    logger = MainLogger(log_interval=10 ** 12)
    exp = MultiAgentExperiment(to_args(cfg), logger)
    learner = exp.home_learner
    assert type(learner) is COMALearner
    exp.start(max_iterations=3)
    assert learner.train_calls == 3
    stats = learner.last_stats
    want = set(CRITIC_STATS) | {"home_comalearner_" + k for k in ACTOR_STATS}
    assert set(stats) == want and all(np.isfinite(v) for v in stats.values()), stats
    assert learner.critic_training_steps > 0
    path = str(tmp_path / "ckpt")
    os.makedirs(path)
    learner.save_models(path, learner.name)
    assert sorted(os.listdir(path)) == ["agent_opt.th", "critic.th", "critic_opt.th", "home_comalearner_agent.th"]
    saved = {"agent": {k: v.clone() for k, v in exp.home_mac.agent.state_dict().items()},
             "critic": {k: v.clone() for k, v in learner.critic.state_dict().items()},
             "sq": learner._sq.clone()}
    # both optimizer files load into a plain torch.optim.RMSprop over parameters of the same shapes
    for name, params in (("agent_opt.th", learner.agent_params), ("critic_opt.th", learner.critic_params)):
        opt = torch.optim.RMSprop([torch.nn.Parameter(torch.zeros_like(p)) for p in params], lr=5e-4)
        opt.load_state_dict(torch.load(f"{path}/{name}", weights_only=True))
    with torch.no_grad():
        for p in learner.params:
            p.add_(1.0)
        learner._sq.zero_()
    learner.load_models(path)
    for k, v in exp.home_mac.agent.state_dict().items():
        assert torch.equal(v, saved["agent"][k]), k
    for k, v in learner.critic.state_dict().items():
        assert torch.equal(v, saved["critic"][k]), k
        assert torch.equal(learner.target_critic.state_dict()[k], v), k
    assert torch.equal(learner._sq, saved["sq"])
