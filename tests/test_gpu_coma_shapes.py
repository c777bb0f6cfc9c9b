"""COMA off the fixture shape, on the GPU: mlg_rollout_policy per reachable instantiation (H 32 / 64 / 128, one to four
agent tiles per wave, weights in LDS or global memory, one to five action tiles), mlg_coma_critic_train at the edges of
its loops, the actor loss past one pass of its stride loop, and COMALearner on the policy rollout's own batch. The
cases, their near-tie shares and their tolerances (4x the fp32-vs-float64 floor of each case, measured on the CPU) are
in tests/coma_shapes.py; tests/test_coma_shapes.py pins, without a GPU, the dispatch table, what each case is named
for and that these comparisons notice the defects they target.

Every policy case first asserts through the host query (stepper.describe_rollout) that it launches the instantiation it
is named for; its runs go through helpers._check_policy_run: env tensors bit-exact against the C env under teacher
forcing, every draw within DELTA = 2e-4 of the float64 cdf, every greedy pick the float64 argmax but for near ties
(at most 2 % of the rows; the float64 oracle alone sees at most 1 % at every (case, mask) that runs it)."""
import numpy as np
import pytest
import torch

import coma_ref as CR
import coma_shapes as CS
import learner_ref as LR
import maleague  # noqa: F401  (registers torch.ops.maleague.*)
from helpers import CriticHarness, _check_policy_run, _golden_batch, _policy_stepper, shape_plan

pytestmark = pytest.mark.gpu


# ---- mlg_rollout_policy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("cid", CS.POLICY_IDS)
def test_rollout_policy_case(device, cid, mask):
    """Episode 0 in train mode (epsilon 0.3), episode 1 in test mode without test_greedy (a draw from the floor-less
    probabilities), episode 2 greedy where the case lists the mask; at the ring cases the train-mode run written into
    ring slots that held other bytes equals the plain-mode bytes."""
    from maleague.components.replay_buffer import ReplayBuffer
    from maleague.envs.teams_env import VecEnvState
    c = CS.policy_case(cid)
    stepper, mac, args, (scheme, groups, preprocess) = _policy_stepper(
        device, shape_plan(c.plan), c.H, mask, B=CS.B, episode_limit=CS.EPISODE_LIMIT, seed=c.seed,
        agent_params=CS.policy_agent_params(c), fc2_scale=c.scale)
    name, lds = stepper.describe_rollout()
    assert name == c.arm and 0 < lds <= 160 * 1024
    spec = stepper.spec
    assert (spec.n_actions + 15) // 16 == CS.n_action_tiles(CS.policy_spec(c).n_actions)
    runs = [("train", CS.EP_TRAIN, False, True), ("draw", CS.EP_DRAW, True, False)]
    if mask in c.greedy:
        runs.append(("greedy", CS.EP_GREEDY, True, True))
    plain = None
    for tag, episode, test_mode, test_greedy in runs:
        mac.action_selector.test_greedy = test_greedy
        batch, _ = stepper.run(test_mode=test_mode)
        st = {}
        _check_policy_run(stepper, mac, args, batch, episode, test_mode, mask, test_greedy=test_greedy, stats=st)
        print(f"{cid} mask={int(mask)} {tag}: {st['rows']} rows, episode lengths "
              f"{int(stepper.last_run['ep_len'].min())}..{int(stepper.last_run['ep_len'].max())}, "
              + (f"{st['near_ties']} near ties ({100.0 * st['near_ties'] / st['rows']:.3f} %)" if tag == "greedy"
                 else f"largest distance of a draw outside its cdf interval {max(st['cdf_excess'], 0.0):.3g}"))
        if tag == "train":
            plain = {k: batch[k].clone() for k in batch.data.transition_data}
    if cid not in CS.RING_CASES:
        return
    # the train-mode run of episode 0 again, written into ring slots that held other bytes
    mac.action_selector.test_greedy = True
    ring = ReplayBuffer(scheme, groups, 40, stepper.episode_limit + 1, preprocess=preprocess, device=device)
    for v in ring.data.transition_data.values():
        v.fill_(7)
    ring.buffer_index = 30  # wraps: slots 30..39, 0..6
    stepper.envs = VecEnvState(stepper.spec, stepper.batch_size, device)
    assert stepper.attach_replay(ring)
    b_ring, _ = stepper.run(test_mode=False)
    for k, v in plain.items():
        assert torch.equal(v, b_ring[k]), k


# ---- mlg_coma_critic_train -----------------------------------------------------------------------------------------
def _critic_setup(c, device, ws_fill=float("nan")):
    pc, store, slots, batch = CS.critic_data(c)
    eb = _golden_batch(store, device)
    rows = None if slots is None else torch.tensor(slots, dtype=torch.int32, device=device)
    return pc, batch, eb, rows, CriticHarness(pc, device, c.B, c.T, c.N, c.A, c.d_obs, c.S, ws_fill=ws_fill)


@pytest.mark.parametrize("cid", CS.CRITIC_IDS)
def test_critic_train_case(device, cid):
    """Two calls against the float64 restatement; the workspace and the outputs are refilled with NaN before each; the
    target critic follows every 200 steps on both sides (between the calls of Tm258).

    These cases found the critic's dense layers less accurate than the bound allows: with one sequential fp32 chain
    over all K inputs (K = 400 at A96), A96's q_vals of call 1 differed by 9.73e-8 against 7.2e-8 and stride's
    parameters by 1.05e-6 against 8.48e-7. An fp32 restatement in that order reproduced the figures on the CPU
    (coma_ref.mm_ascending without blocks: 8.24e-8, 1.18e-6). dense16 now adds 32 inputs per chain and then the chains,
    which CriticRef(ascending=True) restates; measured since (profiles/coma/shapes_test_prints.txt): 3.03e-8 and 5.67e-7, every case within its bound."""
    c = CS.critic_case(cid)
    tol = CS.critic_tol(c)
    pc, batch, eb, rows, h = _critic_setup(c, device)
    ref = CR.CriticRef(pc)
    for i in range(2):
        h.refill()
        eq, etg, esums, taken = ref.train(batch)
        q, tg, st = h.train(eb, rows)
        ref.maybe_update_target(h.interval)
        assert h.interval == CS.TARGET_INTERVAL and h.counters.cpu().tolist() == [ref.steps, ref.last_update]
        assert np.isfinite(q).all() and np.isfinite(tg).all() and np.isfinite(st).all()
        assert st[5] == taken and int(h.counters[0]) == ref.steps
        flat = np.concatenate([ref.p[k].reshape(-1) for k in CR.CRITIC_KEYS])
        err = {"q_vals": np.abs(q - eq).max(), "targets": np.abs(tg - etg).max(),
               "critic_stats": np.abs(st[:5] / max(taken, 1) - esums / max(taken, 1)).max(),
               "critic_params": np.abs(h.params.cpu().numpy() - flat).max()}
        print(f"{cid} call {i}: " + ", ".join(f"{k} {v:.3g} (tol {tol[k]:.3g})" for k, v in err.items())
              + f"; {taken} steps, oracle grad norms {min(ref.norms):.3g}..{max(ref.norms):.3g}")
        for k, v in err.items():
            assert v <= tol[k], (cid, i, k, v, tol[k])
        if cid == "clip":  # the clip coefficient is below 1 at every step: the oracle's norms say so
            assert min(ref.norms) > 10.0 and abs(st[1] / taken - np.mean(ref.norms)) <= tol["critic_stats"]


def test_critic_train_ignores_what_the_workspace_held(device):
    """The same two calls with a NaN-filled workspace refilled before each call, a zero-filled one, and one that keeps
    what the first call left: bit for bit the same outputs, parameters and optimizer state."""
    c = CS.critic_case(CS.ZERO_WORKSPACE_CASE)
    outs = []
    for ws_fill, refill in ((float("nan"), True), (0.0, True), (float("nan"), False)):
        pc, batch, eb, rows, h = _critic_setup(c, device, ws_fill)
        res = []
        for i in range(2):
            if refill:
                h.refill()
            q, tg, st = h.train(eb, rows)
            res += [q, tg, st, h.params.cpu().numpy(), h.sq.cpu().numpy(), h.grads.cpu().numpy()]
        outs.append(res)
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.isfinite(a).all() and a.tobytes() == b.tobytes()


# ---- the actor loss ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,B,Tm,N,A", CS.ACTOR_CASES, ids=[c[0] for c in CS.ACTOR_CASES])
def test_coma_policy_loss_case(device, cid, B, Tm, N, A):
    pi, avail, actions, q, mask = CS.actor_inputs(B, Tm, N, A)
    x = torch.tensor(pi, requires_grad=True)
    exp = CR.actor_loss_torch(x, torch.tensor(avail), torch.tensor(actions), torch.tensor(q), torch.tensor(mask))
    exp[0].backward()
    xg = torch.tensor(pi, dtype=torch.float32, device=device, requires_grad=True)
    stats, _ = torch.ops.maleague.coma_policy_loss(
        xg, torch.tensor(avail, device=device), torch.tensor(actions, device=device),
        torch.tensor(q, dtype=torch.float32, device=device), torch.tensor(mask, dtype=torch.float32, device=device))
    (2.0 * stats[0]).backward()
    got, grad = stats.detach().cpu().numpy(), xg.grad.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(grad).all()
    want = [float(v.detach()) for v in exp]
    print(f"{cid}: stats {np.abs(got - want).max():.3g}, d pi {np.abs(grad - 2.0 * x.grad.numpy()).max():.3g}")
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(grad, 2.0 * x.grad.numpy(), rtol=2e-5, atol=1e-7)
    pad = ~avail.any(axis=-1)
    assert not grad[pad].any() and (pad.any() or cid == "R1")


# ---- COMALearner on the policy rollout's own batch ---------------------------------------------------------------------
def test_coma_learner_on_the_rollouts_own_batch(device):
    """9v9 at H = 64: the sample is cut to the longest episode, so max_seq_length is below the storage length and the
    critic reads the batch with a time stride above cfg.T. Three calls against LearnerRef (float64) on the same bytes.

    Measured on an MI355X (T = 52 of 65 slots): every quantity within 4x its floor. Before the critic's dense layers
    summed in blocks (coma.hip, dense16) pi_max of call 3 differed by 7.59e-8 against 6.52e-8; it is 1.63e-8 since
    (q_vals 1.15e-6 -> 4.9e-7)."""
    from maleague.custom_logging import MainLogger
    from maleague.learners import COMALearner
    c = CS.LEARNER_CASE
    stepper, mac, args, _ = _policy_stepper(device, shape_plan(c.plan), c.H, CS.LEARNER_MASK, B=CS.LEARNER_B,
                                            episode_limit=CS.LEARNER_LIMIT, seed=c.seed,
                                            agent_params=CS.policy_agent_params(c), fc2_scale=c.scale)
    assert stepper.describe_rollout()[0] == c.arm
    batch, _ = stepper.run(test_mode=False)
    T = int(batch.max_t_filled())
    assert T < CS.LEARNER_LIMIT + 1 == batch.max_seq_length
    sample = batch[:, :T]
    assert sample.max_seq_length == T
    nb = {k: v.detach().cpu().numpy() for k, v in sample.data.transition_data.items()}
    spec = stepper.spec
    pa, pc = CS.learner_params(spec)
    for k, v in mac.agent.state_dict().items():
        assert np.array_equal(v.detach().cpu().numpy(), pa[k]), k
    exp = CS.run_learner_ref(nb, spec, np.float64, calls=3)
    learner = COMALearner(mac, sample.scheme, MainLogger(), args, name="home")
    learner.critic.load_state_dict({k: torch.from_numpy(v) for k, v in pc.items()})
    learner.target_critic.load_state_dict({k: torch.from_numpy(v) for k, v in pc.items()})
    learner.build_optimizer()
    tol = CS.learner_tol()
    flat = lambda m: torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()  # noqa: E731
    for i, e in enumerate(exp):
        learner.train(sample, 1000 * (i + 1), 8 * (i + 1))
        st = learner.last_stats
        err = {"q_vals": np.abs(learner.q_vals.cpu().numpy() - e["q_vals"]).max(),
               "targets": np.abs(learner.targets.cpu().numpy() - e["targets"]).max(),
               "critic_stats": max(abs(st[k] - e["stats"][k]) for k in CS.CRITIC_STATS),
               "actor_stats": max(abs(st["home_comalearner_" + k] - e["stats"][k]) for k in CS.ACTOR_STATS),
               "critic_params": np.abs(flat(learner.critic) - e["critic_params"]).max(),
               "agent_params": np.abs(flat(mac.agent) - e["agent_params"]).max()}
        print(f"learner call {i} (T {T} of {CS.LEARNER_LIMIT + 1}): "
              + ", ".join(f"{k} {v:.3g} (tol {tol[k]:.3g})" for k, v in err.items()) + " | "
              + ", ".join(f"{k} {abs(st['home_comalearner_' + k] - e['stats'][k]):.3g} of {e['stats'][k]:.4g}"
                          for k in CS.ACTOR_STATS))
        assert [n for n, _ in mac.agent.named_parameters()] == LR.AGENT_KEYS
        for k, v in err.items():
            assert v <= tol[k], (i, k, v, tol[k])
    assert learner.critic_training_steps == 3 * (T - 1)
