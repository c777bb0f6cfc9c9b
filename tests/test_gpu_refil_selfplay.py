"""GPU parity of mlg_refil_rollout_selfplay (DESIGN.md §3b', §4c''): two EntityMACs in one launch against the float64
oracle, per side (tests/refil_selfplay_shapes.py holds the case table, tests/refil_selfplay_ref.py the oracle,
tests/test_refil_selfplay.py pins dispatch, spec and refusals on the CPU).

Every case asserts its arm through the host query, then runs B = 37 envs (ragged against the 8-env workgroup),
episode_limit 30, grid 20: once in test mode from fresh state and once in train mode on the state the first run left
(episode 1, eps_home 0.525, eps_away 0.3). Both runs go to the teacher-forced checker: both sides' recorded actions
replayed through the oracle env (the away side's through the raw image of its canonical indices), env-side arrays,
episode signals and run summary bit-exact per side, every epsilon draw the oracle's draw and every other pick an argmax
of that side's float64 Q. A different pick passes only at a near tie within Q_TOL = 1e-4, and at most 1 % of a side's
decisions may pass that way (the seeds are chosen so that the float64 oracle alone sees at most 0.5 %).
"""
import numpy as np
import pytest
import torch

import refil_selfplay_ref as SR
import refil_selfplay_shapes as SS
from helpers import Q_TOL, refil_oracle_q

pytestmark = pytest.mark.gpu

NEAR_TIE_CAP = 0.01
F64 = torch.float64
CASES = [c.id for c in SS.SP_CASES]


def _launch(device, c, B=SS.B, **kw):
    spec = SS.spec_for(c, kw.pop("seed", None))
    return (spec,) + SR.sp_rollout(device, spec, SR.case_params(c), la=c.la, B=B, **kw)


@pytest.fixture(scope="module")
def two_runs(device):
    """Per case, computed once and shared (never modified): the test-mode run of episode 0 and the train-mode run of
    episode 1 from the state the first left, host copies."""
    cache = {}

    def get(cid):
        if cid not in cache:
            c = SS.case(cid)
            spec, agents, nbs0, summ0, st, _ = _launch(device, c, eps=(0.0, 0.0), test_mode=True)
            _, _, nbs1, summ1, _, _ = _launch(device, c, eps=(SS.EPS_HOME, SS.EPS_AWAY), test_mode=False, st=st,
                                               agents=agents)
            for nbs, summ in ((nbs0, summ0), (nbs1, summ1)):
                for v in [v for nb in nbs for v in nb.values()] + list(summ.values()):
                    v.setflags(write=False)
            cache[cid] = (spec, agents, ((nbs0, summ0, (0.0, 0.0), True, 0),
                                         (nbs1, summ1, (SS.EPS_HOME, SS.EPS_AWAY), False, 1)))
        return cache[cid]
    return get


def _cap(cid, mode, n):
    for side in SR.SIDES:
        print(f"{cid} [{mode}] {side}: {n[side]}")
        assert n[side]["decisions"] > 0
        assert n[side]["near_ties"] <= NEAR_TIE_CAP * n[side]["decisions"], (cid, mode, side, n[side])


def _check_rows(spec, nbs, summ, B, seed, episode):
    """Padded agent slots (>= the episode's k) have only action 0 available and take it, on both sides; nothing is
    written past an episode's end."""
    S, ks = spec.S, set()
    for b, r in enumerate(SR.ref_envs_for(spec, B, seed)):
        r.episode = episode
        r.reset()
        k, L = int(r.k), int(summ["len"][b])
        ks.add(k)
        for side, nb in zip(SR.SIDES, nbs):
            av = nb["avail_actions"][b, :L + 1, k:]
            assert (av[..., 0] == 1).all() and (av[..., 1:] == 0).all(), (side, b, k)
            assert (nb["actions"][b, :L + 1, k:, 0] == 0).all(), (side, b, k)
            em = nb["entity_mask"][b]
            assert (em[:L + 1, k:S] == 1).all() and (em[:L + 1, S + k:] == 1).all(), (side, b, k)
            assert (em[0, :k] == 0).all() and (em[0, S:S + k] == 0).all(), (side, b, k)
            for key, v in nb.items():
                t0 = L if key in ("reward", "terminated") else L + 1
                assert not v[b, t0:].any(), (side, key, b, L)
    return ks


@pytest.mark.parametrize("cid", CASES)
def test_refil_selfplay_parity(device, cid, two_runs):
    from maleague import _native
    c = SS.case(cid)
    spec, agents, runs = two_runs(cid)
    name, lds = _native.refil_rollout_selfplay_describe(spec.to_c(), agents[0][0].dims())
    print(f"{cid}: arm {name}, {lds} B of LDS, S = {spec.S}, k = {c.kmin}..{c.kmax}, last action {c.la}")
    assert name == c.arm
    assert _native.refil_rollout_selfplay_describe(spec.to_c(), SS.side_dims(spec, c.la)) == (name, lds)
    ks, away_wins, away_acts = set(), 0, []
    for nbs, summ, eps, test_mode, episode in runs:
        n = SR.sp_teacher_check(spec, agents, nbs, summ, SS.B, c.seed, eps, test_mode, episode=episode, dtype=F64)
        _cap(cid, "test" if test_mode else "train", n)
        for s, side in enumerate(SR.SIDES):
            assert (n[side]["epsilon_draws"] == 0) == test_mode, (side, n[side])
        ks |= _check_rows(spec, nbs, summ, SS.B, c.seed, episode)
        away_wins += int(summ["won"][:, 1].sum())
        away_acts.append(np.concatenate([nbs[1]["actions"][b, :L, :, 0].ravel() for b, L in enumerate(summ["len"])]))
        # agent rows: both sides' S rows of every (env, step) up to and including the post-termination pick
        assert int(summ["agent_rows"][0]) == 2 * spec.S * int((summ["len"] + 1).sum())
    assert ks == set(range(c.kmin, c.kmax + 1)), ks  # every team size of the case was played
    # both sides act: the away side's executed actions move and target (and, on refil_8, win a battle)
    acts = np.concatenate(away_acts)
    moves, targets = int(((acts >= 1) & (acts <= 4)).sum()), int((acts >= 5).sum())
    print(f"{cid}: away wins {away_wins}, away moves {moves}, away targets {targets}")
    assert moves > 0 and targets > 0
    if cid == "refil_8":
        assert away_wins >= 1


# ---- the away batch is a self-contained entity batch ------------------------------------------------------------------

def _mac_inputs(nb, S, la, device):
    """EntityMAC._build_inputs over the whole recorded batch."""
    ent = torch.from_numpy(np.array(nb["entities"]))
    if la:
        acs = torch.zeros(ent.shape[:3] + (nb["actions_onehot"].shape[-1],))
        acs[:, 1:, :S] = torch.from_numpy(np.array(nb["actions_onehot"][:, :-1]))
        ent = torch.cat([ent, acs], dim=3)
    return (ent.to(device), torch.from_numpy(np.array(nb["obs_mask"])).to(device),
            torch.from_numpy(np.array(nb["entity_mask"])).to(device))


@pytest.mark.parametrize("cid", CASES)
def test_away_batch_replays_through_the_agent_forward(device, cid, two_runs):
    """mlg_refil_agent_forward with the away weights, teacher-forced along the away batch of the test-mode run alone,
    reproduces the recorded greedy picks up to the near-tie rule: a learner could train on that batch as it stands.
    Prints the largest fp32-vs-float64 Q difference of both sides along their batches."""
    c = SS.case(cid)
    spec, agents, runs = two_runs(cid)
    nbs, summ = runs[0][0], runs[0][1]
    S = spec.S
    worst = []
    for s, side in enumerate(SR.SIDES):
        ag, a = agents[s]
        with torch.no_grad():
            q, _ = ag(_mac_inputs(nbs[s], S, c.la, device), torch.zeros(SS.B, S, 64, device=device))
        q = q.cpu().numpy()
        q64 = refil_oracle_q(ag, a, nbs[s], dtype=F64)
        n_dec = n_tie = 0
        diff = 0.0
        for b in range(SS.B):
            for t in range(int(summ["len"][b]) + 1):
                diff = max(diff, float(np.abs(q[b, t] - q64[b, t]).max()))
                for k in range(S):
                    av = nbs[s]["avail_actions"][b, t, k] != 0
                    got = int(nbs[s]["actions"][b, t, k, 0])
                    m = np.where(av, q[b, t, k], -np.inf)
                    srt = np.sort(np.where(av, q64[b, t, k], -np.inf))
                    n_dec += int(np.isfinite(srt[-2]))
                    if int(np.argmax(m)) != got:
                        assert srt[-1] - srt[-2] <= Q_TOL and m[got] >= m.max() - Q_TOL, (side, b, t, k)
                        n_tie += 1
        print(f"{cid} {side}: max |Q fp32 - Q float64| = {diff:.3g} (Q_TOL {Q_TOL}), {n_tie} near ties of {n_dec}")
        assert diff <= Q_TOL, (side, diff)
        assert n_tie <= NEAR_TIE_CAP * n_dec
        worst.append(diff)


# ---- reruns, full-write mode, B = 1 ----------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", ["refil_8", "s1"])
def test_two_launches_are_bit_identical(device, cid, two_runs):
    c = SS.case(cid)
    _, _, runs = two_runs(cid)
    nbs0, summ0 = runs[0][0], runs[0][1]
    _, agents, nbs, summ, st, _ = _launch(device, c, eps=(0.0, 0.0), test_mode=True)
    for s in range(2):
        for k in nbs0[s]:
            np.testing.assert_array_equal(nbs0[s][k], nbs[s][k], err_msg=f"{SR.SIDES[s]} {k}")
    for k in summ0:
        np.testing.assert_array_equal(summ0[k], summ[k], err_msg=k)
    # and the train-mode run from equal state
    nbs1, summ1 = runs[1][0], runs[1][1]
    _, _, nbs, summ, _, _ = _launch(device, c, eps=(SS.EPS_HOME, SS.EPS_AWAY), test_mode=False, st=st, agents=agents)
    for s in range(2):
        for k in nbs1[s]:
            np.testing.assert_array_equal(nbs1[s][k], nbs[s][k], err_msg=f"{SR.SIDES[s]} {k}")
    for k in summ1:
        np.testing.assert_array_equal(summ1[k], summ[k], err_msg=k)


@pytest.mark.parametrize("cid", ["s5", "s3"])
def test_full_write_slot_extents_both_sides(device, cid):
    """test_refil_rollout_full_write_slot_extents_small_plans for both batches: one garbage-filled pair of batches
    rewritten by successive runs of different episodes in full-write mode with slot extents equals a zero-initialised
    pair every time, and both extents record L + 1. The third round mixes the modes (home full-write, away plain)."""
    c = SS.case(cid)
    B, T = 10, SS.EPISODE_LIMIT
    ext = [torch.full((B,), T + 1, dtype=torch.int32, device=device) for _ in range(2)]
    batches, agents = None, None
    for it, (seed, eps) in enumerate([(9, (0.2, 0.4)), (3, (0.6, 0.1)), (9, (0.0, 0.0)), (5, (0.3, 0.3))]):
        _, agents, nb0, s0, _, _ = _launch(device, c, B=B, seed=seed, eps=eps, test_mode=False, agents=agents)
        _, _, nb1, s1, _, batches = _launch(device, c, B=B, seed=seed, eps=eps, test_mode=False, agents=agents,
                                            full_write=(True, True), batches=batches, extents=ext)
        for s in range(2):
            for k in nb0[s]:
                np.testing.assert_array_equal(nb0[s][k], nb1[s][k], err_msg=f"{it} {SR.SIDES[s]} {k}")
            np.testing.assert_array_equal(ext[s].cpu().numpy(), s1["len"] + 1)
        for k in s0:
            np.testing.assert_array_equal(s0[k], s1[k], err_msg=f"{it} {k}")
    # each batch honours its mode on its own: home full-write over garbage, away plain over zeros
    _, _, nb0, s0, _, _ = _launch(device, c, B=B, seed=4, eps=(0.1, 0.1), test_mode=False, agents=agents)
    _, _, nb1, s1, _, _ = _launch(device, c, B=B, seed=4, eps=(0.1, 0.1), test_mode=False, agents=agents,
                                  full_write=(True, False))
    for s in range(2):
        for k in nb0[s]:
            np.testing.assert_array_equal(nb0[s][k], nb1[s][k], err_msg=f"mixed {SR.SIDES[s]} {k}")


def test_single_env(device):
    """B = 1 on the 5-slot case: one env in an 8-env workgroup, its wave's second env idle."""
    c = SS.case("s5")
    spec, agents, nbs, summ, st, _ = _launch(device, c, B=1, eps=(0.0, 0.0), test_mode=True)
    n = SR.sp_teacher_check(spec, agents, nbs, summ, 1, c.seed, (0.0, 0.0), True, episode=0, dtype=F64)
    assert n["home"]["decisions"] > 0 and n["away"]["decisions"] > 0
    eps = (SS.EPS_HOME, SS.EPS_AWAY)
    _, _, nbs, summ, _, _ = _launch(device, c, B=1, eps=eps, test_mode=False, st=st, agents=agents)
    SR.sp_teacher_check(spec, agents, nbs, summ, 1, c.seed, eps, False, episode=1, dtype=F64)


# ---- the checker itself ----------------------------------------------------------------------------------------------

def _recheck(two_runs, bad_away):
    c = SS.case("s5")
    spec, agents, runs = two_runs("s5")
    nbs, summ = runs[0][0], runs[0][1]
    return SR.sp_teacher_check(spec, agents, [nbs[0], bad_away], summ, SS.B, c.seed, (0.0, 0.0), True, dtype=F64)


def test_checker_rejects_a_wrong_away_greedy_action(two_runs):
    """One recorded greedy action of the away batch replaced by the runner-up at an episode's last step (recorded
    after termination, never executed), its one-hot row changed to match: only the argmax check can fail."""
    spec, agents, runs = two_runs("s5")
    nb, summ = runs[0][0][1], runs[0][1]
    q = refil_oracle_q(agents[1][0], agents[1][1], nb, dtype=F64)
    for b, n in ((b, n) for b in range(SS.B) for n in range(spec.S)):
        t = int(summ["len"][b])
        m = np.where(nb["avail_actions"][b, t, n] == 0, -np.inf, q[b, t, n])
        srt = np.sort(m)
        if np.isfinite(srt[-2]) and srt[-1] - srt[-2] > 10 * Q_TOL:
            break
    else:
        pytest.fail("no final step with two available actions and a clear Q gap")
    bad = {k: v.copy() for k, v in nb.items()}
    wrong = int(np.argsort(m)[-2])
    assert wrong != int(nb["actions"][b, t, n, 0])
    bad["actions"][b, t, n, 0] = wrong
    bad["actions_onehot"][b, t, n] = 0
    bad["actions_onehot"][b, t, n, wrong] = 1
    with pytest.raises(AssertionError) as exc:
        _recheck(two_runs, bad)
    assert f"('away', {b}, {t}, {n}" in str(exc.value), exc.value


def test_checker_rejects_a_flipped_away_obs_mask_bit(two_runs):
    _, _, runs = two_runs("s5")
    nb, summ = runs[0][0][1], runs[0][1]
    b = SS.B - 1
    assert summ["len"][b] > 2
    bad = {k: v.copy() for k, v in nb.items()}
    bad["obs_mask"][b, 2, 1, 3] ^= 1
    with pytest.raises(AssertionError, match=f"away obs_mask b={b} t=2"):
        _recheck(two_runs, bad)


def test_checker_rejects_a_wrong_away_reward(two_runs):
    _, _, runs = two_runs("s5")
    nb, summ = runs[0][0][1], runs[0][1]
    b = SS.B - 1
    assert summ["len"][b] > 3
    bad = {k: v.copy() for k, v in nb.items()}
    bad["reward"][b, 3, 0] += np.float32(1.0 / 16)
    with pytest.raises(AssertionError, match="'away', 'reward'"):
        _recheck(two_runs, bad)
    _recheck(two_runs, {k: v.copy() for k, v in nb.items()})  # and the unmodified copy still passes


# ---- end to end ------------------------------------------------------------------------------------------------------

def test_selfplay_experiment_trains_home_like_the_oracle(device, tmp_path):
    """SelfPlayMultiAgentExperiment with the refil config on the 5-slot plan, B = 8: the stepper is the entity one; one
    _train_episode; the home learner's stats and parameters match REFILLearnerRef on a host copy of the home batch
    (bounds of test_entity_stepper_five_slot_plan_trains_like_the_oracle: stats rtol 2e-4 / atol 1e-5, parameters atol
    2e-5); the away MAC is untouched. Then the trained home vector is loaded into the away MAC and a test-mode run passes
    the teacher check with those weights on the away side: the home weights play away through the canonical view."""
    import refil_ref as RR
    from helpers import refil_args
    from maleague.custom_logging import MainLogger
    from maleague.learners import REFILLearner
    from maleague.runs.sp_ma_experiment import SelfPlayMultiAgentExperiment, agent_vector
    from maleague.steppers import SelfPlayEntityParallelStepper
    from maleague.utils.config import build_config, to_args
    c, B = SS.case("s5"), 8
    cfg = build_config("refil", "ma_entity", overrides=[
        "runner=parallel", f"batch_size_run={B}", f"batch_size={B}", "buffer_cpu_only=False", "buffer_size=16",
        f"seed={c.seed}", "show_exp_parameters=False", "t_max=1000000", "test_interval=100000000",
        f"local_results_path={tmp_path}"])
    cfg["env_args"] = dict(cfg["env_args"], **SS.env_args(c))
    np.random.seed(0)
    torch.manual_seed(c.seed)
    exp = SelfPlayMultiAgentExperiment(to_args(cfg), MainLogger(log_interval=10 ** 12))
    learner = exp.home_learner
    assert type(exp.stepper) is SelfPlayEntityParallelStepper and type(learner) is REFILLearner
    a = exp.args
    assert (a.n_agents, a.total_n_agents, a.n_entities, a.n_actions, a.entity_shape) == (5, 10, 10, 15, 8)
    agent_p = {k: v.detach().cpu().clone() for k, v in exp.home_mac.agent.state_dict().items()}
    mixer_p = {k: v.detach().cpu().clone() for k, v in learner.mixer.state_dict().items()}
    away0 = agent_vector(exp.away_mac).clone()
    assert not torch.equal(away0, agent_vector(exp.home_mac))
    exp._init_stepper()
    assert exp.stepper.describe_rollout()[0] == "sp-ro2/kc2"
    exp.stepper.t_env = SS.FS.T_ENV
    exp._train_episode(0)
    torch.cuda.synchronize()
    assert learner.last_stats is not None and exp.home_buffer.episodes_in_buffer == B
    assert torch.equal(agent_vector(exp.away_mac), away0), "the frozen away MAC changed"
    batch = exp.stepper.home_batch
    T = int(batch.max_t_filled())
    sample = batch[:, :T]
    tb = {k: v.detach().cpu().clone() for k, v in sample.data.transition_data.items()}
    assert tb["entities"].shape == (B, T, 10, 8) and tb["avail_actions"].shape == (B, T, 5, 15)
    groupA = learner._groupA.detach().cpu().reshape(B, 1, 10)
    ref = RR.REFILLearnerRef(agent_p, mixer_p, refil_args(device="cpu", n_agents=5, n_entities=10, n_actions=15))
    want = ref.train(tb, groupA, episode_num=0)
    got = learner.last_stats
    for k in want:
        print(f"  {k}: {got[k]:.7g} vs oracle {want[k]:.7g}")
        np.testing.assert_allclose(got[k], want[k], rtol=2e-4, atol=1e-5, err_msg=k)
    for k, v in exp.home_mac.agent.named_parameters():
        np.testing.assert_allclose(v.detach().cpu().numpy(), ref.agent[k].detach().numpy(), atol=2e-5, rtol=0,
                                   err_msg=f"agent {k}")
    for k, v in learner.mixer.named_parameters():
        np.testing.assert_allclose(v.detach().cpu().numpy(), ref.mixer[k].detach().numpy(), atol=2e-5, rtol=0,
                                   err_msg=f"mixer {k}")
    # the trained home weights as the adversary
    exp.load_adversary_vector(agent_vector(exp.home_mac).clone())
    assert torch.equal(agent_vector(exp.away_mac), agent_vector(exp.home_mac))
    hb, ab, infos = exp.stepper.run(test_mode=True)
    torch.cuda.synchronize()
    from helpers import np_batch
    last = exp.stepper.last_run
    assert len(infos) == B
    host = exp.stepper._env_infos_of(exp.stepper._run_id)  # won / draw in env order (its items are in termination order)
    summ = {"len": last["ep_len"].numpy(), "won": host._won.astype(np.int32), "draw": host._draw.astype(np.int32),
            "ret": last["returns"].numpy(), "ret_away": last["away_returns"].numpy()}
    agents = [(exp.home_mac.agent, exp.args), (exp.away_mac.agent, exp.args)]
    n = SR.sp_teacher_check(exp.stepper.spec, agents, [np_batch(hb), np_batch(ab)], summ, B, c.seed, (0.0, 0.0), True,
                            episode=1, dtype=F64)
    print(f"home weights on both sides: {n}")
    assert n["away"]["decisions"] > 0
