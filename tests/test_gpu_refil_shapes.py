"""GPU parity of mlg_refil_rollout off the refil_8 shape: 1 to 8 unit slots per team on every arm of its dispatch
(tests/refil_shapes.py holds the case table, tests/test_refil_dispatch.py pins the arms on the CPU).

Every case first asserts through the host query (mlg_refil_rollout_describe) that it launches the arm it is named for,
then runs B = 37 envs (ragged against the 16-env workgroup of the four-env kernel and the 8-env workgroup of the
two-env kernel), episode_limit 30, once in test mode and once in train mode on the advanced env state (episode 1,
epsilon 0.525), and hands both runs to the teacher-forced checker of the REFIL suite (helpers.refil_teacher_check): the
recorded actions replayed through the C env oracle -- entities, obs_mask, entity_mask, avail, reward, terminated,
filled, one-hot rows, episode lengths, won / draw, returns -- every epsilon draw the oracle's draw from the counter RNG
and every other pick an argmax of the oracle EntityMAC's masked Q, unrolled in float64 here. A different pick passes
only at a near tie within Q_TOL = 1e-4, and at most NEAR_TIE_CAP = 1 % of a case's decisions (greedy picks with at least
two available actions) may pass that way: the seeds are chosen so that the float64 oracle alone sees at most 0.5 % of
its decisions at such a gap (refil_shapes.py lists the shares).

The weights come from numpy (refil_shapes.entity_agent_params), so the CPU count plays the same policies.
"""
import numpy as np
import pytest
import torch

import envref
import refil_shapes as FS
from helpers import (Q_TOL, ref_entity_envs_for, refil_args, refil_oracle_q, refil_rollout, refil_teacher_check)

pytestmark = pytest.mark.gpu

NEAR_TIE_CAP = 0.01
F64 = torch.float64
# episodes (of 37, train mode at epsilon 0.525 from fresh env state) in which the four-env kernel (fast GRU gates and
# softmax) leaves the two-env kernel's trajectory at a near-tie argmax flip: the measured count plus the margin of 2
# that V7_4V4_MAX_DIVERGING uses
RO4_VS_RO2_MAX_DIVERGING = {"s5": 2,   # measured 0
                            "s3": 2}   # measured 0


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    for k in FS.ENV_VARS:
        monkeypatch.delenv(k, raising=False)


def _setenv(monkeypatch, env):
    for k in FS.ENV_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _kw(cid, B=FS.B):
    _, codes, kmin, kmax, env, arm, seed = FS.case(cid)
    return dict(B=B, T=FS.EPISODE_LIMIT, seed=seed, kmin=kmin, kmax=kmax, plan=FS.plan(codes), grid=FS.GRID,
                agent_params=lambda d0, A: FS.entity_agent_params(d0, A, seed))


def _arm(cid):
    from maleague import _native
    spec = FS.spec_for(cid)
    return _native.refil_rollout_describe(spec.to_c(), FS.refil_dims(spec))


def _check_rows(spec, nb, summ, B, seed, episode):
    """On the recorded arrays: the padded agent slots (>= the episode's k) have only action 0 available and take it,
    and nothing is written past an episode's end (rows t > L of every key; reward and terminated from t = L)."""
    refs = ref_entity_envs_for(spec, B, seed=seed)
    ks = set()
    for b, r in enumerate(refs):
        r.episode = episode
        r.reset()
        k, L = int(r.k), int(summ["len"][b])
        ks.add(k)
        av = nb["avail_actions"][b, :L + 1, k:]
        assert (av[..., 0] == 1).all() and (av[..., 1:] == 0).all(), (b, k)
        assert (nb["actions"][b, :L + 1, k:, 0] == 0).all(), (b, k)
        assert (nb["entity_mask"][b, :L + 1, k:spec.S] == 1).all() and (nb["entity_mask"][b, 0, :k] == 0).all(), (b, k)
        for key, v in nb.items():
            t0 = L if key in ("reward", "terminated") else L + 1
            assert not v[b, t0:].any(), (key, b, L)
    return ks


def _cap(cid, mode, n):
    print(f"{cid} [{mode}]: {n}")
    assert n["decisions"] > 0
    assert n["near_ties"] <= NEAR_TIE_CAP * n["decisions"], (cid, mode, n)


def _parity(device, cid, monkeypatch, B=FS.B):
    from maleague import _native
    _, codes, kmin, kmax, env, arm, seed = FS.case(cid)
    _setenv(monkeypatch, env)
    name, lds = _arm(cid)
    print(f"{cid}: arm {name}, {lds} B of LDS, B = {B}, S = {len(codes.split())}, k = {kmin}..{kmax}")
    assert name == arm
    T = FS.EPISODE_LIMIT
    spec, ag, a, nb, summ, st = refil_rollout(device, eps=0.0, test_mode=True, **_kw(cid, B))
    assert _native.refil_rollout_describe(spec.to_c(), ag.dims()) == (name, lds)  # the dims the launch was given
    n = refil_teacher_check(spec, ag, a, nb, summ, B, T, seed, 0.0, True, dtype=F64, episode=0)
    _cap(cid, "test", n)
    assert n["epsilon_draws"] == 0
    ks = _check_rows(spec, nb, summ, B, seed, 0)
    # the train-mode run continues from the env state the first run left: episode counter 1
    spec, ag, a, nb, summ, st = refil_rollout(device, eps=FS.EPS, test_mode=False, st=st, **_kw(cid, B))
    n = refil_teacher_check(spec, ag, a, nb, summ, B, T, seed, FS.EPS, False, dtype=F64, episode=1)
    _cap(cid, "train", n)
    assert n["epsilon_draws"] > 0
    ks |= _check_rows(spec, nb, summ, B, seed, 1)
    if B == FS.B:
        assert ks == set(range(kmin, kmax + 1)), ks  # every team size of the case was played


@pytest.mark.parametrize("cid", [c[0] for c in FS.REFIL_CASES])
def test_refil_rollout_shape_parity(device, cid, monkeypatch):
    _parity(device, cid, monkeypatch)


def test_refil_rollout_shape_parity_single_env(device, monkeypatch):
    """B = 1 on the 5-slot ro4 case: one env in a 16-env workgroup, three idle env groups in its wave."""
    _parity(device, "s5-ro4", monkeypatch, B=1)


# ---- the four-env kernel against the two-env kernel ---------------------------------------------------------------

PRE_KEYS = ("entities", "obs_mask", "entity_mask", "avail_actions", "filled")


def _assert_near_tie_divergence(ref, got, q, B, seed, eps, episode):
    """Two kernels that agree up to fp32 rounding of the agent's arithmetic produce the same episodes except where a
    near tie flips an argmax. For every episode that differs, the first differing step t has identical pre-transition
    data (the env states agree up to t) and differs in the actions; every differing pick is a greedy pick of both (the
    epsilon coin of the counter RNG is not set: epsilon draws are equal wherever the trajectories coincide), available,
    and a near tie of the float64 oracle's Q along the trajectory (|Q[a_got] - Q[a_ref]| <= Q_TOL). Returns the number
    of differing episodes."""
    n_diff = 0
    for b in range(B):
        T1 = got["actions"].shape[1]
        t_first = next((t for t in range(T1) if any(not np.array_equal(ref[k][b, t], got[k][b, t]) for k in got)), None)
        if t_first is None:
            continue
        n_diff += 1
        for k in PRE_KEYS:
            assert np.array_equal(ref[k][b, t_first], got[k][b, t_first]), (b, t_first, k)
        av = got["avail_actions"][b, t_first].astype(bool)
        flips = np.nonzero(ref["actions"][b, t_first, :, 0] != got["actions"][b, t_first, :, 0])[0]
        assert len(flips) > 0, f"episode {b} diverges at t={t_first} without an action flip"
        key = envref.env_key(seed, b)
        for n in flips:
            coin = envref.u01(envref.rng(key, envref.ctr(episode, t_first, 2, int(n)))) < np.float32(eps)
            assert not coin, (b, t_first, n, "an epsilon draw differs")
            ag_, ar_ = int(got["actions"][b, t_first, n, 0]), int(ref["actions"][b, t_first, n, 0])
            assert av[n, ag_] and av[n, ar_], (b, t_first, n)
            assert abs(float(q[b, t_first, n, ag_]) - float(q[b, t_first, n, ar_])) <= Q_TOL, (b, t_first, n, ag_, ar_)
    return n_diff


@pytest.mark.parametrize("slots", ["s5", "s3"])
def test_refil_ro4_matches_ro2(device, slots, monkeypatch):
    """The four-env and the two-env kernel from the same fresh env state, train mode at epsilon 0.525: both runs pass
    the float64 teacher check on their own trajectories; env-side arrays and epsilon draws are equal bit for bit
    wherever the trajectories coincide; their GRU gate and softmax arithmetic differs (v_exp_f32 / v_rcp_f32 in the
    four-env kernel), so an episode may leave the other's trajectory, but only at a near-tie argmax flip."""
    c4, c2 = f"{slots}-ro4", f"{slots}-ro2"
    seed, T, B = FS.case(c4)[6], FS.EPISODE_LIMIT, FS.B
    runs = {}
    for cid in (c2, c4):
        _setenv(monkeypatch, FS.case(cid)[4])
        assert _arm(cid)[0] == FS.case(cid)[5]
        spec, ag, a, nb, summ, _ = refil_rollout(device, eps=FS.EPS, test_mode=False, **_kw(cid))
        n = refil_teacher_check(spec, ag, a, nb, summ, B, T, seed, FS.EPS, False, dtype=F64, episode=0)
        _cap(cid, "train, fresh state", n)
        runs[cid] = (nb, summ)
    (ref, sref), (got, sgot) = runs[c2], runs[c4]
    q = refil_oracle_q(ag, a, got, dtype=F64)
    n_diff = _assert_near_tie_divergence(ref, got, q, B, seed, FS.EPS, 0)
    same = [b for b in range(B) if all(np.array_equal(ref[k][b], got[k][b]) for k in got)]
    assert len(same) == B - n_diff
    for k in sref:
        np.testing.assert_array_equal(sref[k][same], sgot[k][same], err_msg=k)
    print(f"ro4 vs ro2 [{slots}]: {n_diff} of {B} episodes diverge (near-tie flips)")
    assert n_diff <= RO4_VS_RO2_MAX_DIVERGING[slots], n_diff


# ---- full-write mode where A < 12 ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", ["s5-ro4", "s5-ro2", "s3-ro4"])
def test_refil_rollout_full_write_slot_extents_small_plans(device, cid, monkeypatch):
    """test_rollout_full_write_slot_extents off the refil_8 shape: A = 15 (the second half-wave of the four-env
    kernel's one-hot writer has three columns) and A = 11 (it has none). One garbage-filled batch rewritten by
    successive runs of different episodes in full-write mode with slot extents equals a zero-initialised batch every
    time, and the extents record L + 1."""
    _setenv(monkeypatch, FS.case(cid)[4])
    assert _arm(cid)[0] == FS.case(cid)[5]
    B = 10
    kw = _kw(cid, B)
    T = kw["T"]
    ext = torch.full((B,), T + 1, dtype=torch.int32, device=device)  # rows unknown: a fresh garbage-filled batch
    batch = None
    for it, (seed, eps) in enumerate([(9, 0.2), (3, 0.6), (9, 0.0), (5, 0.3)]):
        kw["seed"] = seed
        *_, nb0, s0, _ = refil_rollout(device, eps=eps, test_mode=False, **kw)  # zero-initialised
        *_, nb1, s1, _ = refil_rollout(device, eps=eps, test_mode=False, ring=True, batch=batch, extent=ext, **kw)
        batch = refil_rollout.last_batch
        for k in nb0:
            np.testing.assert_array_equal(nb0[k], nb1[k], err_msg=f"{it} {k}")
        for k in s0:
            np.testing.assert_array_equal(s0[k], s1[k], err_msg=f"{it} {k}")
        np.testing.assert_array_equal(ext.cpu().numpy(), s1["len"] + 1)


# ---- the checker itself -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def recorded_run(device):
    """One passing test-mode run of the 5-slot ro4 case, copied to the host; shared and never modified."""
    import os
    assert not any(k in os.environ for k in FS.ENV_VARS)
    cid = "s5-ro4"
    seed = FS.case(cid)[6]
    spec, ag, a, nb, summ, _ = refil_rollout(device, eps=0.0, test_mode=True, **_kw(cid))
    args = (spec, ag, a)
    refil_teacher_check(*args, nb, summ, FS.B, FS.EPISODE_LIMIT, seed, 0.0, True, dtype=F64)
    for v in list(nb.values()) + list(summ.values()):
        v.setflags(write=False)
    return args, nb, summ, seed


def _recheck(recorded_run, bad):
    args, nb, summ, seed = recorded_run
    return refil_teacher_check(*args, bad, summ, FS.B, FS.EPISODE_LIMIT, seed, 0.0, True, dtype=F64)


def test_checker_rejects_a_wrong_greedy_action(recorded_run):
    """One recorded greedy action of the host copy replaced by the runner-up, at a step whose float64 Q gap is above
    10 Q_TOL: the checker must raise. The step is an episode's last (the action recorded after termination, which the
    env never executes), with its one-hot row changed to match, so the env replay and the bookkeeping checks still pass
    and the failure can only come from the agent-side argmax check."""
    (spec, ag, a), nb, summ, seed = recorded_run
    q = refil_oracle_q(ag, a, nb, dtype=F64)
    for b, n in ((b, n) for b in range(FS.B) for n in range(spec.n_agents)):
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
        _recheck(recorded_run, bad)
    assert f"({b}, {t}, {n})" in str(exc.value), exc.value  # raised by the argmax assertion, tagged (b, t, n)


def test_checker_rejects_a_flipped_obs_mask_bit(recorded_run):
    """One obs_mask byte of the host copy flipped: the env replay must raise, naming the array."""
    _, nb, summ, _ = recorded_run
    b = FS.B - 1
    assert summ["len"][b] > 2
    bad = {k: v.copy() for k, v in nb.items()}
    bad["obs_mask"][b, 2, 1, 3] ^= 1
    with pytest.raises(AssertionError, match=f"obs_mask b={b} t=2"):
        _recheck(recorded_run, bad)


def test_checker_rejects_a_wrong_reward(recorded_run):
    """One reward entry of the host copy changed by the env's smallest reward step (1 / 16): the env replay must
    raise."""
    _, nb, summ, _ = recorded_run
    b = FS.B - 1
    assert summ["len"][b] > 3
    bad = {k: v.copy() for k, v in nb.items()}
    bad["reward"][b, 3, 0] += np.float32(1.0 / 16)
    with pytest.raises(AssertionError):
        _recheck(recorded_run, bad)
    _recheck(recorded_run, {k: v.copy() for k, v in nb.items()})  # and the unmodified copy still passes


# ---- end to end: the path a user with a 5-unit plan runs -----------------------------------------------------------

class _Log:
    def __init__(self):
        self.stats = {}

    def log_stat(self, k, v, t):
        self.stats[k] = v

    def info(self, *a):
        pass


def test_entity_stepper_five_slot_plan_trains_like_the_oracle(device):
    """EntityParallelStepper over the 5-slot plan (describe_rollout names ro4) produces a train-mode batch; one
    REFILLearner.train on it against REFILLearnerRef on a host copy, within the bounds of
    test_refil_learner_na_not_multiple_of_8_matches_oracle (stats rtol 2e-4 / atol 1e-5, parameters atol 2e-5)."""
    import refil_ref as RR
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import EntityMAC
    from maleague.custom_logging import MainLogger
    from maleague.learners import REFILLearner
    from maleague.steppers import EntityParallelStepper
    from helpers import entity_scheme_for
    cid, B = "s5-ro4", 8
    seed = FS.case(cid)[6]
    args = refil_args(batch_size_run=B, batch_size=B, seed=seed, env_args=FS.env_args(cid))
    stepper = EntityParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.n_entities = info["n_agents"], info["n_actions"], info["n_entities"]
    assert (args.n_agents, args.n_entities, args.n_actions) == (5, 10, 15)
    scheme, groups, preprocess = entity_scheme_for(info, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    torch.manual_seed(seed)
    mac = EntityMAC(proto.scheme, groups, args)
    learner = REFILLearner(mac, proto.scheme, _Log(), args, name="home")
    agent_p = {k: v.detach().cpu().clone() for k, v in mac.agent.state_dict().items()}
    mixer_p = {k: v.detach().cpu().clone() for k, v in learner.mixer.state_dict().items()}
    learner.target_mac.load_state(mac)
    learner.build_optimizer()
    stepper.initialize(scheme, groups, preprocess, mac)
    name, lds = stepper.describe_rollout()
    print(f"EntityParallelStepper [{cid}]: arm {name}, {lds} B of LDS")
    assert name == "ro4"
    stepper.t_env = FS.T_ENV
    batch, infos = stepper.run(test_mode=False)
    torch.cuda.synchronize()
    L = stepper.last_run["ep_len"].numpy()
    assert len(infos) == B and (L >= 1).all() and (L <= FS.EPISODE_LIMIT).all()
    T = int(batch.max_t_filled())
    assert T == int(L.max()) + 1
    sample = batch[:, :T]
    tb = {k: v.detach().cpu().clone() for k, v in sample.data.transition_data.items()}
    assert tb["entities"].shape == (B, T, 10, 8) and tb["avail_actions"].shape == (B, T, 5, 15)
    g = torch.Generator().manual_seed(9)
    groupA = torch.bernoulli(torch.rand(B, 1, 1, generator=g).repeat(1, 1, 10), generator=g).to(torch.uint8)
    a_cpu = refil_args(device="cpu", n_agents=5, n_entities=10, n_actions=15)
    ref = RR.REFILLearnerRef(agent_p, mixer_p, a_cpu)
    want = ref.train(tb, groupA, episode_num=0)
    learner.train(sample, FS.T_ENV, episode_num=0, groupA=groupA.to(device))
    got = learner.last_stats
    for k in want:
        print(f"  {k}: {got[k]:.7g} vs oracle {want[k]:.7g}")
        np.testing.assert_allclose(got[k], want[k], rtol=2e-4, atol=1e-5, err_msg=k)
    for k, v in learner.mac.agent.named_parameters():
        np.testing.assert_allclose(v.detach().cpu().numpy(), ref.agent[k].detach().numpy(), atol=2e-5, rtol=0,
                                   err_msg=f"agent {k}")
    for k, v in learner.mixer.named_parameters():
        np.testing.assert_allclose(v.detach().cpu().numpy(), ref.mixer[k].detach().numpy(), atol=2e-5, rtol=0,
                                   err_msg=f"mixer {k}")
