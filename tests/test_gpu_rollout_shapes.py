"""GPU parity of mlg_rollout and mlg_rollout_selfplay for every dispatch arm: rnn_hidden_dim 32 / 64 / 128, team
sizes 2 to 25, unequal teams, the policy team listed first (tests/rollout_shapes.py holds the case tables,
tests/test_rollout_dispatch.py pins their arms on the CPU).

Every case first asserts through the host query (stepper.describe_rollout) that it launches the arm it is named for,
then runs B = 37 envs (ragged against the 16-env and the 8-env workgroups), episode_limit 30, once in test mode and
once in train mode at t_env = 25000 (epsilon 0.525; self-play: 0.525 / 0.3), and hands both runs to the checkers of
the rollout / self-play suites (helpers.check_run / check_sides): the recorded actions replayed through the C env
oracle -- obs, state, avail, reward, terminated, filled, one-hot, returns, episode lengths bit-exact -- and every
recorded action either the oracle's epsilon draw from the counter RNG or an argmax of the oracle DRQN's masked Q,
unrolled in float64 here. A different pick passes only at a near tie within Q_TOL = 1e-4 (also for the split-bf16
v7 / sp7 arms), and at most NEAR_TIE_CAP = 1 % of a case's greedy picks may pass that way: the seeds are chosen so that
the float64 oracle alone sees at most 0.5 % of its picks at such a gap (rollout_shapes.py lists the shares).

The weights come from numpy (rollout_shapes.agent_params), so the CPU count plays the same policies.
"""
import numpy as np
import pytest
import torch

import rollout_shapes as RS
from helpers import (Q_TOL, assert_near_tie_divergence, build_selfplay, build_stepper, check_run, check_sides, np_batch,
                     oracle_q, shape_plan)

pytestmark = pytest.mark.gpu

NEAR_TIE_CAP = 0.01
F64 = torch.float64
# episodes (of 37) of the runtime-shape split-bf16 kernels that leave the fp32 kernel's trajectory at a near-tie argmax
# flip, test mode: the measured count plus the margin of 2 that V7_MAX_DIVERGING / SP7_MAX_DIVERGING use
V7_4V4_MAX_DIVERGING = 2   # measured 0 (v7 vs v2)
SP7_4V4_MAX_DIVERGING = 2  # measured 0 (sp7 vs sp2)


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    for k in ("MLG_ROLLOUT_KERNEL", "MLG_ROLLOUT_GENERIC", "MLG_ROLLOUT_GLOBAL_WEIGHTS"):
        monkeypatch.delenv(k, raising=False)


def _load_weights(mac, seed):
    a = mac.agent
    p = RS.agent_params(a.input_shape, a.args.rnn_hidden_dim, a.args.n_actions, seed)
    a.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})


def _stepper(device, cid, B=RS.B):
    _, hidden, plan, arm, seed = RS.case(RS.ROLLOUT_CASES, cid)
    stepper, mac, args = build_stepper(device, plan=shape_plan(plan), B=B, episode_limit=RS.EPISODE_LIMIT, seed=seed,
                                       rnn_hidden_dim=hidden)
    _load_weights(mac, seed)
    return stepper, mac, args, arm


def _selfplay(device, cid, B=RS.B):
    _, hidden, plan, arm, seed = RS.case(RS.SELFPLAY_CASES, cid)
    stepper, home, away, args = build_selfplay(device, plan=shape_plan(plan, True), B=B,
                                               episode_limit=RS.EPISODE_LIMIT, seed=seed, rnn_hidden_dim=hidden)
    for mac, s in zip((home, away), RS.side_seeds(seed, True)):
        _load_weights(mac, s)
    return stepper, home, away, args, arm


def _cap(cid, mode, n):
    print(f"{cid} [{mode}]: {n}")
    assert n["near_ties"] <= NEAR_TIE_CAP * n["greedy"], (cid, mode, n)


def _parity(device, cid, B=RS.B):
    stepper, mac, args, arm = _stepper(device, cid, B)
    name, lds = stepper.describe_rollout()
    print(f"{cid}: arm {name}, {lds} B of LDS, B = {B}")
    assert name == arm
    batch, infos = stepper.run(test_mode=True)
    n = check_run(stepper, mac, args, batch, infos, episode=0, test_mode=True, eps=0.0, dtype=F64)
    _cap(cid, "test", n)
    assert stepper.t_env == 0
    stepper.t_env = RS.T_ENV
    batch, infos = stepper.run(test_mode=False)
    n = check_run(stepper, mac, args, batch, infos, episode=1, test_mode=False, eps=RS.EPS_HOME, dtype=F64)
    _cap(cid, "train", n)
    assert n["epsilon_draws"] > 0
    assert stepper.t_env == RS.T_ENV + int(stepper.last_run["ep_len"].sum())


@pytest.mark.parametrize("cid", [c[0] for c in RS.ROLLOUT_CASES])
def test_rollout_shape_parity(device, cid):
    _parity(device, cid)


def test_rollout_shape_parity_single_env(device):
    """B = 1 on the H = 32 v2 arm: one env in a 16-env workgroup."""
    _parity(device, "v2-h32-5v5", B=1)


@pytest.mark.parametrize("cid", [c[0] for c in RS.SELFPLAY_CASES])
def test_selfplay_shape_parity(device, cid):
    stepper, home, away, args, arm = _selfplay(device, cid)
    name, lds = stepper.describe_rollout()
    print(f"{cid}: arm {name}, {lds} B of LDS, B = {RS.B}")
    assert name == arm
    hb, ab, infos = stepper.run(test_mode=True)
    n = check_sides(stepper, (home, away), args, (hb, ab), infos, episode=0, test_mode=True, eps=(0.0, 0.0), dtype=F64)
    _cap(cid, "test", n)
    assert stepper.t_env == 0
    stepper.t_env = RS.T_ENV
    # a different epsilon per side: the away policy is a frozen snapshot with its own selector state
    away.action_selector.schedule.eval = lambda t_env: RS.EPS_AWAY
    hb, ab, infos = stepper.run(test_mode=False)
    eps = (RS.EPS_HOME, RS.EPS_AWAY)
    n = check_sides(stepper, (home, away), args, (hb, ab), infos, episode=1, test_mode=False, eps=eps, dtype=F64)
    _cap(cid, "train", n)
    assert n["epsilon_draws"] > 0
    assert stepper.epsilons == (pytest.approx(RS.EPS_HOME), RS.EPS_AWAY)


# ---- bit-identity between kernels at the new widths and shapes ----------------------------------------------------

def _train_run(stepper, device, kernel, monkeypatch, t_env=RS.T_ENV):
    """One train-mode run from fresh env state under MLG_ROLLOUT_KERNEL=kernel (None: the default arm); the batch(es)
    and the run summary as clones, and the arm that ran."""
    from maleague.envs.teams_env import VecEnvState
    if kernel is None:
        monkeypatch.delenv("MLG_ROLLOUT_KERNEL", raising=False)
    else:
        monkeypatch.setenv("MLG_ROLLOUT_KERNEL", kernel)
    arm = stepper.describe_rollout()[0]
    stepper.envs = VecEnvState(stepper.spec, stepper.batch_size, device)
    stepper.t_env = t_env
    out = stepper.run(test_mode=False)
    batches = [{k: v.clone() for k, v in b.data.transition_data.items()} for b in out[:-1]]
    summary = {k: v.clone() for k, v in stepper.last_run.items() if torch.is_tensor(v)}
    return batches, summary, arm


def _assert_identical(a, b):
    for x, y in zip(a[0], b[0]):
        for k in x:
            assert torch.equal(x[k], y[k]), k
    assert set(a[1]) == set(b[1])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("cid", ["v2-h32-5v5", "v2-h32-7v7", "v2-default-5v7"])
def test_rollout_shape_v2_equals_v1(device, cid, monkeypatch):
    """v2 and v1 compute in the same arithmetic order (test_rollout_v2_equals_v1): the whole batch and the
    run summary of the default arm and of MLG_ROLLOUT_KERNEL=v1 are bit-identical at H = 32 and for unequal teams."""
    stepper, mac, args, arm = _stepper(device, cid)
    default = _train_run(stepper, device, None, monkeypatch)
    v1 = _train_run(stepper, device, "v1", monkeypatch)
    assert default[2] == arm == "v2" and v1[2].startswith("v1-")
    _assert_identical(default, v1)


def test_selfplay_shape_sp2_equals_v1(device, monkeypatch):
    """As test_selfplay_kernel_equals_v1, at H = 32: both batches and the run summary (returns of both sides)."""
    stepper, home, away, args, arm = _selfplay(device, "sp2-h32-5v5")
    default = _train_run(stepper, device, None, monkeypatch)
    v1 = _train_run(stepper, device, "v1", monkeypatch)
    assert default[2] == arm == "sp2" and v1[2].startswith("v1-global")
    assert "away_returns" in default[1]
    _assert_identical(default, v1)


def _test_run(stepper, device, kernel, monkeypatch):
    from maleague.envs.teams_env import VecEnvState
    monkeypatch.setenv("MLG_ROLLOUT_KERNEL", kernel)
    arm = stepper.describe_rollout()[0]
    stepper.envs = VecEnvState(stepper.spec, stepper.batch_size, device)
    out = stepper.run(test_mode=True)
    return [np_batch(b) for b in out[:-1]], stepper.last_run["ep_len"].numpy().copy(), arm


def _fp32_q_and_worst_gap(macs, nbs, ep_len, N):
    """The fp32 oracle's Q along the recorded batches, and the largest amount by which a recorded action falls short
    of the oracle's masked maximum."""
    qs, worst = [], 0.0
    for mac, nb in zip(macs, nbs):
        q = oracle_q(mac, {k: torch.from_numpy(v) for k, v in nb.items()}, N, nb["obs"].shape[1])
        qs.append(q)
        av = nb["avail_actions"].astype(bool)
        for b in range(len(ep_len)):
            for t in range(int(ep_len[b]) + 1):
                qm = np.where(av[b, t], q[b, t], -np.inf)
                chosen = np.take_along_axis(qm, nb["actions"][b, t], axis=-1)[:, 0]
                assert np.isfinite(chosen).all(), (b, t)
                worst = max(worst, float((qm.max(axis=-1) - chosen).max()))
    return qs, worst


def test_rollout_v7_runtime_shape_matches_v2(device, monkeypatch):
    """v7-4v4, as test_rollout_v7_split_bf16_gru_matches_fp32 for a shape that has no compile-time instantiation:
    along v7's own test-mode trajectory every recorded action is an available argmax of the fp32 oracle up to a 1e-5
    tie, and v7 reproduces v2's episodes bit for bit except where a near tie flips an argmax."""
    stepper, mac, args, arm = _stepper(device, "v7-4v4")
    ref, _, arm2 = _test_run(stepper, device, "v2", monkeypatch)
    got, L, arm7 = _test_run(stepper, device, "v7", monkeypatch)
    assert (arm2, arm7) == ("v2", "v7") == ("v2", arm)
    qs, worst = _fp32_q_and_worst_gap((mac,), got, L, args.n_agents)
    assert worst <= 1e-5, worst
    n_diff = assert_near_tie_divergence(ref, got, qs, RS.B)
    print(f"v7 vs v2 [4v4]: {n_diff} of {RS.B} episodes diverge (near-tie flips)")
    assert n_diff <= V7_4V4_MAX_DIVERGING, n_diff


def test_selfplay_sp7_runtime_shape_matches_sp2(device, monkeypatch):
    """sp7-4v4, as test_selfplay_sp7_split_bf16_matches_fp32 for a runtime shape, against sp2."""
    stepper, home, away, args, arm = _selfplay(device, "sp7-4v4")
    ref, _, arm2 = _test_run(stepper, device, "sp2", monkeypatch)
    got, L, arm7 = _test_run(stepper, device, "sp7", monkeypatch)
    assert (arm2, arm7) == ("sp2", "sp7") == ("sp2", arm)
    qs, worst = _fp32_q_and_worst_gap((home, away), got, L, args.n_agents)
    assert worst <= 1e-5, worst
    n_diff = assert_near_tie_divergence(ref, got, qs, RS.B)
    print(f"sp7 vs sp2 [4v4]: {n_diff} of {RS.B} episodes diverge (near-tie flips)")
    assert n_diff <= SP7_4V4_MAX_DIVERGING, n_diff


# ---- the checker itself -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def recorded_run(device):
    """One passing test-mode run of the H = 32 v2 case, copied to the host; shared and never modified."""
    stepper, mac, args, arm = _stepper(device, "v2-h32-5v5")
    batch, infos = stepper.run(test_mode=True)
    nb = np_batch(batch)
    check_run(stepper, mac, args, batch, infos, episode=0, test_mode=True, eps=0.0, dtype=F64, nb=nb)
    for v in nb.values():
        v.setflags(write=False)
    return stepper, mac, args, batch, infos, nb


def test_checker_rejects_a_wrong_greedy_action(recorded_run):
    """One recorded greedy action of the host copy replaced by another available action, at a step whose float64
    Q gap is above Q_TOL: the checker must raise. The step is an episode's last (the action recorded after
    termination, which the env never executes), with its one-hot row changed to match, so the env replay and the
    bookkeeping checks still pass and the failure can only come from the agent-side argmax check."""
    stepper, mac, args, batch, infos, nb = recorded_run
    N = stepper.spec.n_agents
    ep_len = stepper.last_run["ep_len"].numpy()
    q = oracle_q(mac, {k: torch.tensor(nb[k]) for k in ("obs", "actions_onehot")}, N, nb["obs"].shape[1], F64)
    for b, n in ((b, n) for b in range(RS.B) for n in range(N)):
        t = int(ep_len[b])
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
        check_run(stepper, mac, args, batch, infos, episode=0, test_mode=True, eps=0.0, dtype=F64, nb=bad)
    assert f"({b}, {t}, {n}, {wrong}, " in str(exc.value), exc.value  # raised by `assert a == g, (b, t, n, a, g)`


def test_checker_rejects_a_wrong_reward(recorded_run):
    """One reward entry of the host copy changed by the env's smallest reward step (1 / 16): the env replay must
    raise."""
    stepper, mac, args, batch, infos, nb = recorded_run
    assert stepper.last_run["ep_len"][RS.B - 1] > 3
    bad = {k: v.copy() for k, v in nb.items()}
    bad["reward"][RS.B - 1, 3, 0] += np.float32(1.0 / 16)
    with pytest.raises(AssertionError):
        check_run(stepper, mac, args, batch, infos, episode=0, test_mode=True, eps=0.0, dtype=F64, nb=bad)
