"""GPU: mlg_rollout_selfplay_mix (SelfPlayParallelStepper.set_opponent_mix) against plain mlg_rollout_selfplay launches.

The contract (include/maleague.h): env b of a mixture launch runs exactly as env b of the plain self-play launch from
the same MlgEnvState with its group's away policy and roster, so its rows of both EpisodeBatches and its run summary
are bit-identical (torch.equal) to that launch on the same arm family: sp8-mix against sp8, v1-mix against the generic
fp32 kernel (MLG_ROLLOUT_KERNEL=v1). Parity with the float64 / C oracle is inherited through this identity:
tests/test_gpu_selfplay.py and tests/test_gpu_rollout_shapes.py pin mlg_rollout_selfplay to the oracle. Cases, weights
and the early-ending condition on the inputs are tests/mix_shapes.py's.
"""
import numpy as np
import pytest
import torch

import mix_shapes as MS
from helpers import qmix_args, scheme_for

pytestmark = pytest.mark.gpu


def _build(device, plan, H, B, monkeypatch=None, arm=None):
    """A SelfPlayParallelStepper on the mix_shapes env with the home policy loaded, and the [K, n_params] rows of the
    away policies. v1-mix cases run with the generic kernel forced, so that the plain launches are its family."""
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import SelfPlayParallelStepper
    if arm == "v1-mix":
        monkeypatch.setenv("MLG_ROLLOUT_KERNEL", "v1")
    args = qmix_args(batch_size_run=B, seed=MS.SEED, rnn_hidden_dim=H, env_args=MS.env_args(plan),
                     reuse_away_batch=False)
    stepper = SelfPlayParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(dict(info, n_agents=args.n_agents), torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    home, away = BasicMAC(proto.scheme, groups, args), BasicMAC(proto.scheme, groups, args)
    stepper.initialize(scheme, groups, preprocess, home, away)
    away.action_selector.schedule.eval = lambda t_env: MS.EPS_AWAY
    d_in = home.agent.input_shape
    ps = [MS.policy_params(i, d_in, H, args.n_actions) for i in range(MS.N_OPPONENTS + 1)]
    home.agent.load_state_dict({k: torch.as_tensor(v) for k, v in ps[0].items()})
    rows = torch.from_numpy(np.stack([MS.flat_row(p) for p in ps[1:]])).to(device)
    return stepper, away, rows, ps[1:]


def _run(stepper, test_mode, episode):
    """One run from a fresh env state whose episode counters are ``episode``; every output as its own tensor."""
    from maleague.envs.teams_env import VecEnvState
    st = VecEnvState(stepper.spec, stepper.batch_size, stepper.device)
    st.episode.fill_(episode)
    stepper.envs = st
    stepper.t_env = MS.T_ENV
    hb, ab, _ = stepper.run(test_mode=test_mode)
    stepper.flush()
    B = stepper.batch_size
    raw = stepper.last_run_info().clone()
    out = {f"home/{k}": hb[k].clone() for k in hb.data.transition_data}
    out.update({f"away/{k}": ab[k].clone() for k in ab.data.transition_data})
    last = stepper.last_run
    out.update(ep_len=last["ep_len"].clone(), returns=last["returns"].clone(),
               away_returns=last["away_returns"].clone(), won=raw[B:3 * B].view(B, 2).clone(),
               draw=raw[3 * B:4 * B].clone())
    return out


def _plain(stepper, away, params, test_mode, episode, plan=None):
    stepper.set_opponent_mix(None)
    if plan is not None:
        stepper.set_match_build_plan(plan)
    away.agent.load_state_dict({k: torch.as_tensor(v) for k, v in params.items()})
    return _run(stepper, test_mode, episode)


def _mixed(stepper, rows, table, test_mode, episode, plans=None):
    from maleague.steppers import OpponentMix
    stepper.set_opponent_mix(OpponentMix(rows, table, plans))
    return _run(stepper, test_mode, episode)


def _assert_rows_equal(mix, plains, table, B, what):
    """Env b of the mixture equals env b of the plain run of table[b // 16], for every key and summary."""
    for k, envs in MS.group_envs(table, B).items():
        idx = torch.tensor(envs)
        for key, got in mix.items():
            exp = plains[k][key]
            sel = idx.to(got.device)
            assert torch.equal(got[sel], exp[sel]), f"{what}: opponent {k}, {key} differs from the plain launch"


def _assert_early_ends(out, table, B):
    early = (out["ep_len"] < MS.EPISODE_LIMIT).numpy()
    per = {k: int(early[envs].sum()) for k, envs in MS.group_envs(table, B).items()}
    print(f"early ends per opponent: {per}")
    assert sum(per.values()) >= MS.MIN_EARLY, f"inputs: only {sum(per.values())} envs end before the limit"
    assert sum(1 for v in per.values() if v > 0) >= 2, f"inputs: early ends in the groups of one opponent only ({per})"


@pytest.mark.parametrize("cid", [c[0] for c in MS.UNIFORM_CASES])
def test_uniform_mixture_equals_plain_launch(device, monkeypatch, cid):
    """Every group names the same (away, spec): the launch is the plain one, bit for bit, in test and train mode."""
    _, plan, H, B, table, arm = MS.case(cid)
    stepper, away, rows, ps = _build(device, plan, H, B, monkeypatch, arm)
    assert MS.arm_of(stepper.describe_rollout()[0]) == ("sp8" if arm == "sp8-mix" else "v1-global")
    for test_mode, episode in ((True, 0), (False, 1)):
        plain = _plain(stepper, away, ps[1], test_mode, episode)
        mix = _mixed(stepper, rows, [1] * len(table), test_mode, episode)
        assert MS.arm_of(stepper.describe_rollout()[0]) == arm
        for key, got in mix.items():
            assert torch.equal(got, plain[key]), f"{cid} test_mode={test_mode}: {key}"


@pytest.mark.parametrize("cid", [c[0] for c in MS.MIX_CASES])
def test_mixed_table_equals_per_opponent_launches(device, monkeypatch, cid):
    _, plan, H, B, table, arm = MS.case(cid)
    stepper, away, rows, ps = _build(device, plan, H, B, monkeypatch, arm)
    for test_mode, episode in ((True, 0), (False, 1)):
        plains = {k: _plain(stepper, away, ps[k], test_mode, episode) for k in sorted(set(table))}
        mix = _mixed(stepper, rows, table, test_mode, episode)
        assert MS.arm_of(stepper.describe_rollout()[0]) == arm
        if test_mode:
            _assert_early_ends(mix, table, B)
            assert not torch.equal(plains[0]["away/actions"], plains[1]["away/actions"]), "the opponents play alike"
        _assert_rows_equal(mix, plains, table, B, f"{cid} test_mode={test_mode}")
        if cid == "medium_1h_4t-h64" and test_mode:  # determinism: the same state gives the same bits
            again = _mixed(stepper, rows, table, test_mode, episode)
            for key, got in mix.items():
                assert torch.equal(got, again[key]), f"two mixture runs differ in {key}"


@pytest.mark.parametrize("B", [1, 16])
@pytest.mark.parametrize("arm", ["sp8-mix", "v1-mix"])
def test_single_group_batches(device, monkeypatch, B, arm):
    """B = 1 and B = 16: one group, partly and exactly full."""
    stepper, away, rows, ps = _build(device, "small", 64, B, monkeypatch, arm)
    for test_mode, episode in ((True, 0), (False, 1)):
        plain = _plain(stepper, away, ps[2], test_mode, episode)
        mix = _mixed(stepper, rows, [2], test_mode, episode)
        assert MS.arm_of(stepper.describe_rollout()[0]) == arm
        for key, got in mix.items():
            assert torch.equal(got, plain[key]), f"B={B} {arm} test_mode={test_mode}: {key}"


def test_rosters_per_group(device):
    """Three composed away teams at the 5v5 shape: each group plays its opponent's roster (the group specs differ) and
    equals the plain launch after set_match_build_plan."""
    from maleague.league.teams import compose_league_teams, match_plan
    teams = compose_league_teams(5, 4, "HEALER", "RANGED", seed=4)
    assert len({t.codes() for t in teams}) == 4
    plans = [match_plan(teams[0], t) for t in teams[1:]]
    B, table = 48, [0, 1, 2]
    stepper, away, rows, ps = _build(device, plans[0], 64, B)
    for test_mode, episode in ((True, 0), (False, 1)):
        plains = {k: _plain(stepper, away, ps[k], test_mode, episode, plan=plans[k]) for k in range(3)}
        stepper.set_match_build_plan(plans[0])
        mix = _mixed(stepper, rows, table, test_mode, episode, plans=plans)
        assert stepper.describe_rollout()[0] == "sp8-mix"
        specs = stepper._mix["specs"]
        assert len({(tuple(s.role), tuple(s.melee)) for s in specs}) == 3, "the group specs do not differ"
        _assert_rows_equal(mix, plains, table, B, f"rosters test_mode={test_mode}")


@pytest.mark.parametrize("arm", ["sp8-mix", "v1-mix"])
def test_ring_and_full_write_modes(device, monkeypatch, arm):
    """Home episodes written into replay slots pre-filled with other bytes and wrapping the ring's end, away episodes
    into the reused away batch on a second run whose table differs from the first: both equal runs into
    zero-initialised batches."""
    from maleague.components.replay_buffer import ReplayBuffer
    B, T1 = 37, MS.EPISODE_LIMIT + 1
    stepper, away, rows, _ = _build(device, "small", 64, B, monkeypatch, arm)
    info = dict(stepper.get_env_info(), n_agents=stepper.args.n_agents)
    scheme, groups, preprocess = scheme_for(info, torch)
    ring = ReplayBuffer(scheme, groups, 50, T1, preprocess=preprocess, device=device)
    for v in ring.data.transition_data.values():
        v.fill_(7)
    tables = ([0, 1, 2], [2, 0, 1])
    for it, table in enumerate(tables):  # run 1 starts at slot 37 of 50: its 37 slots wrap the ring's end
        stepper._ring = None
        stepper.args.reuse_away_batch = False
        plain = _mixed(stepper, rows, table, False, it)
        assert stepper.attach_replay(ring)
        stepper.args.reuse_away_batch = True
        slot0 = ring.buffer_index
        got = _mixed(stepper, rows, table, False, it)
        assert MS.arm_of(stepper.describe_rollout()[0]) == arm
        assert slot0 == it * B and (it == 0 or slot0 + B > 50)
        for key, exp in plain.items():
            assert torch.equal(got[key], exp), f"{arm} run {it}: {key}"
        assert torch.equal(stepper._away_extent.cpu(), (got["ep_len"] + 1).to(torch.int32))
        ring.insert_episode_batch(stepper.home_batch)
