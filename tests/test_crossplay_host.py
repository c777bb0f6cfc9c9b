"""Host side of the league cross-play evaluation (maleague.league.evaluation, runs.jpc_eval_run): CPU only."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import qmix_args


def _teams(k=3, seed=2):
    from maleague.league.teams import compose_league_teams
    teams = compose_league_teams(5, k, "HEALER", "RANGED", seed=seed)
    assert len({t.codes() for t in teams}) == k
    return teams


def test_build_pairs_order_and_no_teams_case():
    from maleague.league.evaluation import build_pairs
    t = build_pairs([0, 1, 4], [4, 0])
    assert t.shape == (3, 2) and len(t) == 6
    # home-major, pool rows are the pids themselves, one mirrored spec
    assert t.pairs.tolist() == [[0, 4, 0], [0, 0, 0], [1, 4, 0], [1, 0, 0], [4, 4, 0], [4, 0, 0]]
    assert t.cells.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [2, 0], [2, 1]]
    assert t.plans == [None]
    assert t.pairs.dtype == torch.int32 and not t.pairs.is_cuda


def test_build_pairs_deduplicates_specs():
    from maleague.league.evaluation import build_pairs
    from maleague.league.teams import match_plan
    teams = _teams(2)
    # pids 0, 1 players with their own team; pid 2 a snapshot of player 0 (same roster as 0)
    team_of = lambda pid: teams[0] if pid in (0, 2) else teams[1]  # noqa: E731
    t = build_pairs([0, 1, 2], [0, 1, 2], team_of)
    spec = t.pairs[:, 2].reshape(3, 3)
    # four distinct (home roster, away roster) plans, numbered in order of first use
    assert spec.tolist() == [[0, 1, 0], [2, 3, 2], [0, 1, 0]]
    assert len(t.plans) == 4
    assert t.plans[1] == match_plan(teams[0], teams[1]) and t.plans[2] == match_plan(teams[1], teams[0])
    assert t.plans[0] == match_plan(teams[0], teams[0])


def test_aggregate_hand_made_summary():
    from maleague.league.evaluation import aggregate, build_pairs
    t = build_pairs([0, 1], [0, 1])
    #            games wins losses draws ret_h  ret_a  ep_len  0
    s = torch.tensor([[4., 1., 2., 1., 8.0, 4.0, 40., 0.],
                      [4., 4., 0., 0., 20.0, 2.0, 20., 0.],
                      [4., 0., 4., 0., 1.0, 30.0, 24., 0.],
                      [4., 0., 0., 4., 6.0, 6.0, 80., 0.]])
    r = aggregate(s, t, (2, 2))
    assert r.games.tolist() == [[4, 4], [4, 4]]
    assert r.wins.tolist() == [[1, 4], [0, 0]] and r.losses.tolist() == [[2, 0], [4, 0]]
    assert r.draws.tolist() == [[1, 0], [0, 4]]
    assert torch.equal(r.wins + r.losses + r.draws, r.games)
    assert r.mean_return_home.tolist() == [[2.0, 5.0], [0.25, 1.5]]
    assert r.mean_return_away.tolist() == [[1.0, 0.5], [7.5, 1.5]]
    assert r.mean_ep_len.tolist() == [[10.0, 5.0], [6.0, 20.0]]
    assert r.win_rate.tolist() == [[0.375, 1.0], [0.0, 0.5]]
    assert r.jpc_matrix.tolist() == [[3.0, 5.5], [7.75, 3.0]]
    assert float(r.avg_proportional_loss()) == pytest.approx((3.0 - 6.625) / 3.0)
    # rows of a repeated pair (several launches / ranks) add up; an untouched cell has no games and win rate 0.5
    twice = aggregate(torch.cat([s[:2], s[:2]]), torch.tensor([[0, 0, 0], [0, 1, 0], [0, 0, 0], [0, 1, 0]]), (2, 2))
    assert twice.games.tolist() == [[8, 8], [0, 0]] and twice.wins.tolist() == [[2, 8], [0, 0]]
    assert twice.win_rate[1].tolist() == [0.5, 0.5] and twice.mean_ep_len[1].tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        aggregate(s, t, (2, 1))


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_rank_partition_covers_every_pair_once(world):
    from maleague.league.evaluation import aggregate, build_pairs
    t = build_pairs(range(5), range(5))
    seen = []
    totals = torch.zeros(5, 5, 8)
    for r in range(world):
        part = t[r::world]
        assert part.shape == t.shape and part.plans is t.plans
        seen += [tuple(c) for c in part.cells.tolist()]
        s = torch.zeros(len(part), 8)
        s[:, 0] = 3
        totals += aggregate(s, part, part.shape).totals  # what the all_reduce sums
    assert sorted(seen) == sorted(tuple(c) for c in t.cells.tolist()) and len(set(seen)) == 25
    assert (totals[..., 0] == 3).all()


def test_avg_proportional_loss_matches_reference_golden(golden):
    from maleague.league.evaluation import avg_proportional_loss
    g = golden("jpc.npz")
    n = int(g["n"])
    assert n >= 4
    seen_negative = seen_raise = False
    for k in range(n):
        m = torch.from_numpy(g[f"jpc_{k}"])
        if bool(g[f"raises_{k}"]):
            seen_raise = True
            with pytest.raises(NotImplementedError):
                avg_proportional_loss(m)
            continue
        v = avg_proportional_loss(m)
        assert np.float32(float(v)) == g[f"apl_{k}"], k
        seen_negative |= float(v) < 0  # off-diagonal mean greater than the diagonal mean
    assert seen_negative and seen_raise


def test_jpc_run_constructs_with_reference_attributes():
    from maleague.custom_logging import MainLogger
    from maleague.runs import EVAL_REGISTRY, JointPolicyCorrelationEvaluationRun
    assert EVAL_REGISTRY["jpc"] is JointPolicyCorrelationEvaluationRun
    args = qmix_args(t_max=10 ** 6)
    logger = MainLogger()
    run = JointPolicyCorrelationEvaluationRun(args, logger, instances_num=3, eval_episodes=7)
    assert run.args is args and run.args.t_max == 200 and run.logger is logger
    assert run.instances_num == 3 and run.eval_episodes == 7
    assert run.policies == [tuple()] * 3
    assert run.jpc_matrix.shape == (3, 3) and run.jpc_matrix.dtype == torch.float32 and not run.jpc_matrix.any()
    assert callable(run.start) and callable(run.train_instances) and callable(run.evaluate_instances)
    d = JointPolicyCorrelationEvaluationRun(qmix_args(), logger)
    assert d.instances_num == 2 and d.eval_episodes == 100
    # every instance trains the config's policy team against its mirror, with its own seed
    a1 = run._instance_args(1)
    assert a1.seed == args.seed + 1 and [t["is_scripted"] for t in a1.env_args["match_build_plan"]] == [False, False]


def test_evaluate_without_gpu_raises_native_error():
    from maleague import _native
    from maleague.league.evaluation import CrossPlayEvaluator, build_pairs
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    ev = CrossPlayEvaluator(qmix_args(device="cpu"), "cpu")
    with pytest.raises(_native.NativeError):
        ev.evaluate(torch.zeros(2, 8), build_pairs([0, 1], [0, 1]), 4)


def test_evaluator_specs_and_dims_follow_the_env_config():
    """Host-side plumbing of the evaluator: the mirrored two-policy spec, one side's agent dims, the shared seed."""
    from maleague.league.evaluation import CrossPlayEvaluator
    from maleague.league.teams import match_plan
    args = qmix_args(device="cpu", seed=11, league_eval_seed=4)
    ev = CrossPlayEvaluator(args, "cpu", episodes_per_launch=32)
    spec = ev.spec_of(None)
    assert spec.n_policy_teams == 2 and spec.U == 10 and spec.n_agents == 10 and spec.seed == 4
    assert spec.role[:5] == spec.role[5:]
    d = ev.dims_of(spec)
    assert (d.d_obs, d.n_actions, d.n_agents, d.hidden, d.d_in) == (80, 15, 5, 64, 80 + 15 + 5)
    teams = _teams(2)
    sp = ev.spec_of(match_plan(teams[0], teams[1]))
    assert sp.U == 10 and sp.role[:5] == [u["role"].value["id"] for u in teams[0].units]
    assert CrossPlayEvaluator(SimpleNamespace(**{**vars(args), "league_eval_seed": None}), "cpu").spec_of(None).seed == 11


def _host_call(specs, pairs, n_pool=3, E=8, hidden=64):
    """mlg_crossplay_rollout with valid HOST tables and never-dereferenced device pointers: the host checks run (and
    must refuse) before anything is launched, so this needs no GPU."""
    import ctypes
    from maleague import _native
    lib = _native.load()
    cs = (_native.MlgEnvSpec * len(specs))(*[s.to_c() for s in specs])
    cp = (_native.MlgCrossplayPair * len(pairs))(*[_native.MlgCrossplayPair(*p) for p in pairs])
    s0 = specs[0]
    nh, A = max(s0.n_agents // 2, 1), s0.n_actions
    dims = _native.MlgAgentDims(d_obs=8 * s0.U, n_actions=A, n_agents=nh, hidden=hidden, d_in=8 * s0.U + A + nh,
                                obs_last_action=1, obs_agent_id=1)
    fake = 0x10000  # 16-byte aligned, never read on a refused call
    c = _native.MlgCrossplay(fake, n_pool, len(pairs), fake, ctypes.addressof(cp), fake, ctypes.addressof(cs),
                             len(specs), E, 0, fake, 1 << 40, fake, fake, fake, fake, fake, fake)
    rc = lib.mlg_crossplay_rollout(_native.byref(dims), _native.byref(c), None)
    return rc, lib.mlg_last_error().decode()


def _spec(plan="small", self_play=True, **env):
    from maleague.envs.plans import builtin_plan
    from maleague.envs.teams_env import TeamsEnvSpec
    return TeamsEnvSpec.from_env_args({"match_build_plan": builtin_plan(plan, self_play=self_play), "grid_size": 20,
                                       "episode_limit": 30, "seed": 3, **env})


def test_host_validation_refuses_before_any_launch():
    """No GPU is needed to be refused: every check below fails on the host copies of the tables."""
    if torch.cuda.is_available():
        pytest.skip("GPU present (the same refusals are checked there through the evaluator)")
    ok = _spec()
    for bad_pair, word in (((3, 0, 0), "pool"), ((0, -1, 0), "pool"), ((0, 1, 1), "spec")):
        rc, msg = _host_call([ok], [(0, 1, 0), bad_pair])
        assert rc != 0 and "pairs[1]" in msg and word in msg, msg
    rc, msg = _host_call([ok, _spec(self_play=False)], [(0, 1, 0)])
    assert rc != 0 and "n_policy_teams" in msg and "specs[1]" in msg, msg
    rc, msg = _host_call([ok, _spec("medium")], [(0, 1, 0)])
    assert rc != 0 and ".U=" in msg and "specs[1]" in msg, msg
    for key, kw in (("episode_limit", {"episode_limit": 31}), ("grid", {"grid_size": 24}), ("seed", {"seed": 4}),
                    ("stochastic", {"stochastic_spawns": False})):
        rc, msg = _host_call([ok, _spec(**kw)], [(0, 1, 0)])
        assert rc != 0 and key in msg, (key, msg)
    rc, msg = _host_call([ok], [(0, 1, 0)], hidden=48)
    assert rc != 0 and "rnn_hidden_dim" in msg, msg


def test_workspace_floats_is_host_only(monkeypatch):
    from maleague import _native
    lib = _native.load()
    monkeypatch.delenv("MLG_CROSSPLAY_OBS_WORKSPACE", raising=False)
    d = _native.MlgAgentDims(d_obs=80, n_actions=15, n_agents=5, hidden=64, d_in=100, obs_last_action=1, obs_agent_id=1)
    assert lib.mlg_crossplay_workspace_floats(_native.byref(d), 64, 512) == 4  # one step of 5v5 fits LDS
    # rows forced into the workspace: one step per workgroup, 16 envs x 10 agents x (84 obs floats + 15 avail ints)
    monkeypatch.setenv("MLG_CROSSPLAY_OBS_WORKSPACE", "1")
    assert lib.mlg_crossplay_workspace_floats(_native.byref(d), 9, 20) == 9 * 2 * (16 * 10 * 84 + 16 * 10 * 15)
    monkeypatch.delenv("MLG_CROSSPLAY_OBS_WORKSPACE")
    # 25v25 (the `large` plan): one step of 16 envs x 50 agents x 404 floats is past the LDS of a CU
    big = _native.MlgAgentDims(d_obs=400, n_actions=55, n_agents=25, hidden=64, d_in=480, obs_last_action=1,
                               obs_agent_id=1)
    assert lib.mlg_crossplay_workspace_floats(_native.byref(big), 2, 16) == 2 * (16 * 50 * 404 + 16 * 50 * 55)
    bad = _native.MlgAgentDims(d_obs=81, n_actions=15, n_agents=5, hidden=64, d_in=101, obs_last_action=1,
                               obs_agent_id=1)
    assert lib.mlg_crossplay_workspace_floats(_native.byref(bad), 1, 16) == -1 and b"d_obs" in lib.mlg_last_error()
    assert lib.mlg_crossplay_workspace_floats(_native.byref(d), 0, 16) == -1
