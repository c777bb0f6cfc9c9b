"""GPU parity of the cross-play evaluation kernel (mlg_crossplay_rollout, CrossPlayEvaluator, evaluate_pool).

The oracle is the existing fp32 self-play kernel (mlg_rollout_selfplay forced to the generic v1 kernel with
MLG_ROLLOUT_KERNEL=v1, test mode, st.episode = episode0, fresh batches), one run per pair through
SelfPlayParallelStepper: ep_len, won, draw and both returns of every env must be EXACTLY equal.

Policies are flat parameter vectors drawn on the CPU (uniform in [-SCALE, SCALE], one torch.Generator per seed), so
they are the same on every machine. The grid is 6 x 6: the spawn columns of the two teams overlap, units are within
range from the first step and games are decided inside 30 steps. SCALE / the seeds of the plain-plan case were picked
on the CPU oracle (oracle/env_ref.c + learner_ref.drqn_forward greedy policies: 7 distinct episode lengths and 16
decided games over the 9 pairs); the guard itself is asserted on the GPU oracle's output.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from helpers import qmix_args, scheme_for

pytestmark = pytest.mark.gpu

GRID, SCALE, ENV_SEED = 6, 0.3, 5


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _args(plan, episode_limit, H=64, B=20):
    from maleague.envs.plans import builtin_plan
    mbp = builtin_plan(plan, self_play=True) if isinstance(plan, str) else plan
    return qmix_args(batch_size_run=B, seed=ENV_SEED, rnn_hidden_dim=H,
                     env_args={"match_build_plan": mbp, "grid_size": GRID, "stochastic_spawns": True,
                               "episode_limit": episode_limit})


def _n_params(H, d_in, A):
    return H * d_in + H + 6 * H * H + 6 * H + A * H + A


def _pool(seeds, n_params):
    rows = []
    for s in seeds:
        g = torch.Generator().manual_seed(s)
        rows.append((torch.rand(n_params, generator=g) * 2 - 1) * SCALE)
    return torch.stack(rows)


def _stepper(device, args):
    """A self-play stepper with two MACs (the oracle's plumbing, as tests/test_gpu_selfplay.py builds it)."""
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import SelfPlayParallelStepper
    stepper = SelfPlayParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(dict(info, n_agents=args.n_agents), torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    home, away = BasicMAC(proto.scheme, groups, args), BasicMAC(proto.scheme, groups, args)
    stepper.initialize(scheme, groups, preprocess, home, away)
    stepper.args.reuse_away_batch = False  # fresh zero-initialised batches for every run
    return stepper, home, away


def _oracle(device, args, pool, pairs, plans, E, episode0):
    """One v1 self-play run per pair: {ep_len [n, E], won [n, E, 2], draw, ret, ret_away} as numpy arrays."""
    from maleague.envs.teams_env import VecEnvState
    from maleague.runs.sp_ma_experiment import load_agent_vector
    assert args.batch_size_run == E
    out = {k: [] for k in ("ep_len", "won", "draw", "ret", "ret_away")}
    with _env(MLG_ROLLOUT_KERNEL="v1"):
        stepper, home, away = _stepper(device, args)
        for h, a, s in pairs:
            if plans[s] is not None:
                stepper.set_match_build_plan(plans[s])
            load_agent_vector(home, pool[h])
            load_agent_vector(away, pool[a])
            stepper.envs = VecEnvState(stepper.spec, E, device)
            stepper.envs.episode.fill_(episode0)
            stepper.run(test_mode=True)
            stepper.flush()
            torch.cuda.synchronize()
            info = stepper.last_run_info().cpu().numpy().copy()
            out["ep_len"].append(info[0:E])
            out["won"].append(info[E:3 * E].reshape(E, 2))
            out["draw"].append(info[3 * E:4 * E])
            out["ret"].append(info[4 * E:5 * E])       # float32 bits
            out["ret_away"].append(info[5 * E:6 * E])  # float32 bits
    return {k: np.stack(v) for k, v in out.items()}


def _assert_exact(last, ref):
    """Per-env outputs of the evaluation launch against the oracle, bit for bit (returns compared as bits)."""
    got = {k: last[k].cpu().numpy() for k in ("ep_len", "won", "draw", "ret", "ret_away")}
    for k in ("ep_len", "won", "draw"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    for k in ("ret", "ret_away"):
        np.testing.assert_array_equal(got[k].view(np.int32), ref[k], err_msg=k)


def _dims(args, spec):
    nh, A = spec.n_agents // 2, spec.n_actions
    return nh, A, 8 * spec.U + A + nh


@pytest.fixture(scope="module")
def plain(device):
    """The plain-plan case: plan small, episode_limit 30, H = 64, three policies, all 9 pairs, E = 20, episode0 = 3
    (one full and one partial workgroup per pair). The oracle runs once for the module."""
    from maleague.league.evaluation import CrossPlayEvaluator, build_pairs
    args = _args("small", 30)
    ev = CrossPlayEvaluator(args, device, episodes_per_launch=20)
    nh, A, d_in = _dims(args, ev.spec_of(None))
    pool = _pool((41, 42, 43), _n_params(64, d_in, A)).to(device)
    table = build_pairs(range(3), range(3))
    ref = _oracle(device, _args("small", 30), pool, table.pairs.tolist(), table.plans, 20, 3)
    return {"args": args, "ev": ev, "pool": pool, "table": table, "ref": ref}


def test_oracle_guard_games_differ(plain):
    """Asserted on the oracle's output only: the 9 pairs are not 180 copies of one trivial game."""
    ref = plain["ref"]
    print("oracle ep_len values", sorted(set(ref["ep_len"].ravel().tolist())), "decided",
          int((ref["won"][..., 0] != ref["won"][..., 1]).sum()))
    assert len(set(ref["ep_len"].ravel().tolist())) >= 3
    assert ((ref["won"][..., 0] != ref["won"][..., 1]) & (ref["draw"] == 0)).any()


@pytest.mark.parametrize("rows", ["lds", "workspace"])
def test_bit_parity_plain_plan(plain, rows):
    """All 9 pairs in one launch equal 9 v1 self-play runs exactly; with the step's obs / avail rows in LDS and, forced
    by MLG_CROSSPLAY_OBS_WORKSPACE=1, in the per-workgroup workspace slices (the path of shapes whose rows do not fit)."""
    ev = plain["ev"]
    with _env(MLG_CROSSPLAY_OBS_WORKSPACE="1" if rows == "workspace" else None):
        res = ev.evaluate(plain["pool"], plain["table"], 20, episode0=3)
    _assert_exact(ev.last, plain["ref"])
    assert res.games.tolist() == [[20.0] * 3] * 3
    # a different episode counter is a different set of games
    ev.evaluate(plain["pool"], plain["table"], 20, episode0=4)
    assert not np.array_equal(ev.last["ep_len"].cpu().numpy(), plain["ref"]["ep_len"])


def test_summary_reduction(plain):
    """summary[pair] = the documented fixed-order sums of the per-env outputs (torch.equal, counts exact), bitwise
    identical over two calls; the tables of the result are those sums per cell."""
    ev, n, E = plain["ev"], 9, 20
    ev.evaluate(plain["pool"], plain["table"], E, episode0=3)
    last = {k: v.cpu().clone() for k, v in ev.last.items() if torch.is_tensor(v)}
    res = ev.evaluate(plain["pool"], plain["table"], E, episode0=3)
    assert torch.equal(ev.last["summary"].cpu(), last["summary"])
    w0, w1 = last["won"][..., 0] != 0, last["won"][..., 1] != 0
    dr = (last["draw"] != 0) | (w0 == w1)
    want = torch.zeros(n, 8)
    want[:, 0] = E
    want[:, 1] = (~dr & w0).sum(1)
    want[:, 2] = (~dr & ~w0).sum(1)
    want[:, 3] = dr.sum(1)
    want[:, 6] = last["ep_len"].sum(1)

    def fixed_order(x):  # lane l adds envs l, l + 64, ... ascending from 0; then lanes 0..63 ascending from 0
        part = torch.zeros(n, 64)
        for e in range(x.shape[1]):
            part[:, e % 64] = part[:, e % 64] + x[:, e]
        tot = torch.zeros(n)
        for lane in range(64):
            tot = tot + part[:, lane]
        return tot
    want[:, 4], want[:, 5] = fixed_order(last["ret"]), fixed_order(last["ret_away"])
    assert torch.equal(last["summary"], want)
    assert torch.equal(res.games, want[:, 0].view(3, 3)) and torch.equal(res.wins, want[:, 1].view(3, 3))
    assert torch.equal(res.wins + res.losses + res.draws, res.games)
    assert torch.equal(res.mean_return_home, (want[:, 4] / E).view(3, 3))
    # episodes beyond one launch: launch k plays episode counter episode0 + k, the rows add up
    ev2 = type(ev)(plain["args"], ev.device, episodes_per_launch=12)
    two = ev2.evaluate(plain["pool"], plain["table"], E, episode0=3)
    assert ev2.launches == 2 and two.games.tolist() == [[20.0] * 3] * 3
    assert torch.equal(two.wins + two.losses + two.draws, two.games)


def test_per_pair_rosters(device):
    """Two composed 5-unit teams x two policies: 4 pairs, 4 distinct (home roster, away roster) specs through
    spec_idx, each exactly the v1 self-play run configured with match_plan(home, away)."""
    from maleague.league.evaluation import CrossPlayEvaluator, build_pairs
    from maleague.league.teams import compose_league_teams, match_plan
    teams = compose_league_teams(5, 2, "HEALER", "RANGED", seed=0)
    assert len({t.codes() for t in teams}) == 2
    table = build_pairs([0, 1], [0, 1], lambda pid: teams[pid])
    assert len(table.plans) == 4 and sorted(table.pairs[:, 2].tolist()) == [0, 1, 2, 3]
    E = 24
    args = _args(match_plan(teams[0], teams[0]), 30, B=E)
    ev = CrossPlayEvaluator(args, device, episodes_per_launch=E)
    nh, A, d_in = _dims(args, ev.spec_of(table.plans[0]))
    pool = _pool((7, 8), _n_params(64, d_in, A)).to(device)
    ref = _oracle(device, _args(match_plan(teams[0], teams[0]), 30, B=E), pool, table.pairs.tolist(), table.plans, E, 1)
    ev.evaluate(pool, table, E, episode0=1)
    _assert_exact(ev.last, ref)
    # the rosters matter: the same two policies play different games on different rosters
    assert not np.array_equal(ref["ret"][0], ref["ret"][1]) or not np.array_equal(ref["ep_len"][0], ref["ep_len"][1])


def test_h32_second_plan(device):
    """H = 32 on medium_1h_4t (5v5 with a healer): one pair, E = 16, exact."""
    from maleague.league.evaluation import CrossPlayEvaluator, build_pairs
    args = _args("medium_1h_4t", 30, H=32, B=16)
    ev = CrossPlayEvaluator(args, device, episodes_per_launch=16)
    nh, A, d_in = _dims(args, ev.spec_of(None))
    pool = _pool((3, 4), _n_params(32, d_in, A)).to(device)
    table = build_pairs([0], [1])
    ref = _oracle(device, _args("medium_1h_4t", 30, H=32, B=16), pool, table.pairs.tolist(), table.plans, 16, 0)
    ev.evaluate(pool, table, 16, episode0=0)
    _assert_exact(ev.last, ref)


def test_pool_packing_equals_pack_agent(device):
    """mlg_pack_agent_pool rows (P = 3: two rows of a strided `current` tensor, one row of a `historical` tensor)
    are bitwise mlg_pack_agent of the same parameters."""
    from maleague import _native
    from maleague.controllers import BasicMAC
    from maleague.league.evaluation import CrossPlayEvaluator
    from maleague.runs.sp_ma_experiment import load_agent_vector
    args = _args("small", 30)
    stepper, home, _ = _stepper(device, args)
    assert isinstance(home, BasicMAC)
    ev = CrossPlayEvaluator(args, device)
    dims = ev.dims_of(ev.spec_of(None))
    n = _n_params(64, dims.d_in, dims.n_actions)
    flat = _pool((1, 2, 3), n).to(device)
    buf = torch.full((2, n + 8), 9.0, device=device)  # rows with a stride wider than the parameters
    current = buf[:, :n]
    current.copy_(flat[:2])
    historical = torch.empty(4, n, device=device)
    historical[2].copy_(flat[2])
    psize = int(_native.load().mlg_packed_agent_size(_native.byref(dims)))
    packed = torch.zeros(3, psize, device=device)
    stream = _native.stream_ptr(device)
    _native.call("mlg_pack_agent_pool", _native.byref(dims), current.data_ptr(), current.stride(0), 2, packed.data_ptr(),
                 stream)
    _native.call("mlg_pack_agent_pool", _native.byref(dims), historical[2:].data_ptr(), historical.stride(0), 1,
                 packed[2:].data_ptr(), stream)
    for p in range(3):
        load_agent_vector(home, flat[p])
        assert torch.equal(packed[p], home.agent.packed()), p
    with pytest.raises(_native.NativeError, match="row_stride"):
        _native.call("mlg_pack_agent_pool", _native.byref(dims), current.data_ptr(), n - 1, 2, packed.data_ptr(), stream)


def test_league_instance_evaluate_pool(device):
    """Single rank, 2 players + 1 stored snapshot, E = 16, episode_limit 20: a 3 x 3 table with E games per cell that
    leaves the training payoff, its local delta and the home parameters untouched."""
    from maleague.custom_logging import MainLogger
    from maleague.league import DistributedLeague, LeagueInstance, PayoffEntry
    from maleague.league.teams import compose_league_teams
    from maleague.runs.sp_ma_experiment import agent_vector
    from maleague.utils.config import build_config, to_args
    cfg = build_config("qmix", "ma", overrides=["batch_size_run=16", "runner=parallel", "buffer_cpu_only=False",
                                                "buffer_size=64", "env_args.episode_limit=20",
                                                f"env_args.grid_size={GRID}", "t_max=1000000000",
                                                "test_interval=100000000"])
    teams = compose_league_teams(5, 2, "HEALER", "RANGED", seed=1)
    lg = DistributedLeague(n_players=2, device=device, max_historical=3, player_id=1)
    logger = MainLogger()
    inst = LeagueInstance(to_args(cfg), logger, lg, mode="rolebased", role=["main", "main_exploiter"], seed=1,
                          teams=teams)
    home = agent_vector(inst.experiment.home_mac)
    lg.set_player_params(0, home.clone() * 0.5)
    assert lg.exchange(home, 10, checkpoint=True) == [(2, 1)]  # pid 2: a snapshot of player 1
    lg.record(1, 0, PayoffEntry.WIN, n=3)
    lg.sync_payoff()
    lg.record(1, 2, PayoffEntry.DRAW, n=2)
    payoff0, delta0, home0 = lg.payoff.tensor.clone(), lg._delta.clone(), home.clone()
    res = inst.evaluate_pool(16)
    torch.cuda.synchronize()
    assert res.games.shape == (3, 3) and (res.games == 16).all()
    assert torch.equal(res.wins + res.losses + res.draws, res.games)
    for t in (res.win_rate, res.mean_return_home, res.mean_return_away, res.mean_ep_len, res.jpc_matrix):
        assert t.shape == (3, 3) and torch.isfinite(t).all()
    assert ((res.mean_ep_len >= 1) & (res.mean_ep_len <= 20)).all()
    # pid 2 is a copy of pid 1 with its parent's roster: same games against everybody, as home and as away
    assert torch.equal(res.totals[1], res.totals[2]) and torch.equal(res.totals[:, 1], res.totals[:, 2])
    assert torch.equal(lg.payoff.tensor, payoff0) and torch.equal(lg._delta, delta0)
    assert torch.equal(agent_vector(inst.experiment.home_mac), home0)
    logged = logger.stats["league_eval_win_rate_mean"]
    assert [t for t, _ in logged] == [0, 1, 2]
    assert [v for _, v in logged] == pytest.approx(res.win_rate.mean(1).tolist())
    sub = inst.evaluate_pool(16, pids=[2, 0])
    assert torch.equal(sub.totals[0, 1], res.totals[2, 0]) and torch.equal(sub.totals[1, 0], res.totals[0, 2])
    with pytest.raises(KeyError):
        inst.evaluate_pool(16, pids=[0, 3])


def test_validation_refuses_without_launch(plain):
    """An out-of-range pool index, a spec with one policy team and specs that disagree on U are refused with a message
    and nothing is launched (the output tensors keep their contents)."""
    from maleague import _native
    from maleague.envs.plans import builtin_plan
    from maleague.league.evaluation import PairTable, build_pairs
    ev, pool = plain["ev"], plain["pool"]
    ev.evaluate(pool, plain["table"], 20, episode0=3)
    before = {k: v.clone() for k, v in ev.last.items() if torch.is_tensor(v)}
    launches = ev.launches

    def refused(table, word):
        with pytest.raises(_native.NativeError, match=word):
            ev.evaluate(pool, table, 20, episode0=9)
        torch.cuda.synchronize()
        assert ev.launches == launches
        for k, v in before.items():
            assert torch.equal(ev.last[k], v), k

    refused(build_pairs([0, 3], [0, 1]), "out of the pool's range")
    one = build_pairs([0], [1])
    refused(PairTable(one.pairs, one.cells, one.shape, [builtin_plan("small", self_play=False)]), "n_policy_teams")
    two = build_pairs([0, 1], [0])
    two.pairs[1, 2] = 1
    refused(PairTable(two.pairs, two.cells, two.shape, [None, builtin_plan("medium", self_play=True)]), r"\.U=")


def test_league_main_evaluates_after_the_last_iteration(tmp_path, capsys):
    """league/main.py --league_eval_episodes=N (in process, one main player and its snapshots): evaluate_pool runs once
    after the last league iteration and its tables land in the summary; without the key nothing is evaluated."""
    from maleague.league.main import main
    argv = ["--device=0", "--config=qmix", "--env-config=ma", "--league-config=matchmaking", "--experiment=alphastar",
            "--league_size=1", "--main_exploiters_n=0", "--team_size=5", "--league-iterations=2", "--match-iterations=1",
            "--pretrain-iterations=0", "--runner=parallel", "--batch_size_run=64", "--env_args.episode_limit=20",
            f"--env_args.grid_size={GRID}", "--buffer_size=128", "--league_checkpoint_min_steps=1",
            "--league_checkpoint_max_steps=1", f"--local_results_path={tmp_path}", "--show_exp_parameters=False"]
    tail = ["force-unit", "--role=HEALER", "--attack=RANGED"]
    s = main(argv + ["--league_eval_episodes=8"] + tail)
    capsys.readouterr()
    ev = s["league_eval"]
    n = 1 + s["historical_snapshots"]
    assert s["historical_snapshots"] >= 1 and ev["pids"] == list(range(n)) and ev["episodes"] == 8
    assert np.array(ev["games"]).shape == (n, n) and (np.array(ev["games"]) == 8).all()
    assert np.isfinite(np.array(ev["win_rate"])).all() and np.array(ev["mean_ep_len"]).max() <= 20
    games = sum(s["payoff"][i][j][0] for i in range(n) for j in range(n))
    assert games == 2 * 64  # the training payoff holds the training games only
    assert "league_eval" not in main(argv + tail)


@pytest.mark.parametrize("H,per_side", [(128, 3), (64, 9), (32, 13)])
def test_other_widths_and_tile_counts(device, H, per_side):
    """The remaining kernel variants v1 self-play accepts, one pair, E = 16, exact: H = 128; 9 and 13 agents per side
    (3 and 4 agent tiles per wave). One step of 16 envs of the two larger shapes does not fit LDS (170 KB / 353 KB of
    obs rows), so they run with the rows in the workspace without being forced to."""
    from maleague import _native
    from maleague.envs.plans import team_from_codes
    from maleague.league.evaluation import CrossPlayEvaluator, build_pairs
    plan = [team_from_codes(" ".join(["TR", "AR", "HR"][k % 3] for k in range(per_side)), False) for _ in range(2)]
    args = _args(plan, 12, H=H, B=16)
    ev = CrossPlayEvaluator(args, device, episodes_per_launch=16)
    spec = ev.spec_of(None)
    nh, A, d_in = _dims(args, spec)
    assert nh == per_side
    ws = _native.load().mlg_crossplay_workspace_floats(_native.byref(ev.dims_of(spec)), 1, 16)
    assert (ws > 4) == (per_side > 3)
    pool = _pool((5, 6), _n_params(H, d_in, A)).to(device)
    table = build_pairs([0], [1])
    ref = _oracle(device, _args(plan, 12, H=H, B=16), pool, table.pairs.tolist(), table.plans, 16, 2)
    ev.evaluate(pool, table, 16, episode0=2)
    _assert_exact(ev.last, ref)


def test_jpc_run_trains_then_fills_the_matrix(device):
    """JointPolicyCorrelationEvaluationRun.start(): two short self-play instances trained in turn, then ONE evaluate
    call for the 2 x 2 (home of i, away of j) pairs; jpc_matrix = home + away mean return per pair."""
    from maleague.custom_logging import MainLogger
    from maleague.runs import JointPolicyCorrelationEvaluationRun
    from maleague.utils.config import build_config, to_args
    cfg = build_config("qmix", "ma", overrides=["batch_size_run=16", "runner=parallel", "buffer_cpu_only=False",
                                                "buffer_size=64", "batch_size=16", "env_args.episode_limit=20",
                                                f"env_args.grid_size={GRID}", "test_interval=100000000",
                                                "show_exp_parameters=False"])
    run = JointPolicyCorrelationEvaluationRun(to_args(cfg), MainLogger(), instances_num=2, eval_episodes=8)
    run.start()
    assert all(len(p) == 2 and p[0].is_cuda and p[0].shape == p[1].shape for p in run.policies)
    assert not torch.equal(run.policies[0][0], run.policies[1][0])  # independent instances
    r = run.result
    assert (r.games == 8).all() and torch.equal(r.wins + r.losses + r.draws, r.games)
    assert run.jpc_matrix.shape == (2, 2) and run.jpc_matrix.dtype == torch.float32
    assert torch.isfinite(run.jpc_matrix).all()
    assert torch.equal(run.jpc_matrix, (r.mean_return_home + r.mean_return_away).to(torch.float32))
