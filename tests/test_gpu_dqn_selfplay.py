"""GPU parity of the feed-forward agent (agent: dqn) in self-play, the league and cross-play: mlg_rollout_selfplay_ff per
dispatch arm and edge (cases: tests/dqn_selfplay_shapes.py) by the method of tests/test_gpu_selfplay.py with the float64
feed-forward oracle (tests/dqn_ref.py), mlg_ff_pack_pool against mlg_ff_pack, mlg_crossplay_rollout_ff against one
test-mode self-play launch per pair, and the experiment and league layers.

Rollout: both sides' env tensors bit-exact against the C env under teacher forcing, random picks those of the counter
RNG (stream index = global agent index, one epsilon per side), every greedy pick the float64 oracle's argmax except at
a near tie (top-two masked Q within 1e-4), near ties accepted for at most 1 % of a case's greedy picks.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dqn_selfplay_shapes as FSP
import helpers
from helpers import qmix_args, scheme_for, shape_plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NEAR_TIE_CAP = 0.01


@pytest.fixture
def ff_oracle(monkeypatch):
    """helpers.check_sides with the feed-forward oracle in place of the DRQN's, as tests/test_gpu_dqn.py does:
    dqn_ref.oracle_q with the input flags of the case (dqn_selfplay_shapes.oracle_q; with both flags on it is
    dqn_ref.oracle_q). check_sides reads nothing else of the MACs."""
    monkeypatch.setattr(helpers, "oracle_q", FSP.oracle_q)


def _build(device, args, cls=None):
    """A SelfPlayFFParallelStepper over ``args`` with two feed-forward BasicMACs on the device."""
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import SelfPlayFFParallelStepper
    stepper = (cls or SelfPlayFFParallelStepper)(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(dict(info, n_agents=args.n_agents), torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    macs = [BasicMAC(proto.scheme, groups, args) for _ in range(2)]
    return stepper, macs, (scheme, groups, preprocess)


def _stepper(device, cid, B=FSP.B, cls=None):
    """The case's stepper: home weights dqn_ref.agent_params(seed), away weights seeded apart."""
    _, hidden, plan, la, ai, arm, seed, scale = FSP.case(cid)
    args = qmix_args(batch_size_run=B, seed=seed, rnn_hidden_dim=hidden, obs_last_action=la, obs_agent_id=ai,
                     agent="dqn", env_args={"match_build_plan": shape_plan(plan, self_play=True), "grid_size": 20,
                                            "stochastic_spawns": True, "episode_limit": FSP.EPISODE_LIMIT})
    stepper, macs, sch = _build(device, args, cls)
    for mac, ps in zip(macs, FSP.side_params(macs[0].input_shape, hidden, args.n_actions, seed, scale)):
        mac.agent.load_state_dict({k: torch.from_numpy(v) for k, v in ps.items()})
        mac.agent.to(device)
    macs[1].action_selector.schedule.eval = lambda t_env: FSP.EPS_AWAY  # a frozen snapshot with its own selector state
    stepper.initialize(*sch, macs[0], macs[1])
    return stepper, macs, args, arm


def _cap(cid, mode, n):
    print(f"{cid} [{mode}]: {n}  ({100.0 * n['near_ties'] / n['greedy']:.3f} % near ties, cap 1 %)")
    assert n["near_ties"] <= NEAR_TIE_CAP * n["greedy"], (cid, mode, n)


# ---- 1. parity per case ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", FSP.IDS)
def test_rollout_selfplay_ff_parity(device, cid, ff_oracle, monkeypatch):
    monkeypatch.delenv("MLG_ROLLOUT_GLOBAL_WEIGHTS", raising=False)
    stepper, macs, args, arm = _stepper(device, cid)
    name, lds = stepper.describe_rollout()
    print(f"{cid}: arm {name}, {lds} B of LDS, B = {FSP.B}, nh = {args.n_agents}")
    assert name == arm
    hb, ab, infos = stepper.run(test_mode=True)
    n = helpers.check_sides(stepper, macs, args, (hb, ab), infos, episode=0, test_mode=True, eps=(0.0, 0.0), dtype=F64)
    _cap(cid, "test", n)
    assert stepper.t_env == 0
    stepper.t_env = FSP.T_ENV
    hb, ab, infos = stepper.run(test_mode=False)
    n = helpers.check_sides(stepper, macs, args, (hb, ab), infos, episode=1, test_mode=False,
                            eps=(FSP.EPS, FSP.EPS_AWAY), dtype=F64)
    _cap(cid, "train", n)
    assert n["epsilon_draws"] > 0
    assert stepper.epsilons == (pytest.approx(FSP.EPS), FSP.EPS_AWAY)
    assert stepper.t_env == FSP.T_ENV + int(stepper.last_run["ep_len"].sum())


# ---- 2. the two arms, and two launches, bit for bit -----------------------------------------------------------------

def _snapshot(stepper, batches):
    """Everything a run stores: both batches, ep_len, both returns, won and draw."""
    stepper.flush()
    torch.cuda.synchronize()
    B = stepper.batch_size
    out = {f"{side}.{k}": v.detach().cpu().clone() for side, b in zip(("home", "away"), batches)
           for k, v in b.data.transition_data.items()}
    info = stepper.last_run_info().cpu().clone()
    out["ep_len"], out["won"], out["draw"] = info[0:B], info[B:3 * B], info[3 * B:4 * B]
    out["returns"] = stepper.last_run["returns"].clone()
    out["away_returns"] = stepper.last_run["away_returns"].clone()
    assert torch.equal(out["ep_len"], stepper.last_run["ep_len"].to(out["ep_len"].dtype))
    return out


def _two_runs(stepper, device, B=FSP.B):
    """A test-mode run of episode 0 and a train-mode run of episode 1 from fresh env state, as snapshots."""
    from maleague.envs.teams_env import VecEnvState
    stepper.args.reuse_away_batch = False
    snaps = []
    for episode, test_mode in ((0, True), (1, False)):
        st = VecEnvState(stepper.spec, B, device)
        st.episode.fill_(episode)
        stepper.envs = st
        stepper.t_env = FSP.T_ENV
        hb, ab, _ = stepper.run(test_mode=test_mode)
        snaps.append(_snapshot(stepper, (hb, ab)))
    return snaps


@pytest.mark.parametrize("cid,forced", FSP.LDS_VS_GLOBAL, ids=[c for c, _ in FSP.LDS_VS_GLOBAL])
def test_lds_arm_equals_forced_global_arm(device, cid, forced, monkeypatch):
    """The arms differ in where a weight is read from, not in the order of any sum: both batches and the run info of a
    test-mode and a train-mode run are byte-identical under MLG_ROLLOUT_GLOBAL_WEIGHTS; and so are two launches of the
    same arm from the same state."""
    monkeypatch.delenv("MLG_ROLLOUT_GLOBAL_WEIGHTS", raising=False)
    stepper, macs, args, arm = _stepper(device, cid)
    assert stepper.describe_rollout()[0] == arm and arm.startswith("ffsp-lds")
    lds = _two_runs(stepper, device)
    again = _two_runs(stepper, device)
    monkeypatch.setenv("MLG_ROLLOUT_GLOBAL_WEIGHTS", "1")
    assert stepper.describe_rollout()[0] == forced
    glob = _two_runs(stepper, device)
    for want, same, got in zip(lds, again, glob):
        assert int(want["ep_len"].min()) >= 1 and set(got) == set(want)
        for k in want:
            assert torch.equal(same[k], want[k]), (cid, "two launches", k)
            assert torch.equal(got[k], want[k]), (cid, "lds vs global", k)
    assert not torch.equal(lds[1]["home.actions"], lds[1]["away.actions"])  # each side drew with its own epsilon


# ---- 3. ring mode ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", FSP.RING_CASES)
def test_ring_mode_equals_plain_run(device, cid, monkeypatch):
    """Home episodes written straight into replay slots pre-filled with other bytes (full-write mode, wrapping around
    the ring's end), and away episodes written in full-write mode into the reused, pre-filled away batch, equal the
    plain run into zero-initialised batches bit for bit; slot extents follow."""
    from maleague.components.replay_buffer import ReplayBuffer
    from maleague.envs.teams_env import VecEnvState
    monkeypatch.delenv("MLG_ROLLOUT_GLOBAL_WEIGHTS", raising=False)
    stepper, macs, args, arm = _stepper(device, cid)
    assert stepper.describe_rollout()[0] == arm
    info = dict(stepper.get_env_info(), n_agents=args.n_agents)
    scheme, groups, preprocess = scheme_for(info, torch)
    size, T1 = FSP.B + 5, FSP.EPISODE_LIMIT + 1
    ring = ReplayBuffer(scheme, groups, size, T1, preprocess=preprocess, device=device)
    for v in ring.data.transition_data.values():
        v.fill_(7)
    for it in range(2):  # slots 0..36, then 37..41 and 0..31 (wraps)
        runs = []
        for use_ring in (False, True):
            st = VecEnvState(stepper.spec, FSP.B, device)
            st.episode.fill_(it)
            stepper.envs = st
            stepper.t_env = FSP.T_ENV
            stepper._ring = None
            stepper.args.reuse_away_batch = use_ring  # plain: fresh zero-initialised away batch per run
            if use_ring:
                assert stepper.attach_replay(ring)
                if stepper._away_buf is not None:  # written from outside: every row unknown again
                    for v in stepper._away_buf.data.transition_data.values():
                        v.fill_(7)
                    stepper._away_extent.fill_(T1)
            hb, ab, _ = stepper.run(test_mode=False)
            stepper.flush()
            runs.append(({k: hb[k].clone() for k in hb.data.transition_data},
                         {k: ab[k].clone() for k in ab.data.transition_data}, hb))
        plain, ringed = runs
        for side in (0, 1):
            for k in plain[side]:
                assert torch.equal(plain[side][k], ringed[side][k]), (cid, it, side, k)
        hr = ringed[2]
        ring.insert_episode_batch(hr)
        slots = (torch.arange(FSP.B) + hr.slot0) % size
        want = (stepper.last_run["ep_len"] + 1).to(torch.int32)
        assert torch.equal(ring.slot_extent.cpu()[slots], want), (cid, it)
        assert torch.equal(stepper._away_extent.cpu(), want), (cid, it)


# ---- 4. B = 1 -------------------------------------------------------------------------------------------------------

def test_single_env_stepper(device, ff_oracle, monkeypatch):
    """B = 1 through SelfPlayFFStepper: nh live rows in the first tile of either side of the one workgroup."""
    from maleague.steppers import SelfPlayFFStepper
    monkeypatch.delenv("MLG_ROLLOUT_GLOBAL_WEIGHTS", raising=False)
    stepper, macs, args, arm = _stepper(device, "ffsp-n3-h64", B=1, cls=SelfPlayFFStepper)
    assert stepper.describe_rollout()[0] == arm
    hb, ab, env_info = stepper.run(test_mode=True)
    assert set(env_info) == {"battle_won", "draw"}
    helpers.check_sides(stepper, macs, args, (hb, ab), [env_info], episode=0, test_mode=True, eps=(0.0, 0.0),
                        dtype=F64)
    a, b = _two_runs(stepper, device, B=1), _two_runs(stepper, device, B=1)
    for x, y in zip(a, b):
        for k in x:
            assert torch.equal(x[k], y[k]), k


# ---- 5. mlg_ff_pack_pool --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,pad", [(1, 0), (3, 0), (3, 5)], ids=["p1", "p3", "p3-strided"])
def test_ff_pack_pool_equals_ff_pack(device, P, pad):
    """P rows packed in one launch are, bit for bit, P calls of mlg_ff_pack on the same parameters; also with a row
    stride above the parameter count, the padding columns holding NaN."""
    from maleague import _native
    spec = FSP.spec_of("medium_1h_4t")
    for hidden, la, ai in ((64, True, True), (32, False, True), (128, True, False)):
        d = FSP.dims_of(spec, hidden, la, ai)
        H, A, d_in = hidden, d.n_actions, d.d_in
        sizes = [H * d_in, H, A * H, A]
        n_params = sum(sizes)
        g = torch.Generator().manual_seed(7 + P)
        flat = torch.full((P, n_params + pad), float("nan"))
        flat[:, :n_params] = torch.rand(P, n_params, generator=g) * 2 - 1
        flat = flat.to(device)
        psize = int(_native.load().mlg_ff_packed_size(_native.byref(d)))
        got = torch.full((P, psize), float("nan"), device=device)
        _native.call("mlg_ff_pack_pool", _native.byref(d), flat.data_ptr(), int(flat.stride(0)), P, got.data_ptr(),
                     _native.stream_ptr(device))
        for p in range(P):
            parts = [t.contiguous() for t in torch.split(flat[p, :n_params], sizes)]
            want = torch.full((psize,), float("nan"), device=device)
            _native.call("mlg_ff_pack", _native.byref(d), _native.byref(_native.MlgFFParams(*[t.data_ptr() for t in parts])),
                         want.data_ptr(), _native.stream_ptr(device))
            torch.cuda.synchronize()
            assert not torch.isnan(want).any()
            assert torch.equal(got[p].view(torch.int32), want.view(torch.int32)), (hidden, la, ai, p)


# ---- 6. cross-play --------------------------------------------------------------------------------------------------

CP_GRID, CP_SCALE, CP_SEED = 6, 0.3, 5  # tests/test_gpu_crossplay.py's: games are decided inside 30 steps


def _cp_args(plan, H, B):
    return qmix_args(batch_size_run=B, seed=CP_SEED, rnn_hidden_dim=H, agent="dqn",
                     env_args={"match_build_plan": plan, "grid_size": CP_GRID, "stochastic_spawns": True,
                               "episode_limit": FSP.EPISODE_LIMIT})


@pytest.mark.parametrize("plan,H,two_rosters", FSP.CROSSPLAY_CASES,
                         ids=[f"{p}-h{h}" for p, h, _ in FSP.CROSSPLAY_CASES])
def test_crossplay_ff_equals_per_pair_launches(device, plan, H, two_rosters, monkeypatch):
    """A pool of 3 feed-forward policies, all 9 ordered pairs, E = 20 (one full and one partial workgroup per pair),
    episode counter 3: ep_len, ret, ret_away, won and draw of mlg_crossplay_rollout_ff bit-identical to nine test-mode
    mlg_rollout_selfplay_ff launches; the summary rows are the documented fixed-order sums; with
    MLG_CROSSPLAY_OBS_WORKSPACE=1 (the rows in the workspace) the same bits. On the 3v3 plan the pairs alternate between
    two rosters of the spec table."""
    from maleague.envs.teams_env import VecEnvState
    from maleague.league.evaluation import FFCrossPlayEvaluator, PairTable, build_pairs
    from maleague.runs.sp_ma_experiment import agent_vector, load_agent_vector
    monkeypatch.delenv("MLG_ROLLOUT_GLOBAL_WEIGHTS", raising=False)
    monkeypatch.delenv("MLG_CROSSPLAY_OBS_WORKSPACE", raising=False)
    E, P, ep0 = FSP.CROSSPLAY_E, FSP.CROSSPLAY_POOL, FSP.CROSSPLAY_EPISODE0
    base = shape_plan(plan, self_play=True)
    stepper, macs, sch = _build(device, _cp_args(base, H, E))
    for m in macs:
        m.cuda()
    stepper.initialize(*sch, *macs)
    stepper.args.reuse_away_batch = False
    n_params = sum(p.numel() for p in macs[0].agent.parameters())
    rows = []
    for s in range(P):
        g = torch.Generator().manual_seed(41 + s)
        rows.append((torch.rand(n_params, generator=g) * 2 - 1) * CP_SCALE)
    pool = torch.stack(rows).to(device)
    table = build_pairs(range(P), range(P))
    plans = [None]
    if two_rosters:  # pair k plays roster k % 2: the env config's own plan, or the TR AR HR mirror
        plans = [None, shape_plan("3v3", self_play=True)]
        pairs = table.pairs.clone()
        pairs[:, 2] = torch.arange(P * P, dtype=torch.int32) % 2
        table = PairTable(pairs, table.cells, table.shape, plans)
    ref = {k: [] for k in ("ep_len", "won", "draw", "ret", "ret_away")}
    for h, a, s in table.pairs.tolist():
        stepper.set_match_build_plan(plans[s] if plans[s] is not None else base)
        load_agent_vector(macs[0], pool[h])
        load_agent_vector(macs[1], pool[a])
        assert torch.equal(agent_vector(macs[1]), pool[a])
        stepper.envs = VecEnvState(stepper.spec, E, device)
        stepper.envs.episode.fill_(ep0)
        stepper.run(test_mode=True)
        stepper.flush()
        torch.cuda.synchronize()
        info = stepper.last_run_info().cpu().numpy().copy()
        ref["ep_len"].append(info[0:E])
        ref["won"].append(info[E:3 * E].reshape(E, 2))
        ref["draw"].append(info[3 * E:4 * E])
        ref["ret"].append(info[4 * E:5 * E])       # float32 bits
        ref["ret_away"].append(info[5 * E:6 * E])  # float32 bits
    ref = {k: np.stack(v) for k, v in ref.items()}
    # asserted on the self-play launches' output only: the pairs do not all play the games of pair 0 (the policy
    # indices are read)
    assert any(not np.array_equal(ref["ret"][0], ref["ret"][k]) or
               not np.array_equal(ref["ret_away"][0], ref["ret_away"][k]) for k in range(1, P * P))
    # the summary: the reduction of the per-env results in the documented fixed order
    n = P * P
    w0, w1 = ref["won"][..., 0] != 0, ref["won"][..., 1] != 0
    dr = (ref["draw"] != 0) | (w0 == w1)
    want = np.zeros((n, 8), np.float32)
    want[:, 0] = E
    want[:, 1], want[:, 2], want[:, 3] = (~dr & w0).sum(1), (~dr & ~w0).sum(1), dr.sum(1)
    want[:, 6] = ref["ep_len"].sum(1)
    for col, key in ((4, "ret"), (5, "ret_away")):
        tot = np.zeros(n, np.float32)
        for e in range(E):  # E <= 64: one env per lane, lanes added in ascending order from 0
            tot = (tot + ref[key][:, e].view(np.float32)).astype(np.float32)
        want[:, col] = tot
    for workspace in (False, True):
        if workspace:
            monkeypatch.setenv("MLG_CROSSPLAY_OBS_WORKSPACE", "1")
        ev = FFCrossPlayEvaluator(_cp_args(base, H, E), device, episodes_per_launch=E)
        res = ev.evaluate(pool, table, E, episode0=ep0)
        assert (ev._buf["workspace"].numel() > 4) == workspace
        got = {k: ev.last[k].cpu().numpy() for k in ref}
        for k in ("ep_len", "won", "draw"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{k} workspace={workspace}")
        for k in ("ret", "ret_away"):
            np.testing.assert_array_equal(got[k].view(np.int32), ref[k], err_msg=f"{k} workspace={workspace}")
        np.testing.assert_array_equal(ev.last["summary"].cpu().numpy(), want)
        assert res.games.tolist() == [[float(E)] * P] * P
        assert torch.equal(res.wins + res.losses + res.draws, res.games)
    print(f"{plan} H={H}: episode lengths per pair {[(int(x.min()), int(x.max())) for x in ref['ep_len']]}, "
          f"decided {int((~dr).sum())} of {n * E}")


# ---- 7. experiment and league ---------------------------------------------------------------------------------------

LG_B, LG_LIMIT = 32, 20


def _league_args(seed=1, **kw):
    from maleague.utils.config import build_config, to_args
    over = {"agent": "dqn", "batch_size_run": LG_B, "batch_size": LG_B, "buffer_size": LG_B,
            "runner": "parallel", "buffer_cpu_only": False, "env_args.episode_limit": LG_LIMIT,
            "env_args.match_build_plan": "small", "t_max": 1000000, "test_interval": 100000000,
            "learner_log_interval": 0, "show_exp_parameters": False, "seed": seed,
            "league_checkpoint_min_steps": 2000000000, "league_checkpoint_max_steps": 4000000000}
    over.update(kw)
    return to_args(build_config("qmix", "ma", overrides=[f"{k}={v}" for k, v in over.items()]))


def test_selfplay_experiment_trains_home_only(device):
    """SelfPlayMultiAgentExperiment with --config=qmix agent=dqn on 3v3, 8 envs, four iterations: the stepper is the
    feed-forward one, the home parameters move, the away parameters do not, the learner's statistics are finite."""
    from maleague.custom_logging import MainLogger
    from maleague.envs.plans import builtin_plan
    from maleague.modules.agents import DQNAgentNetwork
    from maleague.runs.sp_ma_experiment import SelfPlayMultiAgentExperiment, agent_vector
    from maleague.steppers import SelfPlayFFParallelStepper
    args = _league_args(seed=3, batch_size_run=8, batch_size=8, buffer_size=16)
    args.env_args = dict(args.env_args, match_build_plan=builtin_plan("small", self_play=True))
    np.random.seed(0)
    torch.manual_seed(0)
    exp = SelfPlayMultiAgentExperiment(args, MainLogger(log_interval=10 ** 12))
    assert type(exp.stepper) is SelfPlayFFParallelStepper
    assert isinstance(exp.home_mac.agent, DQNAgentNetwork) and isinstance(exp.away_mac.agent, DQNAgentNetwork)
    assert exp.args.n_agents == 3 and exp.args.total_n_agents == 6
    home0, away0 = agent_vector(exp.home_mac).clone(), agent_vector(exp.away_mac).clone()
    assert not torch.equal(home0, away0)
    exp.start(max_iterations=4)
    torch.cuda.synchronize()
    assert exp.stepper.describe_rollout()[0] == "ffsp-lds/tpw1"
    assert exp.home_learner.train_calls == 4 and exp.stepper.t_env > 0
    assert not torch.equal(agent_vector(exp.home_mac), home0), "the home agent did not train"
    assert torch.equal(agent_vector(exp.away_mac), away0), "the frozen away agent changed"
    stats = exp.home_learner.last_stats
    assert stats and all(np.isfinite(v) for v in stats.values()), stats
    h, a = exp.evaluate_mean_returns(episode_n=1)
    assert torch.isfinite(h) and torch.isfinite(a)


def test_league_instance_with_feed_forward_agents(device):
    """Player 1 of a two-player league with composed 3-unit teams (player 0 a fixed replica): after sync the away MAC
    holds the opponent's vector bit for bit and the pool rows are the four tensors flat; two syncs and plays book B games
    per iteration into the payoff and move the home agent; evaluate_pool equals a direct FFCrossPlayEvaluator.evaluate
    over the league's pool."""
    from maleague.custom_logging import MainLogger
    from maleague.league import DistributedLeague, LeagueInstance, PayoffEntry, league_instance_for
    from maleague.league.evaluation import FFCrossPlayEvaluator, build_pairs
    from maleague.league.teams import compose_league_teams
    from maleague.modules.agents import DQNAgentNetwork
    from maleague.runs.sp_ma_experiment import agent_vector
    from maleague.steppers import SelfPlayFFParallelStepper
    torch.manual_seed(1)
    np.random.seed(1)
    teams = compose_league_teams(3, 2, "HEALER", "RANGED", seed=1)
    lg = DistributedLeague(n_players=2, device=device, max_historical=2, player_id=1)
    inst = league_instance_for(_league_args(), MainLogger(log_interval=10 ** 12), lg, mode="rolebased",
                               role=["main", "main_exploiter"], seed=1, teams=teams)
    ex = inst.experiment
    assert type(inst) is LeagueInstance and type(ex.stepper) is SelfPlayFFParallelStepper
    assert isinstance(ex.home_mac.agent, DQNAgentNetwork) and isinstance(ex.away_mac.agent, DQNAgentNetwork)
    assert ex.stepper.describe_rollout()[0] == "ffsp-lds/tpw1"
    H, A, d_in = ex.args.rnn_hidden_dim, ex.args.n_actions, ex.home_mac.input_shape
    n_params = H * d_in + H + A * H + A
    assert agent_vector(ex.home_mac).numel() == n_params
    opp = (agent_vector(ex.home_mac).clone() * 0.5).contiguous()
    lg.set_player_params(0, opp)
    home0 = agent_vector(ex.home_mac).clone()
    for it in range(2):
        assert inst.sync() == (0, False)
        assert tuple(lg.current.shape) == (2, n_params) and lg.historical.shape[1] == n_params
        assert torch.equal(agent_vector(ex.away_mac), opp) and torch.equal(lg.params_of(0), opp)
        assert torch.equal(lg.params_of(1), agent_vector(ex.home_mac))
        inst.play(2)
    lg.sync_payoff()
    torch.cuda.synchronize()
    pay = lg.payoff.tensor.cpu()
    assert float(pay[1, 0, PayoffEntry.GAMES]) == 4 * LG_B  # the envs played
    assert float(pay[1, 0, PayoffEntry.WIN:PayoffEntry.DRAW + 1].sum()) == 4 * LG_B
    assert ex.home_learner.train_calls == 4 and ex.home_mac.agent.trained_steps > 0
    assert not torch.equal(agent_vector(ex.home_mac), home0)
    assert torch.equal(agent_vector(ex.away_mac), opp), "the frozen away MAC changed"
    res = inst.evaluate_pool(20)
    assert type(inst._evaluator) is FFCrossPlayEvaluator
    assert tuple(res.games.shape) == (2, 2) and float(res.games.sum()) == 80.0
    assert torch.equal(res.wins + res.losses + res.draws, res.games)
    assert torch.isfinite(res.jpc_matrix).all() and (res.mean_ep_len >= 1).all() and (res.mean_ep_len <= LG_LIMIT).all()
    direct = FFCrossPlayEvaluator(ex.args, device).evaluate([lg.current, lg.historical],
                                                            build_pairs([0, 1], [0, 1], inst.team_of), 20)
    assert torch.equal(direct.totals, res.totals)


def test_pretrain_vs_ai_hands_over_the_feed_forward_agent(device):
    """One pre-training iteration against the mirrored scripted AI (mlg_rollout_ff, the fused learner's feed-forward
    branch): the league experiment's home MAC then holds the pre-trained agent."""
    from maleague.custom_logging import MainLogger
    from maleague.league import DistributedLeague, league_instance_for
    from maleague.runs.sp_ma_experiment import agent_vector
    torch.manual_seed(2)
    np.random.seed(2)
    lg = DistributedLeague(n_players=1, device=device, max_historical=1)
    inst = league_instance_for(_league_args(seed=2), MainLogger(log_interval=10 ** 12), lg, mode="matchmaking", seed=2)
    home0 = agent_vector(inst.experiment.home_mac).clone()
    inst.pretrain_vs_ai(iterations=1)
    assert not torch.equal(agent_vector(inst.experiment.home_mac), home0)
    assert inst.sync() is not None and inst.opponent == 0
    assert torch.equal(agent_vector(inst.experiment.away_mac), lg.params_of(0))


def test_league_main_dqn_single_rank(tmp_path):
    """league/main.py --config=qmix agent=dqn, one rank: pre-training against the scripted AI (mlg_rollout_ff), two
    league iterations of two matches (mlg_rollout_selfplay_ff), the final cross-play evaluation
    (mlg_crossplay_rollout_ff); ends cleanly and prints the payoff."""
    iters, per_match = 2, 2
    cmd = [sys.executable, os.path.join(ROOT, "ma-league_amd", "maleague", "league", "main.py"), "--device=0",
           "--config=qmix", "--env-config=ma", "--league-config=matchmaking", "--experiment=matchmaking",
           "--league_size=1", "--team_size=3", f"--league-iterations={iters}", f"--match-iterations={per_match}",
           "--pretrain-iterations=1", "--runner=parallel", "--agent=dqn",
           f"--batch_size_run={LG_B}", f"--batch_size={LG_B}", f"--buffer_size={LG_B}",
           f"--env_args.episode_limit={LG_LIMIT}", "--league_eval_episodes=4", f"--local_results_path={tmp_path}"]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:] + p.stdout[-2000:]
    s = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert s["league_iterations"] == iters and [m["iterations"] for m in s["matches"][0]] == [per_match] * iters
    pay = s["payoff"]
    assert sum(pay[0][j][0] for j in range(len(pay[0]))) == iters * per_match * LG_B
    assert s["league_eval"]["games"] == [[4.0]]
    assert "Stats for Team #" in p.stdout and "Win [" in p.stdout
