"""GPU parity of distinct per-agent networks in self-play, the league and cross-play: mlg_rollout_selfplay_distinct per
dispatch arm and edge (cases: tests/distinct_selfplay_shapes.py) by the method of tests/test_gpu_selfplay.py with the
per-agent float64 oracle (tests/distinct_ref.py), mlg_crossplay_rollout_distinct against one test-mode self-play launch
per pair, and DistinctLeagueInstance through the Python layers.

Rollout: both sides' env tensors bit-exact against the C env under teacher forcing, random picks those of the counter
RNG (stream index = global agent index, one epsilon per side), every greedy pick the float64 oracle's argmax except at
a near tie (top-two masked Q within 1e-4), near ties accepted for at most 1 % of a case's greedy picks. With nh equal
networks per side a run stores, bit for bit, what two BasicMACs store on the generic fp32 kernel.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distinct_ref as DR
import distinct_selfplay_shapes as DSP
import helpers
from helpers import qmix_args, scheme_for, shape_plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NEAR_TIE_CAP = 0.01


@pytest.fixture
def distinct_oracle(monkeypatch):
    """helpers.check_sides with the per-agent oracle in place of the shared DRQN's (its env replay and pick rules as
    is; check_sides reads nothing else of the MACs)."""
    monkeypatch.setattr(helpers, "oracle_q", DR.oracle_q)


def _stepper(device, cid, B=DSP.B, shared=False, cls=None):
    """A SelfPlayDistinctParallelStepper over the case's plan with two DistinctMACs: nh different seeded networks per
    side, the away side seeded apart, or (shared) nh copies of each side's network 0."""
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import DistinctMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import SelfPlayDistinctParallelStepper
    _, hidden, plan, la, arm, seed, scale = DSP.case(cid)
    args = qmix_args(batch_size_run=B, seed=seed, rnn_hidden_dim=hidden, obs_last_action=la, obs_agent_id=False,
                     mac="distinct", env_args={"match_build_plan": shape_plan(plan, self_play=True), "grid_size": 20,
                                               "stochastic_spawns": True, "episode_limit": DSP.EPISODE_LIMIT})
    stepper = (cls or SelfPlayDistinctParallelStepper)(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(dict(info, n_agents=args.n_agents), torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    macs = [DistinctMAC(proto.scheme, groups, args) for _ in range(2)]
    sides = DSP.side_params(args.n_agents, macs[0].input_shape, hidden, args.n_actions, seed, scale)
    for mac, ps in zip(macs, sides):
        DR.load_agents(mac, [ps[0]] * args.n_agents if shared else ps)
        mac.cuda()
    macs[1].action_selector.schedule.eval = lambda t_env: DSP.EPS_AWAY  # a frozen snapshot with its own selector state
    stepper.initialize(scheme, groups, preprocess, macs[0], macs[1])
    return stepper, macs, args, arm, sides


def _cap(cid, mode, n):
    print(f"{cid} [{mode}]: {n}  ({100.0 * n['near_ties'] / n['greedy']:.3f} % near ties, cap 1 %)")
    assert n["near_ties"] <= NEAR_TIE_CAP * n["greedy"], (cid, mode, n)


# ---- 1. parity per case ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", DSP.IDS)
def test_rollout_selfplay_distinct_parity(device, cid, distinct_oracle):
    stepper, macs, args, arm, _ = _stepper(device, cid)
    name, lds = stepper.describe_rollout()
    print(f"{cid}: arm {name}, {lds} B of LDS, B = {DSP.B}, nh = {args.n_agents}")
    assert name == arm
    hb, ab, infos = stepper.run(test_mode=True)
    n = helpers.check_sides(stepper, macs, args, (hb, ab), infos, episode=0, test_mode=True, eps=(0.0, 0.0), dtype=F64)
    _cap(cid, "test", n)
    assert stepper.t_env == 0
    stepper.t_env = DSP.T_ENV
    hb, ab, infos = stepper.run(test_mode=False)
    n = helpers.check_sides(stepper, macs, args, (hb, ab), infos, episode=1, test_mode=False,
                            eps=(DSP.EPS, DSP.EPS_AWAY), dtype=F64)
    _cap(cid, "train", n)
    assert n["epsilon_draws"] > 0
    assert stepper.epsilons == (pytest.approx(DSP.EPS), DSP.EPS_AWAY)
    assert stepper.t_env == DSP.T_ENV + int(stepper.last_run["ep_len"].sum())


# ---- 2. equal networks, bit for bit ---------------------------------------------------------------------------------

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


@pytest.mark.parametrize("cid", DSP.SHARED_CASES)
def test_equal_networks_equal_two_basic_macs_on_the_generic_kernel(device, cid, monkeypatch):
    """All of a side's nh networks hold that side's one weight set: a test-mode and a train-mode run store, bit for
    bit, what a SelfPlayParallelStepper with two BasicMACs (obs_agent_id off) of those weights stores under
    MLG_ROLLOUT_KERNEL=v1 -- both batches, ep_len, both returns, won and draw. A row's arithmetic is agent_device.h's in
    both tilings (an MFMA column depends on its own row only)."""
    monkeypatch.setenv("MLG_ROLLOUT_KERNEL", "v1")
    _, hidden, plan, la, arm, seed, _ = DSP.case(cid)
    stepper, macs, args, _, sides = _stepper(device, cid, shared=True)
    ref_stepper, ref_home, ref_away, ref_args = helpers.build_selfplay(
        device, plan=shape_plan(plan, self_play=True), B=DSP.B, episode_limit=DSP.EPISODE_LIMIT, seed=seed,
        rnn_hidden_dim=hidden, obs_agent_id=False, obs_last_action=la)
    for mac, ps in zip((ref_home, ref_away), sides):
        mac.agent.load_state_dict({k: torch.from_numpy(v) for k, v in ps[0].items()})
        mac.agent.to(device)
    ref_away.action_selector.schedule.eval = lambda t_env: DSP.EPS_AWAY
    assert ref_stepper.describe_rollout()[0].startswith("v1-") and stepper.describe_rollout()[0] == arm
    for test_mode in (True, False):
        snaps = []
        for st in (stepper, ref_stepper):
            if not test_mode:
                st.t_env = DSP.T_ENV
            hb, ab, _ = st.run(test_mode=test_mode)
            snaps.append(_snapshot(st, (hb, ab)))
        got, want = snaps
        assert int(want["ep_len"].min()) >= 1 and set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), (cid, test_mode, k)
        if not test_mode:  # the two sides drew with their own epsilons: the batches are not copies of each other
            assert not torch.equal(want["home.actions"], want["away.actions"])


# ---- 3. ring mode ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", DSP.RING_CASES)
def test_ring_mode_equals_plain_run(device, cid):
    """Home episodes written straight into replay slots pre-filled with other bytes (full-write mode, wrapping around
    the ring's end), and away episodes written in full-write mode into the reused, pre-filled away batch, equal the
    plain run into zero-initialised batches bit for bit; slot extents follow. The plain run repeated from the same
    state gives the same bits."""
    from maleague.components.replay_buffer import ReplayBuffer
    from maleague.envs.teams_env import VecEnvState
    stepper, macs, args, arm, _ = _stepper(device, cid)
    assert stepper.describe_rollout()[0] == arm
    info = dict(stepper.get_env_info(), n_agents=args.n_agents)
    scheme, groups, preprocess = scheme_for(info, torch)
    size, T1 = DSP.B + 5, DSP.EPISODE_LIMIT + 1
    ring = ReplayBuffer(scheme, groups, size, T1, preprocess=preprocess, device=device)
    for v in ring.data.transition_data.values():
        v.fill_(7)
    for it in range(2):  # slots 0..36, then 37..41 and 0..31 (wraps)
        runs = []
        for use_ring in (False, False, True):
            st = VecEnvState(stepper.spec, DSP.B, device)
            st.episode.fill_(it)
            stepper.envs = st
            stepper.t_env = DSP.T_ENV
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
        plain, again, ringed = runs
        for side in (0, 1):
            for k in plain[side]:
                assert torch.equal(plain[side][k], again[side][k]), (cid, it, side, k)
                assert torch.equal(plain[side][k], ringed[side][k]), (cid, it, side, k)
        hr = ringed[2]
        ring.insert_episode_batch(hr)
        slots = (torch.arange(DSP.B) + hr.slot0) % size
        want = (stepper.last_run["ep_len"] + 1).to(torch.int32)
        assert torch.equal(ring.slot_extent.cpu()[slots], want), (cid, it)
        assert torch.equal(stepper._away_extent.cpu(), want), (cid, it)


# ---- 4. small runs --------------------------------------------------------------------------------------------------

def test_single_env_stepper(device, distinct_oracle):
    """B = 1 through SelfPlayDistinctStepper: one live column in every agent tile of the one workgroup; two runs from
    the same state are bit-identical."""
    from maleague.envs.teams_env import VecEnvState
    from maleague.steppers import SelfPlayDistinctStepper
    stepper, macs, args, arm, _ = _stepper(device, "dxsp-n3-h64", B=1, cls=SelfPlayDistinctStepper)
    assert stepper.describe_rollout()[0] == arm
    hb, ab, env_info = stepper.run(test_mode=True)
    assert set(env_info) == {"battle_won", "draw"}
    helpers.check_sides(stepper, macs, args, (hb, ab), [env_info], episode=0, test_mode=True, eps=(0.0, 0.0),
                        dtype=F64)
    stepper.args.reuse_away_batch = False
    runs = []
    for _ in range(2):
        st = VecEnvState(stepper.spec, 1, device)
        st.episode.fill_(1)
        stepper.envs = st
        stepper.t_env = DSP.T_ENV
        hb, ab, _ = stepper.run(test_mode=False)
        runs.append(_snapshot(stepper, (hb, ab)))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


# ---- 5. cross-play --------------------------------------------------------------------------------------------------

CP_GRID, CP_SCALE, CP_SEED = 6, 0.3, 5  # tests/test_gpu_crossplay.py's: games are decided inside 30 steps


def _cp_args(plan, H, B):
    return qmix_args(batch_size_run=B, seed=CP_SEED, rnn_hidden_dim=H, obs_agent_id=False, mac="distinct",
                     env_args={"match_build_plan": plan, "grid_size": CP_GRID, "stochastic_spawns": True,
                               "episode_limit": DSP.EPISODE_LIMIT})


def _cp_stepper(device, args):
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import DistinctMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import SelfPlayDistinctParallelStepper
    stepper = SelfPlayDistinctParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(dict(info, n_agents=args.n_agents), torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    macs = [DistinctMAC(proto.scheme, groups, args) for _ in range(2)]
    for m in macs:
        m.cuda()
    stepper.initialize(scheme, groups, preprocess, *macs)
    stepper.args.reuse_away_batch = False
    return stepper, macs


@pytest.mark.parametrize("plan,H,two_rosters", DSP.CROSSPLAY_CASES,
                         ids=[f"{p}-h{h}" for p, h, _ in DSP.CROSSPLAY_CASES])
def test_crossplay_distinct_equals_per_pair_launches(device, plan, H, two_rosters):
    """A pool of 3 distinct policies (nh networks each), all 9 ordered pairs, E = 20 (one full and one partial
    workgroup per pair): ep_len, ret, ret_away, won and draw of mlg_crossplay_rollout_distinct bit-identical to nine
    test-mode mlg_rollout_selfplay_distinct launches; the summary rows are the documented fixed-order sums. On the 3v3
    plan the pairs alternate between two rosters of the spec table."""
    from maleague.envs.teams_env import VecEnvState
    from maleague.league.evaluation import DistinctCrossPlayEvaluator, PairTable, build_pairs
    from maleague.runs.sp_ma_experiment import agent_vector, load_agent_vector
    E, P, ep0 = DSP.CROSSPLAY_E, DSP.CROSSPLAY_POOL, DSP.CROSSPLAY_EPISODE0
    base = shape_plan(plan, self_play=True)
    stepper, macs = _cp_stepper(device, _cp_args(base, H, E))
    nh = macs[0].n_agents
    n_params = sum(p.numel() for p in macs[0].agents[0].parameters())
    rows = []
    for s in range(P):
        g = torch.Generator().manual_seed(41 + s)
        rows.append((torch.rand(nh * n_params, generator=g) * 2 - 1) * CP_SCALE)
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
    ev = DistinctCrossPlayEvaluator(_cp_args(base, H, E), device, episodes_per_launch=E)
    res = ev.evaluate(pool, table, E, episode0=ep0)
    got = {k: ev.last[k].cpu().numpy() for k in ref}
    for k in ("ep_len", "won", "draw"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    for k in ("ret", "ret_away"):
        np.testing.assert_array_equal(got[k].view(np.int32), ref[k], err_msg=k)
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
    np.testing.assert_array_equal(ev.last["summary"].cpu().numpy(), want)
    assert res.games.tolist() == [[float(E)] * P] * P
    assert torch.equal(res.wins + res.losses + res.draws, res.games)
    print(f"{plan} H={H}: episode lengths per pair {[(int(x.min()), int(x.max())) for x in got['ep_len']]}, "
          f"decided {int((~dr).sum())} of {n * E}")


# ---- 6. league ------------------------------------------------------------------------------------------------------

LG_B, LG_LIMIT = 32, 20


def _league_args(seed=1, **kw):
    from maleague.utils.config import build_config, to_args
    over = {"mac": "distinct", "obs_agent_id": False, "batch_size_run": LG_B, "batch_size": LG_B, "buffer_size": LG_B,
            "runner": "parallel", "buffer_cpu_only": False, "env_args.episode_limit": LG_LIMIT,
            "env_args.match_build_plan": "small", "t_max": 1000000, "test_interval": 100000000,
            "learner_log_interval": 0, "show_exp_parameters": False, "seed": seed,
            "league_checkpoint_min_steps": 2000000000, "league_checkpoint_max_steps": 4000000000}
    over.update(kw)
    return to_args(build_config("qmix", "ma", overrides=[f"{k}={v}" for k, v in over.items()]))


def _kill_slot(buffer, slot):
    """Only the no-op (action 0) is ever available to ``slot``, and taken, in every stored step of the buffer."""
    td = buffer.data.transition_data
    td["avail_actions"][:, :, slot] = 0
    td["avail_actions"][:, :, slot, 0] = 1
    td["actions"][:, :, slot] = 0
    td["actions_onehot"][:, :, slot] = 0
    td["actions_onehot"][:, :, slot, 0] = 1


def test_distinct_league_instance(device):
    """Player 1 of a two-player league with composed 3-unit teams (player 0 a fixed replica): after sync the away MAC
    holds the opponent's vector bit for bit and the pool rows are nh x n_params wide; play(2) books B games per
    iteration into the payoff and moves the home networks; with slot 1 dead in every stored step of the batches the
    learner sees, network 1 stays bit-unchanged through play while the others move; evaluate_pool(20) returns a 2 x 2
    table whose games sum to 80."""
    from maleague.custom_logging import MainLogger
    from maleague.controllers import DistinctMAC
    from maleague.league import DistinctLeagueInstance, DistributedLeague, PayoffEntry, league_instance_for
    from maleague.league.evaluation import DistinctCrossPlayEvaluator
    from maleague.league.teams import compose_league_teams
    from maleague.runs.sp_ma_experiment import agent_vector
    from maleague.steppers import SelfPlayDistinctParallelStepper
    torch.manual_seed(1)
    np.random.seed(1)
    teams = compose_league_teams(3, 2, "HEALER", "RANGED", seed=1)
    assert len({t.codes() for t in teams}) == 2
    lg = DistributedLeague(n_players=2, device=device, max_historical=2, player_id=1)
    inst = league_instance_for(_league_args(), MainLogger(log_interval=10 ** 12), lg, mode="rolebased",
                               role=["main", "main_exploiter"], seed=1, teams=teams)
    ex = inst.experiment
    assert type(inst) is DistinctLeagueInstance and type(ex.stepper) is SelfPlayDistinctParallelStepper
    assert isinstance(ex.home_mac, DistinctMAC) and isinstance(ex.away_mac, DistinctMAC)
    assert ex.stepper.describe_rollout()[0] == "dxsp-global/tpw1"
    nh = ex.home_mac.n_agents
    n_params = sum(p.numel() for p in ex.home_mac.agents[0].parameters())
    assert nh == 3 and agent_vector(ex.home_mac).numel() == nh * n_params
    opp = (agent_vector(ex.home_mac).clone() * 0.5).contiguous()
    lg.set_player_params(0, opp)
    assert inst.sync() == (0, False)
    assert tuple(lg.current.shape) == (2, nh * n_params) and lg.historical.shape[1] == nh * n_params
    assert torch.equal(agent_vector(ex.away_mac), opp) and torch.equal(lg.params_of(0), opp)
    assert torch.equal(lg.params_of(1), agent_vector(ex.home_mac))
    for i, a in enumerate(ex.away_mac.agents):  # network i of the away MAC is block i of the row
        got = torch.cat([p.detach().reshape(-1) for p in a.parameters()])
        assert torch.equal(got, opp[i * n_params:(i + 1) * n_params]), i
    assert ex.stepper.spec.role[nh:] == [u["role"].value["id"] for u in teams[0].units]
    home0 = agent_vector(ex.home_mac).clone()
    inst.play(2)
    lg.sync_payoff()
    torch.cuda.synchronize()
    pay = lg.payoff.tensor.cpu()
    assert float(pay[1, 0, PayoffEntry.GAMES]) == 2 * LG_B
    assert float(pay[1, 0, PayoffEntry.WIN:PayoffEntry.DRAW + 1].sum()) == 2 * LG_B
    assert ex.home_learner.train_calls == 2 and ex.home_mac.agents[0].trained_steps > 0
    assert len({a.trained_steps for a in ex.home_mac.agents}) == 1
    home1 = agent_vector(ex.home_mac).clone()
    for i in range(nh):
        assert not torch.equal(home1[i * n_params:(i + 1) * n_params], home0[i * n_params:(i + 1) * n_params]), i
    assert torch.equal(agent_vector(ex.away_mac), opp), "the frozen away MAC changed"
    # a slot dead in every stored step of the batches the learner samples: its network does not move
    dead = 1
    train_home = ex._train_home

    def killed(episode_num):
        _kill_slot(ex.home_buffer, dead)
        train_home(episode_num)
    ex._train_home = killed
    assert inst.sync() == (0, False)
    inst.play(2)
    torch.cuda.synchronize()
    ex._train_home = train_home
    home2 = agent_vector(ex.home_mac).clone()
    assert ex.home_learner.train_calls == 4
    for i in range(nh):
        same = torch.equal(home2[i * n_params:(i + 1) * n_params], home1[i * n_params:(i + 1) * n_params])
        assert same == (i == dead), (i, same)
    res = inst.evaluate_pool(20)
    assert type(inst._evaluator) is DistinctCrossPlayEvaluator
    assert tuple(res.games.shape) == (2, 2) and float(res.games.sum()) == 80.0
    assert torch.equal(res.wins + res.losses + res.draws, res.games)
    assert torch.isfinite(res.jpc_matrix).all() and (res.mean_ep_len >= 1).all() and (res.mean_ep_len <= LG_LIMIT).all()


def test_pretrain_vs_ai_hands_over_n_state_dicts(device):
    """One pre-training iteration against the mirrored scripted AI (mlg_rollout_distinct, the fused learner): the
    league experiment's home MAC then holds the pre-trained networks, all N of them."""
    from maleague.custom_logging import MainLogger
    from maleague.league import DistributedLeague, league_instance_for
    from maleague.runs.sp_ma_experiment import agent_vector
    torch.manual_seed(2)
    np.random.seed(2)
    lg = DistributedLeague(n_players=1, device=device, max_historical=1)
    inst = league_instance_for(_league_args(seed=2), MainLogger(log_interval=10 ** 12), lg, mode="matchmaking", seed=2)
    nh = inst.experiment.home_mac.n_agents
    home0 = agent_vector(inst.experiment.home_mac).clone()
    inst.pretrain_vs_ai(iterations=1)
    home1 = agent_vector(inst.experiment.home_mac)
    n_params = home0.numel() // nh
    for i in range(nh):
        assert not torch.equal(home1[i * n_params:(i + 1) * n_params], home0[i * n_params:(i + 1) * n_params]), i
    assert inst.sync() is not None and inst.opponent == 0
    assert torch.equal(agent_vector(inst.experiment.away_mac), lg.params_of(0))


def test_league_main_distinct_single_rank(tmp_path):
    """league/main.py --config=qmix mac=distinct obs_agent_id=False, one rank: pre-training against the scripted AI
    (mlg_rollout_distinct), two league iterations of two matches (mlg_rollout_selfplay_distinct), the final cross-play
    evaluation (mlg_crossplay_rollout_distinct); ends cleanly and prints the payoff."""
    iters, per_match = 2, 2
    cmd = [sys.executable, os.path.join(ROOT, "ma-league_amd", "maleague", "league", "main.py"), "--device=0",
           "--config=qmix", "--env-config=ma", "--league-config=matchmaking", "--experiment=matchmaking",
           "--league_size=1", "--team_size=3", f"--league-iterations={iters}", f"--match-iterations={per_match}",
           "--pretrain-iterations=1", "--runner=parallel", "--mac=distinct", "--obs_agent_id=False",
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
