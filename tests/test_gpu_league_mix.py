"""GPU: the league side of opponent mixtures -- mlg_league_record_runs_mix against a numpy count, and LeagueInstance
with opponents_per_match = 3 on one rank (matchmaking and role based), K = 1 being today's code path bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _numpy_counts(won, draw, group_col, n_cols):
    """[n_cols, 4] GAMES, WIN, LOSS, DRAW by mlg_league_record_runs's rule, per column."""
    out = np.zeros((n_cols, 4), dtype=np.int64)
    for b in range(len(draw)):
        w0, w1 = bool(won[b, 0]), bool(won[b, 1])
        dr = bool(draw[b]) or w0 == w1
        c = group_col[b // 16]
        out[c, 0] += 1
        out[c, 1 + (2 if dr else (0 if w0 else 1))] += 1
    return out


@pytest.mark.parametrize("count_games", [0, 1])
def test_record_runs_mix_kernel_exact(device, count_games):
    """B = 37 with columns [2, 0, 2] (a repeated column, a partly filled last group), results read from a pinned summary
    slot as LeagueInstance.play passes them; and a device-memory table with more columns than waves."""
    from maleague import _native
    from maleague.league import DistributedLeague
    rng = np.random.RandomState(5)
    for B, n_cols, cols, pinned in ((37, 3, [2, 0, 2], True), (4096, 40, list(rng.randint(0, 40, size=256)), False)):
        won = rng.randint(0, 2, size=(B, 2)).astype(np.int32)
        draw = (rng.rand(B) < 0.25).astype(np.int32)
        info = torch.zeros(6 * B, dtype=torch.int32, pin_memory=True) if pinned else \
            torch.zeros(6 * B, dtype=torch.int32, device=device)
        info[B:3 * B] = torch.from_numpy(won.reshape(-1)).to(info.device)
        info[3 * B:4 * B] = torch.from_numpy(draw).to(info.device)
        row = torch.zeros(n_cols, 5, device=device)
        row[:, 4] = 9.0  # MATCHES: not the kernel's to touch
        gcol = torch.tensor(cols, dtype=torch.int32, device=device)
        for _ in range(2):  # accumulates
            _native.call("mlg_league_record_runs_mix", info[B:3 * B].data_ptr(), info[3 * B:4 * B].data_ptr(), B,
                         gcol.data_ptr(), n_cols, row.data_ptr(), 5, count_games, _native.stream_ptr(device))
        torch.cuda.synchronize()
        exp = 2 * _numpy_counts(won, draw, cols, n_cols)
        if not count_games:
            exp[:, 0] = 0
        np.testing.assert_array_equal(row[:, :4].cpu().numpy().astype(np.int64), exp)
        assert (row[:, 4] == 9.0).all()
        # DistributedLeague.record_runs_mix: the device launch equals the host reduction
        lg_d = DistributedLeague(n_players=n_cols, device=device, reference_compat=not count_games)
        lg_h = DistributedLeague(n_players=n_cols, device="cpu", reference_compat=not count_games)
        pids = sorted(set(cols))
        table = [pids.index(c) for c in cols]
        lg_d.record_runs_mix(1, pids, table, info[B:3 * B].view(B, 2), info[3 * B:4 * B])
        lg_h.record_runs_mix(1, pids, table, torch.from_numpy(won), torch.from_numpy(draw))
        np.testing.assert_array_equal(lg_d._delta.cpu().numpy(), lg_h._delta.numpy())


def _args(B, seed=0):
    from maleague.utils.config import build_config, to_args
    cfg = build_config("qmix", "ma", overrides=[f"batch_size_run={B}", "runner=parallel", "buffer_cpu_only=False",
                                                "buffer_size=256", "batch_size=32", "env_args.episode_limit=30",
                                                "t_max=1000000", "test_interval=100000000", f"seed={seed}",
                                                "league_checkpoint_min_steps=1", "league_checkpoint_max_steps=1"])
    return to_args(cfg)


def _instance(device, mode, seed, **kw):
    from maleague.custom_logging import MainLogger
    from maleague.league import DistributedLeague, LeagueInstance
    torch.manual_seed(seed)
    np.random.seed(seed)
    lg = DistributedLeague(n_players=1, device=device, max_historical=3, seed=seed)
    inst = LeagueInstance(_args(48, seed), MainLogger(), lg, mode=mode, role=["main"] if mode == "rolebased" else None,
                          seed=seed, **kw)
    return lg, inst


@pytest.mark.parametrize("mode", ["matchmaking", "rolebased"])
def test_league_instance_three_opponents_per_match(device, mode):
    """K = 3 at B = 48 (one group per draw): two syncs with one training iteration each. Every game lands in the column
    of its group's opponent, MATCHES counts the draws, the home learner trained; role based, the second sync draws the
    snapshot taken at its start (seed 3: the main player's fourth coin is 0.33 < 0.5, the PFSP-over-historical
    branch)."""
    from maleague.league import PayoffEntry
    from maleague.runs.sp_ma_experiment import agent_vector
    lg, inst = _instance(device, mode, 3, opponents_per_match=3)
    st = inst.experiment.stepper
    home0 = agent_vector(inst.experiment.home_mac).clone()
    games = np.zeros(lg.capacity)
    for it in range(2):
        assert inst.sync() is not None
        assert len(inst.opponents) == 3 and inst.opponent == inst.opponents[0]
        assert inst.group_draw == [0, 1, 2]
        assert st.describe_rollout()[0] == "sp8-mix"
        inst.play(1)
        for opp in inst.opponents:
            games[opp] += 16
    lg.sync_payoff()
    torch.cuda.synchronize()
    pay = lg.payoff.tensor.cpu()
    np.testing.assert_array_equal(pay[0, :, PayoffEntry.GAMES].numpy(), games)
    np.testing.assert_array_equal(pay[0, :, PayoffEntry.WIN:PayoffEntry.DRAW + 1].sum(-1).numpy(), games)
    assert pay[0, :, PayoffEntry.MATCHES].sum() == 6
    assert len(inst.history) == 6
    assert not torch.equal(agent_vector(inst.experiment.home_mac), home0), "the home learner did not train"
    if mode == "rolebased":
        assert len(lg.historical_meta) >= 1
        assert any(h for _, _, h in inst.history[3:]), inst.history
        assert any(o >= lg.n for o in inst.opponents)


@pytest.mark.parametrize("mode", ["matchmaking", "rolebased"])
def test_one_opponent_per_match_is_the_plain_path(device, mode):
    """opponents_per_match = 1 on the same seed: the history, the payoff and the home agent's parameters after two
    iterations equal those of an instance built without the argument, bit for bit, on the plain entry point."""
    from maleague.runs.sp_ma_experiment import agent_vector
    outs = []
    for kw in ({}, {"opponents_per_match": 1}):
        lg, inst = _instance(device, mode, 3, **kw)
        for _ in range(2):
            assert inst.sync() is not None
            assert inst.experiment.stepper.describe_rollout()[0] == "sp8" and inst.group_draw is None
            inst.play(1)
        lg.sync_payoff()
        torch.cuda.synchronize()
        outs.append((list(inst.history), lg.payoff.tensor.cpu().clone(), agent_vector(inst.experiment.home_mac).clone()))
    assert outs[0][0] == outs[1][0]
    assert torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][2], outs[1][2])


def test_league_main_opponents_per_match_flag(tmp_path, capsys):
    """league/main.py --league_opponents_per_match=3 (in process, one main player with a composed team and its
    snapshots, B = 64: four groups): every match lists three draws, every training game is booked once, and the
    default (no key) lists one draw per match."""
    from maleague.league.main import main
    argv = ["--device=0", "--config=qmix", "--env-config=ma", "--league-config=matchmaking", "--experiment=alphastar",
            "--league_size=1", "--main_exploiters_n=0", "--team_size=5", "--league-iterations=2", "--match-iterations=1",
            "--pretrain-iterations=0", "--runner=parallel", "--batch_size_run=64", "--env_args.episode_limit=20",
            "--buffer_size=128", "--league_checkpoint_min_steps=1", "--league_checkpoint_max_steps=1",
            f"--local_results_path={tmp_path}", "--show_exp_parameters=False"]
    tail = ["force-unit", "--role=HEALER", "--attack=RANGED"]
    s = main(argv + ["--league_opponents_per_match=3"] + tail)
    capsys.readouterr()
    n = 1 + s["historical_snapshots"]
    (matches,) = s["matches"]
    assert len(matches) == 2 and all(len(m["opponents"]) == 3 and m["opponent"] == m["opponents"][0] for m in matches)
    pay = np.array(s["payoff"])
    assert pay[0, :n, 0].sum() == 2 * 64 and pay[0, :n, 1:4].sum() == 2 * 64 and pay[0, :n, 4].sum() == 6
    exp = np.zeros(pay.shape[1])
    for m in matches:  # draw j of three on the groups [floor(4 j / 3), floor(4 (j + 1) / 3)): 1, 1 and 2 groups
        for opp, groups in zip(m["opponents"], (1, 1, 2)):
            exp[opp] += 16 * groups
    np.testing.assert_array_equal(pay[0, :, 0], exp)
    s1 = main(argv + tail)
    capsys.readouterr()
    assert all(m["opponents"] == [m["opponent"]] for m in s1["matches"][0])
