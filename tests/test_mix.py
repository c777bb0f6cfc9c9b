"""CPU: the opponent-mixture ABI (struct layouts, the describe table, every host refusal of mlg_rollout_selfplay_mix
before a launch), the group assignment, DistributedLeague.record_runs_mix on host tensors and LeagueInstance with
opponents_per_match on a fake experiment."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mix_shapes as MS
from helpers import drqn_dims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maleague.h")


# ---- ABI -------------------------------------------------------------------------------------------------
def _header_struct(name):
    """[(field, ctypes type)] of a typedef struct of maleague.h (int32_t and pointer fields)."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", src).group(1)
    out = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        m = re.match(r"(const\s+)?(\w+)\s+(.*)$", decl)
        ctype = m.group(2)
        for var in [v.strip() for v in m.group(3).split(",")]:
            if var.startswith("*"):
                out.append((var.lstrip("* "), ctypes.c_void_p))
            else:
                out.append((var, {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}[ctype]))
    return out


@pytest.mark.parametrize("name", ["MlgMixGroup", "MlgOpponentMix"])
def test_struct_layout_matches_header(name):
    from maleague import _native
    fields = getattr(_native, name)._fields_
    assert [(f, t) for f, t in fields] == _header_struct(name)


def test_header_declares_and_library_exports_the_mixture_entry_points():
    from maleague import _native
    lib = _native.load()
    src = open(HEADER).read()
    for sym in ("mlg_rollout_selfplay_mix", "mlg_rollout_selfplay_mix_describe", "mlg_league_record_runs_mix"):
        assert re.search(r"\b" + sym + r"\s*\(", src) and hasattr(lib, sym) and sym in _native.SIGNATURES
    assert ctypes.sizeof(_native.MlgMixGroup) == 8
    assert len(_native.SIGNATURES["mlg_rollout_selfplay_mix"][1]) == 12
    assert len(_native.SIGNATURES["mlg_league_record_runs_mix"][1]) == 9


# ---- describe --------------------------------------------------------------------------------------------
def _spec(plan):
    from maleague.envs.teams_env import TeamsEnvSpec
    return TeamsEnvSpec.from_env_args(MS.env_args(plan))


@pytest.mark.parametrize("cid,plan,H,force,arm", MS.DESCRIBE_CASES)
def test_describe_table(monkeypatch, cid, plan, H, force, arm):
    """sp8-mix exactly where mlg_rollout_selfplay launches sp8; everything else, a forced generic kernel included,
    is v1-mix."""
    from maleague import _native
    monkeypatch.delenv("MLG_ROLLOUT_KERNEL", raising=False)
    monkeypatch.delenv("MLG_ROLLOUT_GENERIC", raising=False)
    if force:
        monkeypatch.setenv("MLG_ROLLOUT_KERNEL", force)
    spec = _spec(plan)
    dims = drqn_dims(spec, H, self_play=True)
    name, lds = _native.rollout_selfplay_mix_describe(spec.to_c(), dims)
    plain, plain_lds = _native.rollout_describe(spec.to_c(), dims, True)
    assert MS.arm_of(name) == arm, (cid, name)
    assert (arm == "sp8-mix") == (plain == "sp8")
    if arm == "sp8-mix":
        assert lds == plain_lds
    else:
        assert name.startswith("v1-mix/tpw") and 0 < lds <= 160 * 1024


@pytest.mark.parametrize("var,val", [("MLG_ROLLOUT_GENERIC", "1"), ("MLG_ROLLOUT_KERNEL", "sp7"),
                                     ("MLG_ROLLOUT_KERNEL", "sp2")])
def test_describe_other_forced_arms_get_v1_mix(monkeypatch, var, val):
    from maleague import _native
    monkeypatch.delenv("MLG_ROLLOUT_KERNEL", raising=False)
    monkeypatch.delenv("MLG_ROLLOUT_GENERIC", raising=False)
    monkeypatch.setenv(var, val)
    spec = _spec("small")
    assert MS.arm_of(_native.rollout_selfplay_mix_describe(spec.to_c(), drqn_dims(spec, 64, self_play=True))[0]) == \
        "v1-mix"


# ---- refusals: nothing is read or launched (every device pointer is garbage) -----------------------------
GARBAGE = 0x7000  # 16-byte aligned, never dereferenced by a refused call


class _Call:
    """A valid argument set of mlg_rollout_selfplay_mix over garbage device pointers; a test breaks one thing."""

    def __init__(self, plan="small", H=64, B=37, n_pool=3, n_specs=2):
        from maleague import _native
        self.n = _native
        spec = _spec(plan)
        self.spec0 = spec.to_c()
        self.dims = drqn_dims(spec, H, self_play=True)
        self.st = _native.MlgEnvState(GARBAGE, GARBAGE, GARBAGE, GARBAGE, GARBAGE, B)
        T1 = spec.episode_limit + 1
        mk = lambda: _native.MlgBatch(*([GARBAGE] * 8), B, T1, 0, 0, 0, None, None)  # noqa: E731
        self.home, self.away = mk(), mk()
        self.info = _native.MlgRunInfo(GARBAGE, GARBAGE, GARBAGE, GARBAGE, None, GARBAGE)
        G = (B + 15) // 16
        self.groups = (_native.MlgMixGroup * G)(*[_native.MlgMixGroup(g % n_pool, g % n_specs) for g in range(G)])
        self.specs = (_native.MlgEnvSpec * n_specs)(*[spec.to_c() for _ in range(n_specs)])
        self.mix = _native.MlgOpponentMix(GARBAGE, n_pool, G, GARBAGE, ctypes.addressof(self.groups), GARBAGE,
                                          ctypes.addressof(self.specs), n_specs)
        self.home_packed = GARBAGE

    def refused(self, mix=True):
        n = self.n
        lib = n.load()
        rc = lib.mlg_rollout_selfplay_mix(n.byref(self.spec0), n.byref(self.st), n.byref(self.dims), self.home_packed,
                                          n.byref(self.mix) if mix else None, n.byref(self.home), n.byref(self.away),
                                          n.byref(self.info), 0.5, 0.3, 0, None)
        assert rc != 0, "the call was not refused"
        return lib.mlg_last_error().decode()


def test_refuses_null_pointers():
    assert "null pointer" in _Call().refused(mix=False)
    c = _Call()
    c.home_packed = None
    assert "null pointer" in c.refused()
    for field in ("packed_pool", "groups", "host_groups", "specs", "host_specs"):
        c = _Call()
        setattr(c.mix, field, None)
        assert "null pool / groups / specs" in c.refused(), field
    c = _Call()
    c.info.won = None
    assert "run info" in c.refused()


def test_refuses_wrong_group_count():
    c = _Call()
    c.mix.n_groups = 2
    assert "n_groups=2" in c.refused() and "= 3 groups" in c.refused()


def test_refuses_indices_out_of_range():
    for away, spec, word in ((3, 0, "away=3"), (-1, 0, "away=-1"), (0, 2, "spec=2"), (0, -1, "spec=-1")):
        c = _Call()
        c.groups[1].away, c.groups[1].spec = away, spec
        msg = c.refused()
        assert "groups[1]" in msg and word in msg, msg


@pytest.mark.parametrize("field,value", [("U", 8), ("n_agents", 4), ("grid", 9), ("episode_limit", 41),
                                         ("stochastic", 0), ("policy_team", 1), ("seed", 12)])
def test_refuses_specs_that_disagree(field, value):
    """Each spec stays valid in itself, so that the shape rule is what refuses it (n_actions is 5 + U in a valid spec
    and cannot disagree on its own)."""
    c = _Call()
    s = c.specs[1]
    setattr(s, field, value)
    if field == "U":
        s.n_actions = 5 + value
        for u in (6, 7):
            s.team[u] = u % 2
    if field == "policy_team":  # the other team first: home agents are then team 1's units
        for u in range(s.U):
            s.team[u] = 1 - s.team[u]
    msg = c.refused()
    assert "specs[1]" in msg, msg
    if field != "n_agents":  # four agents: units 2 and 3 are then away agents of the home team
        assert f"specs[1].{field}" in msg, msg


def test_refuses_home_agents_not_the_home_team():
    c = _Call()
    s = c.specs[0]
    nh = s.n_agents // 2
    units = [s.agent_unit[a] for a in range(s.n_agents)]
    for a in range(s.n_agents):
        s.agent_unit[a] = units[(a + nh) % s.n_agents]
    assert "must be the home team" in c.refused()
    c = _Call()
    c.spec0.n_policy_teams = 1
    assert "two-team" in c.refused()


def test_refuses_unaligned_pool():
    c = _Call()
    c.mix.packed_pool = GARBAGE + 4
    assert "16-byte aligned" in c.refused()


def test_refuses_bad_batches_and_dims():
    c = _Call()
    c.away.T1 += 1
    assert "(away)" in c.refused()
    c = _Call()
    c.dims.n_agents += 1
    c.dims.d_in += 1  # a valid agent of four per side, over an env of three per side
    assert "agent dims" in c.refused()


def test_record_runs_mix_refusals():
    from maleague import _native
    lib = _native.load()
    assert lib.mlg_league_record_runs_mix(None, GARBAGE, 37, GARBAGE, 3, GARBAGE, 5, 1, None) != 0
    assert lib.mlg_league_record_runs_mix(GARBAGE, GARBAGE, 37, GARBAGE, 0, GARBAGE, 5, 1, None) != 0
    assert lib.mlg_league_record_runs_mix(GARBAGE, GARBAGE, 37, GARBAGE, 3, GARBAGE, 3, 1, None) != 0
    assert b"entry_stride" in lib.mlg_last_error()


# ---- group assignment / host reduction -------------------------------------------------------------------
@pytest.mark.parametrize("K,G,blocks", [(1, 3, [3]), (3, 3, [1, 1, 1]), (3, 5, [1, 2, 2]), (4, 256, [64] * 4),
                                        (5, 3, [1, 1, 1])])
def test_group_assignment(K, G, blocks):
    """Draw j gets the contiguous groups [floor(j G / K), floor((j + 1) G / K)); K is clipped to G."""
    from maleague.league.instance import group_assignment, group_count
    table = group_assignment(K, G)
    assert len(table) == G and table == sorted(table)
    assert [table.count(j) for j in range(min(K, G))] == blocks
    for j in range(min(K, G)):
        k = min(K, G)
        assert [g for g, d in enumerate(table) if d == j] == list(range(j * G // k, (j + 1) * G // k))
    assert group_count(37) == 3 and group_count(48) == 3 and group_count(4096) == 256 and group_count(1) == 1


@pytest.mark.parametrize("compat", [False, True])
def test_record_runs_mix_host_equals_per_opponent_record_runs(compat):
    """Host tensors: the mixture booking equals record_runs of every opponent's envs; a repeated draw shares its
    column."""
    from maleague.league import DistributedLeague
    rng = np.random.RandomState(7)
    B = 70  # 5 groups, the last one partly filled
    won = torch.from_numpy(rng.randint(0, 2, size=(B, 2)).astype(np.int32))
    draw = torch.from_numpy((rng.rand(B) < 0.3).astype(np.int32))
    cols, table = [3, 0, 3], [0, 1, 1, 2, 2]  # draws 0 and 2 are the same opponent
    a = DistributedLeague(n_players=2, device="cpu", max_historical=2, reference_compat=compat)
    b = DistributedLeague(n_players=2, device="cpu", max_historical=2, reference_compat=compat)
    a.record_runs_mix(1, cols, table, won, draw)
    env_col = np.repeat([cols[k] for k in table], 16)[:B]
    for c in (0, 3):
        sel = torch.from_numpy(env_col == c)
        b.record_runs(1, c, won[sel], draw[sel])
    assert torch.equal(a._delta, b._delta)
    assert a._delta[1, :, 1:4].sum() == B
    if not compat:
        assert a._delta[1, 3, 0] == 16 + (B - 48) and a._delta[1, 0, 0] == 32
    with pytest.raises(ValueError):
        a.record_runs_mix(1, cols, [0, 1, 2], won, draw)
    with pytest.raises(ValueError):
        a.record_runs_mix(1, [9], [0] * 5, won, draw)


# ---- LeagueInstance on a fake experiment -----------------------------------------------------------------
class _FakeAgent(torch.nn.Module):
    def __init__(self, value):
        super().__init__()
        self.w = torch.nn.Parameter(torch.full((6,), float(value)))
        self.trained_steps = 0


class _FakeExperiment:
    """Stands in for LeagueExperiment on CPU (the style of tests/test_league.py): random battle outcomes."""

    def __init__(self, B):
        self.home_mac = SimpleNamespace(agent=_FakeAgent(0))
        self.away_mac = SimpleNamespace(agent=_FakeAgent(-1))
        self.stepper = SimpleNamespace(batch_size=B, _info=torch.zeros(6 * B, dtype=torch.int32))
        self.rng = np.random.RandomState(0)
        self.adversaries, self.mixes, self.matches = [], [], []

    def load_adversary_vector(self, vec):
        self.adversaries.append(vec.clone())

    def load_adversary_mix(self, rows, group_opponent, teams=None, home=None):
        self.mixes.append((rows.clone(), list(group_opponent), teams, home))

    def configure_match(self, home, away=None):
        self.matches.append((home, away))

    def _train_episode(self, episode):
        B = self.stepper.batch_size
        self.stepper._info[B:3 * B] = torch.from_numpy(self.rng.randint(0, 2, 2 * B).astype(np.int32))
        self.stepper._info[3 * B:4 * B] = torch.from_numpy(self.rng.randint(0, 2, B).astype(np.int32))
        self.home_mac.agent.trained_steps += B * 10
        with torch.no_grad():
            self.home_mac.agent.w.add_(1.0)


def _fake_instance(B=80, n=3, teams=None, matchmaking="pfsp", **kw):
    from maleague.league import DistributedLeague, LeagueInstance
    args = SimpleNamespace(matchmaking=matchmaking, env_args={})
    lg = DistributedLeague(n_players=n, device="cpu", seed=0, max_historical=2, player_id=0)
    for p in range(1, n):
        lg.set_player_params(p, torch.full((6,), 10.0 * p))
    exp = _FakeExperiment(B)
    return lg, exp, LeagueInstance(args, None, lg, mode="matchmaking", seed=0, experiment=exp, teams=teams, **kw)


def test_one_opponent_per_match_is_todays_path():
    """opponents_per_match = 1: the history, payoff and matchmaker RNG state of an instance built without the argument,
    through load_adversary_vector / record_runs only."""
    outs = []
    for kw in ({}, {"opponents_per_match": 1}):
        lg, exp, inst = _fake_instance(**kw)
        hist = inst.run(league_iterations=4, iterations_per_match=2)
        assert exp.mixes == [] and len(exp.adversaries) == 4 and inst.group_draw is None
        assert inst.opponents == [inst.opponent]
        outs.append((list(hist), lg.payoff.tensor.clone(), inst.matchmaker.rng.get_state()))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1])
    for x, y in zip(outs[0][2], outs[1][2]):
        assert np.array_equal(x, y)


def test_three_opponents_per_match_bookkeeping():
    """K = 3 over G = 5 groups: MATCHES += 3 per sync, every column's games = 16 x its groups, the mixture rows are the
    pool rows of the draws."""
    from maleague.league import PayoffEntry
    lg, exp, inst = _fake_instance(B=80, opponents_per_match=3)
    games = np.zeros(lg.capacity)
    for it in range(3):
        assert inst.sync() is not None
        assert len(inst.opponents) == 3 and inst.opponent == inst.opponents[0]
        assert inst.group_draw == [0, 1, 1, 2, 2]
        rows, table, teams, home = exp.mixes[-1]
        assert table == inst.group_draw and teams is None
        for j, opp in enumerate(inst.opponents):
            assert torch.equal(rows[j], lg.params_of(opp))
            games[opp] += 2 * 16 * inst.group_draw.count(j)
        inst.play(2)
    pay = lg.sync_payoff()
    assert pay[0, :, PayoffEntry.MATCHES].sum() == 9
    np.testing.assert_array_equal(pay[0, :, PayoffEntry.GAMES].numpy(), games)
    np.testing.assert_array_equal(pay[0, :, PayoffEntry.WIN:PayoffEntry.DRAW + 1].sum(-1).numpy(), games)
    assert len(inst.history) == 9 and [h[0] for h in inst.history] == list(range(9))
    # K clipped to the launch's groups
    _, exp2, inst2 = _fake_instance(B=20, opponents_per_match=5)
    assert inst2.sync() is not None and len(inst2.opponents) == 2 and inst2.group_draw == [0, 1]
    with pytest.raises(ValueError):
        _fake_instance(opponents_per_match=0)


def test_three_opponents_with_teams_list_each_roster():
    from maleague.league.teams import compose_league_teams
    teams = compose_league_teams(5, 3, "HEALER", "RANGED", seed=4)
    lg, exp, inst = _fake_instance(B=48, teams=teams, matchmaking="random", opponents_per_match=3)
    for it in range(2):
        assert inst.sync() is not None
        rows, table, aways, home = exp.mixes[-1]
        assert home == teams[0] and aways == [teams[o] for o in inst.opponents]
        assert inst.away_team == teams[inst.opponents[0]] and exp.matches[-1] == (teams[0], inst.away_team)
        assert inst.away_teams[-3:] == [teams[o].codes() for o in inst.opponents]
    assert len(inst.away_teams) == 6


def test_league_ends_when_a_draw_is_none():
    """The league ends for everybody if any of the K draws is None: the non-recurring matchmaker reads the synced
    MATCHES, so its three draws of a sync agree; after both other players were played every draw is None."""
    lg, exp, inst = _fake_instance(B=48, n=3, matchmaking="adversaries", opponents_per_match=3)
    assert inst.sync() == (1, False) and inst.opponents == [1, 1, 1]
    assert inst.sync() == (2, False) and inst.opponents == [2, 2, 2]
    assert inst.sync() is None and len(exp.mixes) == 2 and len(inst.history) == 6
