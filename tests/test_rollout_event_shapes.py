"""The eventful rollout cases (tests/rollout_event_shapes.py) on the CPU: every case's arm through its family's
host-only describe query, the arms the table has to reach, the conditions that keep a case (near ties, early-ending
envs, ragged workgroups, wins) on the counts written beside it, those counts re-counted with the float64 oracle for the
cases of at most 5 units per side (scripts/rollout_event_counts.py counts all of them), the policy-heavy plan
spelling of helpers.shape_plan, and EnvInfos' termination order on unequal episode lengths."""
import functools

import numpy as np
import pytest

import rollout_event_shapes as ES
from helpers import shape_plan

LDS_LIMIT = 160 * 1024
ROLLOUT_ENV = ("MLG_ROLLOUT_KERNEL", "MLG_ROLLOUT_GENERIC", "MLG_ROLLOUT_GLOBAL_WEIGHTS")

# the arm names the eventful table has to reach, per entry point
REQUIRED_ARMS = {
    ("drqn", False): {"v7", "v7-static", "v2"} | {f"v1-{w}/tpw{k}" for w in ("lds", "global") for k in range(1, 5)},
    ("drqn", True): {"sp8", "sp7", "sp2"} | {f"v1-global/tpw{k}" for k in range(1, 5)},
    ("ff", False): {f"ff-lds/tpw{k}" for k in range(1, 5)} | {f"ff-global/tpw{k}" for k in range(2, 5)},
    ("ff", True): {f"ffsp-lds/tpw{k}" for k in range(1, 5)} | {f"ffsp-global/tpw{k}" for k in range(1, 5)},
    ("dx", False): {f"dx-global/tpw{k}" for k in range(1, 5)},
    ("dx", True): {f"dxsp-global/tpw{k}" for k in range(1, 5)},
}


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    for k in ROLLOUT_ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("cid", ES.IDS)
def test_case_arm(cid, monkeypatch):
    c = ES.case(cid)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    name, lds = ES.describe(c)
    assert name == c.arm
    assert 0 < lds <= LDS_LIMIT


def test_forced_global_cases_are_lds_by_default():
    import dqn_selfplay_shapes as FSP
    forced = [c for c in ES.CASES if c.env]
    assert sorted(c.arm for c in forced) == sorted(arm for _, arm in FSP.LDS_VS_GLOBAL)
    for c in forced:
        assert ES.describe(c)[0] == c.arm.replace("global", "lds")


def test_every_required_arm_has_an_eventful_case():
    for (family, sp), arms in REQUIRED_ARMS.items():
        have = {c.arm for c in ES.CASES if c.family == family and c.sp == sp}
        assert arms <= have, (family, sp, arms - have)
    policy = [c for c in ES.CASES if c.family == "policy" and not c.wins]
    assert sorted(c.arm.split("/")[1] for c in policy) == [f"tpw{k}" for k in range(1, 5)]
    assert {c.arm.split("/")[0] for c in policy} == {"policy-lds", "policy-global"}


def test_policy_wins_cases_per_family():
    """A policy-heavy case in mlg_rollout on a split-bf16 arm and on a v1 arm, in mlg_rollout_ff, mlg_rollout_distinct
    and mlg_rollout_policy; both orders of listing occur."""
    wins = [c for c in ES.CASES if c.wins]
    assert all(not c.sp for c in wins)
    arms = {(c.family, c.arm) for c in wins}
    assert any(f == "drqn" and a.startswith("v7") for f, a in arms)
    assert any(f == "drqn" and a.startswith("v1-") for f, a in arms)
    assert {"ff", "dx", "policy"} <= {f for f, _ in arms}
    assert {c.plan[-1] for c in wins} == {"p", "s"}


def test_policy_heavy_plan_spelling():
    from maleague.envs.teams_env import TeamsEnvSpec
    for name, first_scripted in (("7p2s", False), ("2s7p", True)):
        plan = shape_plan(name)
        spec = TeamsEnvSpec.from_env_args({"match_build_plan": plan, "grid_size": 8})
        assert (spec.n_agents, spec.U, spec.n_actions) == (7, 9, 14)
        assert list(spec.scripted) == [first_scripted, not first_scripted]
        team = list(spec.team)
        assert team == ([0] * 2 + [1] * 7 if first_scripted else [0] * 7 + [1] * 2)
    for bad in ("2p7s", "7s2p", "3p3s", "7p2p", "7p0s"):  # P > S > 0, one team of each kind
        with pytest.raises(AssertionError):
            shape_plan(bad)
    with pytest.raises(AssertionError):
        shape_plan("7p2s", self_play=True)


@pytest.mark.parametrize("cid", ES.IDS)
def test_table_counts_meet_the_conditions(cid):
    c = ES.case(cid)
    assert ES.conditions(c, dict(c.oracle, envs=2 * ES.B)) == []
    assert c.oracle["home_wins"] + c.oracle["away_wins"] + c.oracle["draws"] == 2 * ES.B
    assert 8 <= c.grid <= 12 and c.limit <= 60


def test_conditions_reject():
    c = ES.case("ev-sp8-3v3")
    ok = dict(c.oracle, envs=74)
    assert ES.conditions(c, dict(ok, near_ties=ok["greedy"] // 100)) == ["near ties above 0.5 %"]
    assert ES.conditions(c, dict(ok, early=7)) and ES.conditions(c, dict(ok, ragged=1))
    assert ES.conditions(c, dict(ok, home_wins=0)) == ["a side never wins"]
    w = ES.case("win-ff-7p2s")
    assert ES.conditions(w, dict(w.oracle, envs=74, home_wins=7))
    assert ES.conditions(w, dict(w.oracle, envs=74, home_wins=74)) == ["every env ends in a policy win"]


def test_events_counts():
    """early: strictly before the limit; ragged: a 16-env group whose lengths differ by at least 2."""
    L = np.full(37, 40)
    won = np.zeros((37, 2), np.int64)
    assert ES.events([L], [won], 40) == {"early": 0, "ragged": 0, "home_wins": 0, "away_wins": 0, "draws": 37}
    L[3], L[17], L[36] = 39, 38, 5  # a difference of 1 is not ragged; groups 1 and 2 are
    won[3, 0] = won[17, 1] = won[36, 1] = 1
    assert ES.events([L], [won], 40) == {"early": 3, "ragged": 2, "home_wins": 1, "away_wins": 2, "draws": 34}
    assert ES.events([L, L], [won, won], 40)["ragged"] == 4


@functools.lru_cache(maxsize=None)
def _counts(key):
    return ES.oracle_counts(next(c for c in ES.CASES if c._replace(id="", arm="", env=None, oracle=None) == key))


@pytest.mark.parametrize("cid", ES.CHEAP_IDS)
def test_oracle_counts_of_the_small_cases(cid):
    """The float64 oracle alone, rolled again: the counts are the table's (cases that differ in the arm only share
    one count)."""
    c = ES.case(cid)
    n = _counts(c._replace(id="", arm="", env=None, oracle=None))
    assert {k: n[k] for k in ES.ORACLE_KEYS} == c.oracle, ES.count_line(c, n)
    assert ES.conditions(c, n) == []


def test_env_infos_order_on_unequal_lengths():
    """EnvInfos (by episode length, then env index) against the order in which the restated reference stepper
    (oracle/stepper_ref.py) collects the infos of envs that end at different steps."""
    import stepper_ref
    from maleague.steppers.parallel_stepper import EnvInfos
    L = np.array([5, 2, 7, 2, 5, 1, 7, 3])
    B = len(L)
    won = np.array([[b % 2, (b // 2) % 2] for b in range(B)]) != 0
    draw = ~won.any(axis=1)

    class Fake:
        t = [0] * B

        def reset(self, i):
            self.t[i] = 0
            return np.zeros(1, np.float32), np.ones((1, 2), np.int32), np.zeros((1, 1), np.float32)

        def step(self, i, actions):
            self.t[i] += 1
            info = {"battle_won": [bool(won[i, 0]), bool(won[i, 1])], "draw": bool(draw[i]), "env": i}
            return ([0.0], self.t[i] == L[i], info, np.zeros(1, np.float32), np.ones((1, 2), np.int32),
                    np.zeros((1, 1), np.float32))

    out = stepper_ref.run(Fake(), lambda t, running, batch: np.zeros((len(running), 1), np.int64), B, int(L.max()) + 1,
                          1, 2, 1, 1)
    assert out["info_env"] == [5, 1, 3, 7, 0, 4, 2, 6]
    want = [{k: v for k, v in info.items() if k != "env"} for info in out["env_infos"]]
    infos = EnvInfos(won, draw, L)
    assert list(infos) == want and infos[1:3] == want[1:3]
    assert infos.won.tolist() == won[out["info_env"]].tolist()
