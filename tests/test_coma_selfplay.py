"""COMA in self-play and the league on the CPU (no GPU call): the dispatch of mlg_rollout_selfplay_policy pinned through
its host-only query, the rejections by message, the ABI of the new entry points, which stepper registry and which
evaluator agent_output_type selects, the refusals the old classes keep, the mixture refused by name, and the near-tie
conditions of the case table (tests/coma_selfplay_shapes.py) recomputed for the two smallest cases."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

import coma_selfplay_shapes as SP
from helpers import coma_args, drqn_dims, qmix_args, scheme_for

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maleague.h")
LDS_LIMIT = 160 * 1024


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from maleague import _native
    lib = _native.load()
    src = open(HEADER).read()
    for sym in ("mlg_rollout_selfplay_policy", "mlg_rollout_selfplay_policy_describe", "mlg_crossplay_rollout_policy"):
        assert re.search(r"\b" + sym + r"\s*\(", src) and hasattr(lib, sym) and sym in _native.SIGNATURES
    # mlg_rollout_selfplay's arguments plus mask_before_softmax and test_greedy
    sp, pol = _native.SIGNATURES["mlg_rollout_selfplay"][1], _native.SIGNATURES["mlg_rollout_selfplay_policy"][1]
    assert list(pol) == list(sp[:-1]) + [ctypes.c_int32, ctypes.c_int32] + [sp[-1]]
    cp, cpp = _native.SIGNATURES["mlg_crossplay_rollout"][1], _native.SIGNATURES["mlg_crossplay_rollout_policy"][1]
    assert len(cpp) == len(cp) + 2


# ---- mlg_rollout_selfplay_policy_describe -----------------------------------------------------------------------------
@pytest.mark.parametrize("c", SP.CASES, ids=SP.IDS)
def test_case_arm(c, monkeypatch):
    monkeypatch.delenv("MLG_ROLLOUT_GLOBAL_WEIGHTS", raising=False)
    name, lds = SP.describe(c.plan, c.H)
    assert name == c.arm and 0 < lds <= LDS_LIMIT
    assert (lds > 32 * 1024) == name.startswith("sp-policy-lds")  # the two weight images are what fills LDS
    monkeypatch.setenv("MLG_ROLLOUT_GLOBAL_WEIGHTS", "1")  # forces the global arm, as it does for v1
    forced, lds_g = SP.describe(c.plan, c.H)
    assert forced == c.arm.replace("-lds", "-global") and lds_g <= 32 * 1024


def test_cases_cover_the_arms(monkeypatch):
    """6 / 10 / 18 / 32 tiles (K = 1..4) on the global arm, K = 1..4 on the LDS arm, one to three action tiles, all three
    widths; the LDS arm at H = 32 only (never at H = 64: one 3v3 image is ~117 KB), and where two images fit."""
    monkeypatch.delenv("MLG_ROLLOUT_GLOBAL_WEIGHTS", raising=False)
    arms = {c.arm for c in SP.CASES}
    assert arms == {f"sp-policy-{w}/tpw{k}" for w in ("lds", "global") for k in (1, 2, 3, 4)}
    assert {c.H for c in SP.CASES} == {32, 64, 128}
    assert {(SP.spec_of(c.plan).n_actions + 15) // 16 for c in SP.CASES} == {1, 2, 3}
    assert {SP.spec_of(c.plan).n_actions for c in SP.CASES} >= {11, 15, 23, 37}
    assert all(True in c.greedy for c in SP.CASES)
    assert [c.id for c in SP.CASES if False in c.greedy][:2] == ["3v3-h32", "5v5-h64"]
    for k in range(1, 17):
        for H in (64, 128):
            assert SP.describe(f"{k}v{k}", H)[0].startswith("sp-policy-global")
        assert SP.describe(f"{k}v{k}", 32)[0].startswith("sp-policy-lds" if k <= 14 else "sp-policy-global"), k
    assert set(SP.RING_CASES) <= set(SP.IDS) and SP.EPS[0] != SP.EPS[1]


def test_rejections_by_message():
    from maleague import _native
    from maleague.envs.teams_env import TeamsEnvSpec
    with pytest.raises(_native.NativeError, match="agent tiles per wave"):  # 17v17: no launch, no pointer read
        SP.describe(SP.REJECTED_PLAN, 32)
    spec = SP.spec_of("3v3")
    for hidden in (16, 48, 256):
        with pytest.raises(_native.NativeError, match="rnn_hidden_dim"):
            _native.rollout_selfplay_policy_describe(spec.to_c(), drqn_dims(spec, hidden, self_play=True))
    with pytest.raises(_native.NativeError, match="agent dims do not match one side"):
        _native.rollout_selfplay_policy_describe(spec.to_c(), drqn_dims(spec, 32))  # both sides' agents as one MAC
    ai = TeamsEnvSpec.from_env_args({"match_build_plan": "small", "grid_size": 8, "episode_limit": 40})
    with pytest.raises(_native.NativeError, match="two-team scenario"):
        _native.rollout_selfplay_policy_describe(ai.to_c(), drqn_dims(ai, 32))
    lib = _native.load()
    name, lds = ctypes.create_string_buffer(4), ctypes.c_int64(0)
    assert lib.mlg_rollout_selfplay_policy_describe(ctypes.byref(spec.to_c()), ctypes.byref(drqn_dims(spec, 32, True)),
                                                    name, len(name), ctypes.byref(lds)) != 0
    assert b"too small" in lib.mlg_last_error()
    # the entry points themselves refuse null arguments through mlg_last_error, before anything is launched
    big = SP.spec_of(SP.REJECTED_PLAN)
    assert lib.mlg_rollout_selfplay_policy(ctypes.byref(big.to_c()), None, None, None, None, None, None, None, 0.0, 0.0,
                                           0, 1, 1, None) != 0
    assert b"null" in lib.mlg_last_error()
    assert lib.mlg_crossplay_rollout_policy(ctypes.byref(drqn_dims(spec, 32, True)), None, 1, 1, None) != 0
    assert b"crossplay: null argument block" in lib.mlg_last_error()


# ---- Python: registries, refusals -----------------------------------------------------------------------------------
def _macs(args, info):
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    scheme, groups, preprocess = scheme_for(dict(info, n_agents=args.n_agents), torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device="cpu")
    return (scheme, groups, preprocess), BasicMAC(proto.scheme, groups, args), BasicMAC(proto.scheme, groups, args)


def _stepper(cls, args):
    from maleague.custom_logging import MainLogger
    stepper = cls(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    return stepper, info


def test_registries_and_stepper_refusals():
    from maleague import steppers
    from maleague.steppers import (SELF_POLICY_REGISTRY, SELF_REGISTRY, OpponentMix, SelfPlayParallelStepper,
                                   SelfPlayPolicyParallelStepper, SelfPlayPolicyStepper, SelfPlayStepper)
    assert SELF_POLICY_REGISTRY == {"parallel": SelfPlayPolicyParallelStepper, "episode": SelfPlayPolicyStepper}
    assert SELF_REGISTRY == {"parallel": SelfPlayParallelStepper, "episode": SelfPlayStepper}
    assert "SELF_POLICY_REGISTRY" in steppers.__all__
    assert issubclass(SelfPlayPolicyStepper, SelfPlayPolicyParallelStepper)
    pi = SP.coma_sp_args("3v3", 32, True, device="cpu")
    q = qmix_args(batch_size_run=SP.B, seed=SP.SEED, rnn_hidden_dim=32, env_args=SP.env_args("3v3"), device="cpu")
    # the policy stepper takes two pi_logits MACs and reports the arm
    st, info = _stepper(SelfPlayPolicyParallelStepper, pi)
    sch, home, away = _macs(pi, info)
    st.initialize(*sch, home, away)
    assert st.describe_rollout()[0] == "sp-policy-lds/tpw1"
    with pytest.raises(NotImplementedError, match="pi_logits"):
        st.set_opponent_mix(OpponentMix(torch.zeros(1, 4), [0, 0]))
    st.set_opponent_mix(None)
    # ... and refuses a Q side, naming what it wants
    stq, infoq = _stepper(SelfPlayPolicyParallelStepper, q)
    _, hq, aq = _macs(q, infoq)
    for pair in ((hq, aq), (home, aq), (hq, away)):
        with pytest.raises(NotImplementedError, match="pi_logits"):
            stq.initialize(*sch, *pair)
    # the Q stepper keeps refusing pi_logits and points to the new registry
    old, _ = _stepper(SelfPlayParallelStepper, q)
    with pytest.raises(NotImplementedError, match="agent_output_type.*SELF_POLICY_REGISTRY"):
        old.initialize(*sch, home, away)
    # B = 1
    one = SP.coma_sp_args("3v3", 32, True, n_envs=1, device="cpu")
    s1, i1 = _stepper(SelfPlayPolicyStepper, one)
    sch1, h1, a1 = _macs(one, i1)
    s1.initialize(*sch1, h1, a1)
    assert s1.describe_rollout()[0] == "sp-policy-lds/tpw1" and s1.batch_size == 1


def test_dqn_agent_under_pi_logits_is_refused_by_name():
    from maleague.steppers import SelfPlayPolicyParallelStepper
    pi = SP.coma_sp_args("3v3", 32, True, device="cpu")
    st, info = _stepper(SelfPlayPolicyParallelStepper, pi)
    sch, home, away = _macs(pi, info)
    dq = SP.coma_sp_args("3v3", 32, True, device="cpu", agent="dqn")
    dq.n_agents, dq.n_actions, dq.state_shape = pi.n_agents, pi.n_actions, pi.state_shape
    _, hd, _ = _macs(dq, info)
    with pytest.raises(NotImplementedError, match="agent='rnn'"):
        st.initialize(*sch, hd, away)


def test_experiment_picks_the_registry_by_output_type():
    from maleague.runs.sp_ma_experiment import SelfPlayMultiAgentExperiment
    from maleague.steppers import SelfPlayParallelStepper, SelfPlayPolicyParallelStepper
    for args, cls in ((SP.coma_sp_args("3v3", 32, True, device="cpu", runner="parallel"), SelfPlayPolicyParallelStepper),
                      (qmix_args(batch_size_run=SP.B, env_args=SP.env_args("3v3"), device="cpu", runner="parallel"),
                       SelfPlayParallelStepper)):
        exp = SelfPlayMultiAgentExperiment.__new__(SelfPlayMultiAgentExperiment)
        from maleague.custom_logging import MainLogger
        exp.args, exp.logger = args, MainLogger()
        assert type(exp._build_stepper()) is cls


def test_evaluator_selection_and_refusals():
    from maleague.league.evaluation import CrossPlayEvaluator, PolicyCrossPlayEvaluator, evaluator_for
    pi, q = coma_args(device="cpu"), qmix_args(device="cpu")
    assert type(evaluator_for(pi, "cpu")) is PolicyCrossPlayEvaluator
    assert issubclass(PolicyCrossPlayEvaluator, CrossPlayEvaluator)
    assert type(evaluator_for(q, "cpu")) is CrossPlayEvaluator
    with pytest.raises(NotImplementedError, match="agent_output_type.*PolicyCrossPlayEvaluator"):
        CrossPlayEvaluator(pi, "cpu")
    with pytest.raises(NotImplementedError, match="agent_output_type"):
        PolicyCrossPlayEvaluator(q, "cpu")
    for kw, word in (({"agent": "dqn"}, "agent='rnn'"), ({"mac": "distinct"}, "distinct")):
        with pytest.raises(NotImplementedError, match=word):
            PolicyCrossPlayEvaluator(coma_args(device="cpu", **kw), "cpu")


def test_league_instance_refuses_a_pi_logits_mixture_at_construction():
    from maleague.league import DistributedLeague, LeagueInstance
    lg = DistributedLeague(n_players=2, device="cpu", seed=0, player_id=0)
    args = SimpleNamespace(matchmaking="pfsp", env_args={}, agent_output_type="pi_logits")
    with pytest.raises(NotImplementedError, match="pi_logits"):
        LeagueInstance(args, None, lg, experiment=object(), opponents_per_match=2)
    LeagueInstance(args, None, lg, experiment=object(), opponents_per_match=1)
    args.agent_output_type = "q"
    LeagueInstance(args, None, lg, experiment=object(), opponents_per_match=2)


def test_coma_learner_counts_trained_steps_on_the_agent_counter():
    """The source of COMALearner.train adds the mask count to the agent's counter (checked on the GPU in
    tests/test_gpu_coma_league.py); add_trained_steps with a tensor accumulates without a host read."""
    from maleague.modules.agents import DRQNAgentNetwork
    a = DRQNAgentNetwork(20, SimpleNamespace(rnn_hidden_dim=32, n_actions=11))
    a.add_trained_steps(torch.count_nonzero(torch.tensor([[1.0, 0.0, 1.0]])))
    a.add_trained_steps(torch.count_nonzero(torch.ones(4)))
    assert a.trained_steps == 6


# ---- the conditions on the inputs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["3v3-h32", "3v3-h128"])
def test_near_tie_conditions_of_the_smallest_cases(cid):
    """The float64 oracle alone at the greedy run (episode 2): at most 1 % near ties on each side where the case lists
    the mask, the shares written beside the case, and at least 2 envs ending before the limit."""
    c = SP.case(cid)
    want = {("3v3-h32", True): ((1, 0), 1776, 7), ("3v3-h32", False): ((15, 4), 1776, 7),
            ("3v3-h128", True): ((0, 0), 1752, 6), ("3v3-h128", False): ((5, 48), 1752, 6)}
    for mask in (True, False):
        ep_len, picks, near = SP.oracle_run(c.plan, c.H, mask, "greedy", SP.EP_GREEDY)
        early = int((ep_len < SP.EPISODE_LIMIT).sum())
        assert (tuple(near), picks[0], early) == want[cid, mask] and picks[0] == picks[1]
        ok = max(near[s] / picks[s] for s in range(2)) <= SP.ORACLE_NEAR_TIE_CAP
        assert ok == (mask in c.greedy), (cid, mask, near, picks)
        assert early >= SP.MIN_EARLY
    assert SP.ORACLE_NEAR_TIE_CAP == 0.01 and SP.NEAR_TIE_CAP == 0.02 and SP.DELTA == 2e-4 and SP.MIN_EARLY == 2
