"""Distinct per-agent networks in self-play, the league and cross-play on the CPU (no GPU call): the dispatch table of
mlg_rollout_selfplay_distinct pinned through its host-only query, the refusals by message, the ABI of the new entry
points, the stepper registry and what SelfPlayMultiAgentExperiment._build_stepper picks, agent vectors of a DistinctMAC,
the evaluator and league-instance selection and the mixture refusals. Cases: tests/distinct_selfplay_shapes.py."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

import distinct_selfplay_shapes as DSP
from helpers import qmix_args, scheme_for, sp_args

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maleague.h")


class _Log:
    test_mode = False

    def info(self, *_a, **_k):
        pass

    def log_stat(self, *_a, **_k):
        pass


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from maleague import _native
    lib = _native.load()
    src = open(HEADER).read()
    for sym in ("mlg_rollout_selfplay_distinct", "mlg_rollout_selfplay_distinct_describe",
                "mlg_crossplay_rollout_distinct"):
        assert re.search(r"\b" + sym + r"\s*\(", src) and hasattr(lib, sym) and sym in _native.SIGNATURES
    # mlg_rollout_selfplay's and mlg_crossplay_rollout's argument lists
    assert list(_native.SIGNATURES["mlg_rollout_selfplay_distinct"][1]) == \
        list(_native.SIGNATURES["mlg_rollout_selfplay"][1])
    assert list(_native.SIGNATURES["mlg_crossplay_rollout_distinct"][1]) == \
        list(_native.SIGNATURES["mlg_crossplay_rollout"][1])


# ---- mlg_rollout_selfplay_distinct_describe -------------------------------------------------------------------------
def test_describe_table():
    from maleague import _native
    for cid, hidden, plan, la, arm, seed, _ in DSP.CASES:
        spec = DSP.spec_of(plan, seed)
        name, lds = _native.rollout_selfplay_distinct_describe(spec.to_c(), DSP.dims_of(spec, hidden, la))
        assert name == arm, cid
        assert 0 < lds <= 64 * 1024  # the env part only: weights stay in global memory
    for nh, arm in DSP.DESCRIBE:
        spec = DSP.spec_of(f"{nh}v{nh}")
        assert spec.n_agents == 2 * nh
        for hidden in (32, 64, 128):
            if arm is None:
                with pytest.raises(_native.NativeError, match=r"34 agent tiles \(one per agent, 17 per side\) > 32"):
                    _native.rollout_selfplay_distinct_describe(spec.to_c(), DSP.dims_of(spec, hidden))
            else:
                assert _native.rollout_selfplay_distinct_describe(spec.to_c(), DSP.dims_of(spec, hidden))[0] == arm
    assert {c[4] for c in DSP.CASES} == {f"dxsp-global/tpw{k}" for k in (1, 2, 3, 4)}
    assert {c[1] for c in DSP.CASES} == {32, 64, 128}
    assert set(DSP.RING_CASES) | set(DSP.SHARED_CASES) <= set(DSP.IDS) and DSP.EPS != DSP.EPS_AWAY


def test_rejections_by_message():
    """Every refusal comes through mlg_last_error before a pointer is read or anything is launched (no GPU needed)."""
    from maleague import _native
    from maleague.envs.teams_env import TeamsEnvSpec
    lib = _native.load()
    spec = DSP.spec_of("small")
    cs = spec.to_c()
    d = DSP.dims_of(spec, 64)
    with pytest.raises(_native.NativeError, match="obs_agent_id must be 0"):
        _native.rollout_selfplay_distinct_describe(cs, DSP.dims_of(spec, 64, agent_id=True))
    for hidden in (16, 48, 256):
        with pytest.raises(_native.NativeError, match="rnn_hidden_dim"):
            _native.rollout_selfplay_distinct_describe(cs, DSP.dims_of(spec, hidden))
    both = _native.MlgAgentDims(d_obs=8 * spec.U, n_actions=spec.n_actions, n_agents=spec.n_agents, hidden=64,
                                d_in=8 * spec.U + spec.n_actions, obs_last_action=1, obs_agent_id=0)
    with pytest.raises(_native.NativeError, match="agent dims do not match one side"):
        _native.rollout_selfplay_distinct_describe(cs, both)  # both sides' agents as one MAC
    ai = TeamsEnvSpec.from_env_args({"match_build_plan": "small", "grid_size": 8, "episode_limit": 40})
    ai_d = _native.MlgAgentDims(d_obs=8 * ai.U, n_actions=ai.n_actions, n_agents=ai.n_agents, hidden=64,
                                d_in=8 * ai.U + ai.n_actions, obs_last_action=1, obs_agent_id=0)
    with pytest.raises(_native.NativeError, match="two-team scenario"):
        _native.rollout_selfplay_distinct_describe(ai.to_c(), ai_d)
    name, lds = ctypes.create_string_buffer(4), ctypes.c_int64(0)
    assert lib.mlg_rollout_selfplay_distinct_describe(ctypes.byref(cs), ctypes.byref(d), name, len(name),
                                                      ctypes.byref(lds)) != 0
    assert b"too small" in lib.mlg_last_error()
    assert lib.mlg_rollout_selfplay_distinct_describe(ctypes.byref(cs), ctypes.byref(d), None, 0, None) != 0
    assert b"null output" in lib.mlg_last_error()
    # the launch entry point: null pointers, then the agent id, each before anything else is read
    assert lib.mlg_rollout_selfplay_distinct(ctypes.byref(cs), None, None, None, None, None, None, None, 0.0, 0.0, 1,
                                             None) != 0
    assert b"null" in lib.mlg_last_error()
    st = _native.MlgEnvState(1, 1, 1, 1, 1, 4)  # never dereferenced: the dims and the pools are checked first
    bad = DSP.dims_of(spec, 64, agent_id=True)
    assert lib.mlg_rollout_selfplay_distinct(ctypes.byref(cs), ctypes.byref(st), ctypes.byref(bad), None, None, None,
                                             None, None, 0.0, 0.0, 1, None) != 0
    assert b"rollout_selfplay_distinct: obs_agent_id must be 0" in lib.mlg_last_error()
    assert lib.mlg_rollout_selfplay_distinct(ctypes.byref(cs), ctypes.byref(st), ctypes.byref(d), None, None, None,
                                             None, None, 0.0, 0.0, 1, None) != 0
    assert b"rollout_selfplay_distinct: null pointer" in lib.mlg_last_error()
    # cross-play
    assert lib.mlg_crossplay_rollout_distinct(ctypes.byref(d), None, None) != 0
    assert b"crossplay: null argument block" in lib.mlg_last_error()
    c = _native.MlgCrossplay()
    assert lib.mlg_crossplay_rollout_distinct(ctypes.byref(bad), ctypes.byref(c), None) != 0
    assert b"crossplay_distinct: obs_agent_id must be 0" in lib.mlg_last_error()


# ---- Python: registries, refusals -----------------------------------------------------------------------------------
def _stepper(cls, args):
    stepper = cls(args, _Log())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    return stepper, info


def _macs(args, info, kinds=("distinct", "distinct")):
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import REGISTRY
    scheme, groups, preprocess = scheme_for(dict(info, n_agents=args.n_agents), torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device="cpu")
    return (scheme, groups, preprocess), [REGISTRY[k](proto.scheme, groups, args) for k in kinds]


def _dx_args(B=4, plan="small", **kw):
    return sp_args(B, 10, 1, plan=plan, device="cpu", mac="distinct", obs_agent_id=False, **kw)


def test_registries_and_stepper_refusals():
    from maleague import steppers
    from maleague.steppers import (SELF_DISTINCT_REGISTRY, SELF_REGISTRY, OpponentMix, SelfPlayDistinctParallelStepper,
                                   SelfPlayDistinctStepper, SelfPlayParallelStepper, SelfPlayStepper)
    assert SELF_DISTINCT_REGISTRY == {"parallel": SelfPlayDistinctParallelStepper, "episode": SelfPlayDistinctStepper}
    assert SELF_REGISTRY == {"parallel": SelfPlayParallelStepper, "episode": SelfPlayStepper}
    assert "SELF_DISTINCT_REGISTRY" in steppers.__all__
    assert issubclass(SelfPlayDistinctStepper, SelfPlayDistinctParallelStepper)
    assert issubclass(SelfPlayDistinctParallelStepper, SelfPlayParallelStepper)
    args = _dx_args()
    st, info = _stepper(SelfPlayDistinctParallelStepper, args)
    sch, (home, away) = _macs(args, info)
    st.initialize(*sch, home, away)
    assert st.describe_rollout()[0] == "dxsp-global/tpw1"
    # mixtures over distinct MACs are refused by name; None stays a no-op
    with pytest.raises(NotImplementedError, match="mixtures with mac='distinct'"):
        st.set_opponent_mix(OpponentMix(torch.zeros(1, 4), [0]))
    st.set_opponent_mix(None)
    # a distinct side against a parameter-shared side, either way round, and a missing away MAC
    _, (basic,) = _macs(args, info, kinds=("basic",))
    for pair in ((home, basic), (basic, away), (basic, basic)):
        with pytest.raises(NotImplementedError, match="two DistinctMACs.*BasicMAC"):
            st.initialize(*sch, *pair)
    with pytest.raises(ValueError, match="away MAC"):
        st.initialize(*sch, home)
    # unequal dims
    wide = _dx_args(rnn_hidden_dim=32)
    wide.n_agents, wide.n_actions, wide.state_shape = args.n_agents, args.n_actions, args.state_shape
    _, (other,) = _macs(wide, info, kinds=("distinct",))
    with pytest.raises(ValueError, match="same architecture"):
        st.initialize(*sch, home, other)
    # the old steppers keep refusing and name the class that runs it
    old, _ = _stepper(SelfPlayParallelStepper, _dx_args())
    with pytest.raises(NotImplementedError, match="mac='distinct'.*SelfPlayDistinctParallelStepper.*"
                                                  "SELF_DISTINCT_REGISTRY"):
        old.initialize(*sch, home, away)
    # B = 1
    one = _dx_args(B=1)
    s1, i1 = _stepper(SelfPlayDistinctStepper, one)
    sch1, (h1, a1) = _macs(one, i1)
    s1.initialize(*sch1, h1, a1)
    assert s1.describe_rollout()[0] == "dxsp-global/tpw1" and s1.batch_size == 1
    # 5 agents per side: the tpw2 arm
    five = _dx_args(plan="medium_1h_4t")
    s5, i5 = _stepper(SelfPlayDistinctParallelStepper, five)
    sch5, (h5, a5) = _macs(five, i5)
    s5.initialize(*sch5, h5, a5)
    assert s5.describe_rollout()[0] == "dxsp-global/tpw2"


def test_experiment_picks_the_registry_by_mac():
    from maleague.runs.sp_ma_experiment import SelfPlayMultiAgentExperiment
    from maleague.steppers import (SelfPlayDistinctParallelStepper, SelfPlayDistinctStepper, SelfPlayParallelStepper)
    for args, cls in ((_dx_args(runner="parallel"), SelfPlayDistinctParallelStepper),
                      (_dx_args(B=1, runner="episode"), SelfPlayDistinctStepper),
                      (sp_args(4, 10, 1, plan="small", device="cpu", runner="parallel"), SelfPlayParallelStepper)):
        exp = SelfPlayMultiAgentExperiment.__new__(SelfPlayMultiAgentExperiment)
        exp.args, exp.logger = args, _Log()
        assert type(exp._build_stepper()) is cls


# ---- agent vectors --------------------------------------------------------------------------------------------------
def test_agent_vector_round_trip_and_wrong_length():
    """The N networks back to back, agent 0 first, each in named_parameters() order; a load is followed by
    mark_dirty(); a vector of the wrong length raises ValueError. On separate parameters and on one flat buffer."""
    from maleague.learners.q_learner import FlatParams
    from maleague.runs.sp_ma_experiment import agent_vector, load_agent_vector
    args = _dx_args()
    _, info = _stepper(__import__("maleague.steppers", fromlist=["x"]).SelfPlayDistinctParallelStepper, args)
    _, (src, dst, flat_dst) = _macs(args, info, kinds=("distinct",) * 3)
    FlatParams(flat_dst.agents.parameters(), "cpu")  # as the experiment re-homes the away MAC's parameters
    want = torch.cat([p.detach().reshape(-1) for a in src.agents for _, p in a.named_parameters()])
    n_params = sum(p.numel() for p in src.agents[0].parameters())
    vec = agent_vector(src)
    assert vec.numel() == args.n_agents * n_params and torch.equal(vec, want)
    assert agent_vector(flat_dst).data_ptr() == flat_dst.agents[0].fc1.weight.data_ptr()  # a view of the flat buffer
    for mac in (dst, flat_dst):
        assert not torch.equal(agent_vector(mac), want)
        dirty0 = [a._dirty for a in mac.agents]
        load_agent_vector(mac, vec.clone())
        assert torch.equal(agent_vector(mac), want)
        assert all(a._dirty != d for a, d in zip(mac.agents, dirty0)), "mark_dirty() did not follow the load"
        for a, b in zip(mac.agents, src.agents):
            for (k, v), (_, w) in zip(a.state_dict().items(), b.state_dict().items()):
                assert torch.equal(v, w), k
        for bad in (vec[:-1], torch.cat([vec, vec[:1]]), vec[:n_params]):
            with pytest.raises(ValueError, match="parameter vector of"):
                load_agent_vector(mac, bad)
    # the shared-agent path is unchanged
    _, (basic,) = _macs(args, info, kinds=("basic",))
    bvec = agent_vector(basic)
    assert bvec.numel() == sum(p.numel() for p in basic.agent.parameters())
    with pytest.raises(ValueError, match="parameter vector of"):
        load_agent_vector(basic, bvec[:-1])


# ---- evaluator and league instance ----------------------------------------------------------------------------------
def test_evaluator_selection_and_refusals():
    from maleague.league.evaluation import (CrossPlayEvaluator, DistinctCrossPlayEvaluator, PolicyCrossPlayEvaluator,
                                            evaluator_for)
    dx = qmix_args(device="cpu", mac="distinct", obs_agent_id=False)
    q = qmix_args(device="cpu")
    ev = evaluator_for(dx, "cpu")
    assert type(ev) is DistinctCrossPlayEvaluator and issubclass(DistinctCrossPlayEvaluator, CrossPlayEvaluator)
    assert type(evaluator_for(q, "cpu")) is CrossPlayEvaluator
    with pytest.raises(NotImplementedError, match="mac='distinct'.*DistinctCrossPlayEvaluator"):
        CrossPlayEvaluator(dx, "cpu")
    with pytest.raises(NotImplementedError, match="mac='distinct' policies only"):
        DistinctCrossPlayEvaluator(q, "cpu")
    # pi_logits under mac=distinct stays refused: the policy evaluator is picked and refuses the MAC by name
    with pytest.raises(NotImplementedError, match="mac='distinct'"):
        evaluator_for(qmix_args(device="cpu", mac="distinct", agent_output_type="pi_logits"), "cpu")
    assert PolicyCrossPlayEvaluator is not DistinctCrossPlayEvaluator
    # dims_of: one side's dims with the agent id off, whatever args say
    spec = DSP.spec_of("small")
    for flag in (False, True):
        dx.obs_agent_id = flag
        d = ev.dims_of(spec)
        assert (d.n_agents, d.obs_agent_id, d.d_in) == (3, 0, 8 * spec.U + spec.n_actions)


def test_league_instance_selection_and_mixture_refusal():
    from maleague.league import DistinctLeagueInstance, DistributedLeague, LeagueInstance, league_instance_for
    lg = DistributedLeague(n_players=2, device="cpu", seed=0, player_id=0)
    dx = SimpleNamespace(matchmaking="pfsp", env_args={}, agent_output_type="q", mac="distinct")
    q = SimpleNamespace(matchmaking="pfsp", env_args={}, agent_output_type="q")
    assert issubclass(DistinctLeagueInstance, LeagueInstance)
    with pytest.raises(NotImplementedError, match="mac='distinct'.*DistinctLeagueInstance"):
        LeagueInstance(dx, None, lg, experiment=object())
    inst = DistinctLeagueInstance(dx, None, lg, experiment=object())  # constructs where LeagueInstance refuses
    assert inst.opponents_per_match == 1 and inst.pid == 0
    assert type(league_instance_for(dx, None, lg, experiment=object())) is DistinctLeagueInstance
    assert type(league_instance_for(q, None, lg, experiment=object(), opponents_per_match=2)) is LeagueInstance
    for make in (DistinctLeagueInstance, league_instance_for):
        with pytest.raises(NotImplementedError, match="mixtures with mac='distinct'"):
            make(dx, None, lg, experiment=object(), opponents_per_match=2)
    with pytest.raises(NotImplementedError, match="mac='distinct' only"):
        DistinctLeagueInstance(q, None, lg, experiment=object())


def test_distributed_league_carries_rows_of_n_networks():
    """The pool's row width is whatever the exchanged vector holds (N x n_params for a DistinctMAC): no assumption of
    one network."""
    from maleague.league import DistributedLeague
    lg = DistributedLeague(n_players=2, device="cpu", seed=0, player_id=1, max_historical=1)
    n_params, N = 37, 3
    lg.set_player_params(0, torch.arange(N * n_params, dtype=torch.float32))
    mine = torch.arange(N * n_params, dtype=torch.float32) * 2
    lg.exchange(mine, 5, checkpoint=True)
    assert tuple(lg.current.shape) == (2, N * n_params) and tuple(lg.historical.shape) == (1, N * n_params)
    assert torch.equal(lg.params_of(1), mine) and torch.equal(lg.params_of(2), mine)
