"""The feed-forward agent (agent: dqn) in self-play, the league and cross-play on the CPU (no GPU call): the dispatch
table of mlg_rollout_selfplay_ff pinned through its host-only query, the host refusals by message, the ABI of the new
entry points, mlg_ff_pack_pool's argument checks, the stepper registry and what SelfPlayMultiAgentExperiment
._build_stepper picks, the evaluator selection, what each new class refuses and that the old classes still refuse dqn,
and the near-tie condition of the float64 oracle for two cases. Cases: tests/dqn_selfplay_shapes.py."""
import ctypes
import os
import re

import pytest
import torch

import dqn_selfplay_shapes as FSP
from helpers import qmix_args, scheme_for, sp_args

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maleague.h")
SYMBOLS = ("mlg_ff_pack_pool", "mlg_rollout_selfplay_ff", "mlg_rollout_selfplay_ff_describe",
           "mlg_crossplay_ff_workspace_floats", "mlg_crossplay_rollout_ff")


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
    for sym in SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", src) and hasattr(lib, sym) and sym in _native.SIGNATURES, sym
    sig = _native.SIGNATURES
    # the argument lists of the entry points they follow
    assert list(sig["mlg_rollout_selfplay_ff"][1]) == list(sig["mlg_rollout_selfplay"][1])
    assert list(sig["mlg_crossplay_rollout_ff"][1]) == list(sig["mlg_crossplay_rollout"][1])
    assert list(sig["mlg_crossplay_ff_workspace_floats"][1]) == list(sig["mlg_crossplay_workspace_floats"][1])
    assert list(sig["mlg_ff_pack_pool"][1]) == list(sig["mlg_pack_agent_pool"][1])


# ---- mlg_rollout_selfplay_ff_describe -------------------------------------------------------------------------------
def test_describe_table(monkeypatch):
    from maleague import _native
    monkeypatch.delenv("MLG_ROLLOUT_GLOBAL_WEIGHTS", raising=False)
    for cid, hidden, plan, la, ai, arm, seed, _ in FSP.CASES:
        spec = FSP.spec_of(plan, seed)
        name, lds = _native.rollout_selfplay_ff_describe(spec.to_c(), FSP.dims_of(spec, hidden, la, ai))
        assert name == arm, cid
        assert 0 < lds <= 160 * 1024
        assert (lds > 20 * 1024) == arm.startswith("ffsp-lds"), (cid, lds)  # the env part alone stays under 20 KiB
    for nh, arms in FSP.DESCRIBE:
        spec = FSP.spec_of(f"{nh}v{nh}")
        assert spec.n_agents == 2 * nh
        for k, hidden in enumerate((32, 64, 128)):
            if arms is None:
                with pytest.raises(_native.NativeError, match=r"5 agent tiles per wave > 4 \(more than 16 agents per "
                                                              r"side\)"):
                    _native.rollout_selfplay_ff_describe(spec.to_c(), FSP.dims_of(spec, hidden))
            else:
                assert _native.rollout_selfplay_ff_describe(spec.to_c(), FSP.dims_of(spec, hidden))[0] == arms[k], \
                    (nh, hidden)
    arms = {c[5] for c in FSP.CASES}
    assert {f"ffsp-lds/tpw{k}" for k in (1, 2, 3, 4)} | {"ffsp-global/tpw3", "ffsp-global/tpw4"} == arms
    assert {a for _, a in FSP.LDS_VS_GLOBAL} == {"ffsp-global/tpw1", "ffsp-global/tpw2"}
    assert {c[1] for c in FSP.CASES} == {32, 64, 128}
    assert {(c[3], c[4]) for c in FSP.CASES} == {(True, True), (True, False), (False, True), (False, False)}
    assert set(FSP.RING_CASES) | set(FSP.ORACLE_CASES) | {c for c, _ in FSP.LDS_VS_GLOBAL} <= set(FSP.IDS)
    assert FSP.EPS != FSP.EPS_AWAY


def test_environment_variable_forces_the_global_arm(monkeypatch):
    from maleague import _native
    monkeypatch.setenv("MLG_ROLLOUT_GLOBAL_WEIGHTS", "1")
    for cid, hidden, plan, la, ai, arm, seed, _ in FSP.CASES:
        spec = FSP.spec_of(plan, seed)
        name, lds = _native.rollout_selfplay_ff_describe(spec.to_c(), FSP.dims_of(spec, hidden, la, ai))
        assert name == arm.replace("ffsp-lds", "ffsp-global"), cid
        assert 0 < lds <= 20 * 1024  # the env part only
    for cid, forced in FSP.LDS_VS_GLOBAL:
        _, hidden, plan, la, ai, arm, seed, _ = FSP.case(cid)
        spec = FSP.spec_of(plan, seed)
        assert arm.startswith("ffsp-lds")
        assert _native.rollout_selfplay_ff_describe(spec.to_c(), FSP.dims_of(spec, hidden, la, ai))[0] == forced


def test_rejections_by_message():
    """Every refusal comes through mlg_last_error before a pointer is read or anything is launched (no GPU needed)."""
    from maleague import _native
    from maleague.envs.teams_env import TeamsEnvSpec
    lib = _native.load()
    spec = FSP.spec_of("small")
    cs = spec.to_c()
    d = FSP.dims_of(spec, 64)
    for hidden in (16, 48, 256):
        with pytest.raises(_native.NativeError, match="rnn_hidden_dim"):
            _native.rollout_selfplay_ff_describe(cs, FSP.dims_of(spec, hidden))
    both = _native.MlgAgentDims(d_obs=8 * spec.U, n_actions=spec.n_actions, n_agents=spec.n_agents, hidden=64,
                                d_in=8 * spec.U + spec.n_actions + spec.n_agents, obs_last_action=1, obs_agent_id=1)
    with pytest.raises(_native.NativeError, match="rollout_selfplay_ff: agent dims do not match one side"):
        _native.rollout_selfplay_ff_describe(cs, both)  # both sides' agents as one MAC
    ai = TeamsEnvSpec.from_env_args({"match_build_plan": "small", "grid_size": 8, "episode_limit": 40})
    ai_d = _native.MlgAgentDims(d_obs=8 * ai.U, n_actions=ai.n_actions, n_agents=ai.n_agents, hidden=64,
                                d_in=8 * ai.U + ai.n_actions + ai.n_agents, obs_last_action=1, obs_agent_id=1)
    with pytest.raises(_native.NativeError, match="rollout_selfplay_ff: .*two-team scenario"):
        _native.rollout_selfplay_ff_describe(ai.to_c(), ai_d)
    name, lds = ctypes.create_string_buffer(4), ctypes.c_int64(0)
    assert lib.mlg_rollout_selfplay_ff_describe(ctypes.byref(cs), ctypes.byref(d), name, len(name),
                                                ctypes.byref(lds)) != 0
    assert b"too small" in lib.mlg_last_error()
    assert lib.mlg_rollout_selfplay_ff_describe(ctypes.byref(cs), ctypes.byref(d), None, 0, None) != 0
    assert b"null output" in lib.mlg_last_error()
    # the launch entry point: null pointers before anything else is read
    assert lib.mlg_rollout_selfplay_ff(ctypes.byref(cs), None, None, None, None, None, None, None, 0.0, 0.0, 1,
                                       None) != 0
    assert b"null" in lib.mlg_last_error()
    st = _native.MlgEnvState(1, 1, 1, 1, 1, 4)  # never dereferenced: the weights are checked first
    assert lib.mlg_rollout_selfplay_ff(ctypes.byref(cs), ctypes.byref(st), ctypes.byref(d), None, None, None, None,
                                       None, 0.0, 0.0, 1, None) != 0
    assert b"rollout_selfplay_ff: null pointer" in lib.mlg_last_error()
    # cross-play: mlg_crossplay_rollout's checks
    assert lib.mlg_crossplay_rollout_ff(ctypes.byref(d), None, None) != 0
    assert b"crossplay: null argument block" in lib.mlg_last_error()
    c = _native.MlgCrossplay()
    assert lib.mlg_crossplay_rollout_ff(ctypes.byref(d), ctypes.byref(c), None) != 0
    assert b"crossplay: null pool / pairs / specs / workspace pointer" in lib.mlg_last_error()
    assert lib.mlg_crossplay_ff_workspace_floats(ctypes.byref(d), 0, 4) == -1
    assert b"must be >= 1" in lib.mlg_last_error()
    assert lib.mlg_crossplay_ff_workspace_floats(ctypes.byref(d), 9, 20) == \
        lib.mlg_crossplay_workspace_floats(ctypes.byref(d), 9, 20) == 4


def test_ff_pack_pool_argument_checks():
    from maleague import _native
    lib = _native.load()
    spec = FSP.spec_of("small")
    d = FSP.dims_of(spec, 64)
    n_params = 64 * d.d_in + 64 + d.n_actions * 64 + d.n_actions
    one = ctypes.c_void_p(16)  # never dereferenced: every check below fails before the launch
    assert lib.mlg_ff_pack_pool(ctypes.byref(d), None, n_params, 1, one, None) != 0
    assert b"ff_pack_pool: null pointer" in lib.mlg_last_error()
    assert lib.mlg_ff_pack_pool(ctypes.byref(d), one, n_params, 1, None, None) != 0
    assert b"ff_pack_pool: null pointer" in lib.mlg_last_error()
    for P in (0, -3):
        assert lib.mlg_ff_pack_pool(ctypes.byref(d), one, n_params, P, one, None) != 0
        assert f"ff_pack_pool: P={P} must be".encode() in lib.mlg_last_error()
    assert lib.mlg_ff_pack_pool(ctypes.byref(d), one, n_params - 1, 2, one, None) != 0
    assert f"ff_pack_pool: row_stride={n_params - 1} < {n_params} parameters".encode() in lib.mlg_last_error()
    bad = FSP.dims_of(spec, 48)
    assert lib.mlg_ff_pack_pool(ctypes.byref(bad), one, n_params, 1, one, None) != 0


# ---- Python: registries, refusals -----------------------------------------------------------------------------------
def _stepper(cls, args):
    stepper = cls(args, _Log())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    return stepper, info


def _macs(args, info, kinds=("dqn", "dqn")):
    """MACs over ``args``: 'dqn' / 'rnn' a BasicMAC with that agent, 'distinct' a DistinctMAC (no agent id),
    'pi' a BasicMAC of the feed-forward agent with pi_logits outputs."""
    import copy
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import REGISTRY
    scheme, groups, preprocess = scheme_for(dict(info, n_agents=args.n_agents), torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device="cpu")
    macs = []
    for k in kinds:
        a = copy.copy(args)
        if k == "distinct":
            a.agent, a.mac, a.obs_agent_id = "rnn", "distinct", False
        elif k == "pi":
            a.agent_output_type, a.action_selector = "pi_logits", "multinomial"
        else:
            a.agent = k
        macs.append(REGISTRY[getattr(a, "mac", "basic")](proto.scheme, groups, a))
    return (scheme, groups, preprocess), macs


def _ff_args(B=4, plan="small", **kw):
    return sp_args(B, 10, 1, plan=plan, device="cpu", agent="dqn", mac="basic", **kw)


def test_registries_and_stepper_refusals():
    from maleague import steppers
    from maleague.modules.agents import DQNAgentNetwork
    from maleague.steppers import (SELF_FF_REGISTRY, SELF_REGISTRY, OpponentMix, SelfPlayFFParallelStepper,
                                   SelfPlayFFStepper, SelfPlayParallelStepper, SelfPlayPolicyParallelStepper,
                                   SelfPlayDistinctParallelStepper, SelfPlayStepper)
    assert SELF_FF_REGISTRY == {"parallel": SelfPlayFFParallelStepper, "episode": SelfPlayFFStepper}
    assert SELF_REGISTRY == {"parallel": SelfPlayParallelStepper, "episode": SelfPlayStepper}
    assert {"SELF_FF_REGISTRY", "SelfPlayFFParallelStepper", "SelfPlayFFStepper"} <= set(steppers.__all__)
    assert issubclass(SelfPlayFFStepper, SelfPlayFFParallelStepper)
    assert issubclass(SelfPlayFFParallelStepper, SelfPlayParallelStepper)
    args = _ff_args()
    st, info = _stepper(SelfPlayFFParallelStepper, args)
    sch, (home, away) = _macs(args, info)
    assert isinstance(home.agent, DQNAgentNetwork)
    st.initialize(*sch, home, away)
    assert st.describe_rollout()[0] == "ffsp-lds/tpw1"
    # mixtures over feed-forward MACs are refused by name; None stays a no-op
    with pytest.raises(NotImplementedError, match="mixtures with agent='dqn'.*mlg_rollout_selfplay_mix packs"):
        st.set_opponent_mix(OpponentMix(torch.zeros(1, 4), [0]))
    st.set_opponent_mix(None)
    # a feed-forward side against a recurrent side, either way round
    _, (rnn,) = _macs(args, info, kinds=("rnn",))
    for pair, side in (((home, rnn), "away"), ((rnn, away), "home"), ((rnn, rnn), "home")):
        with pytest.raises(NotImplementedError, match=f"the {side} MAC's agent is a DRQNAgentNetwork .*"
                                                      "SelfPlayParallelStepper, steppers.SELF_REGISTRY"):
            st.initialize(*sch, *pair)
    # pi_logits and DistinctMACs, each naming the class that runs the recurrent form
    _, (pi,) = _macs(args, info, kinds=("pi",))
    with pytest.raises(NotImplementedError, match="agent_output_type='pi_logits'.*SelfPlayPolicyParallelStepper"):
        st.initialize(*sch, home, pi)
    _, (dx,) = _macs(args, info, kinds=("distinct",))
    with pytest.raises(NotImplementedError, match="mac='distinct'.*SelfPlayDistinctParallelStepper"):
        st.initialize(*sch, dx, away)
    with pytest.raises(ValueError, match="away MAC"):
        st.initialize(*sch, home)
    # the old steppers keep refusing dqn, by the same message
    for cls in (SelfPlayParallelStepper, SelfPlayPolicyParallelStepper, SelfPlayDistinctParallelStepper):
        old, _ = _stepper(cls, _ff_args())
        with pytest.raises(NotImplementedError):
            old.initialize(*sch, home, away)
    old, _ = _stepper(SelfPlayParallelStepper, _ff_args())
    with pytest.raises(NotImplementedError, match="the home MAC's DQNAgentNetwork is not supported .agent='dqn'"):
        old.initialize(*sch, home, away)
    # B = 1
    one = _ff_args(B=1)
    s1, i1 = _stepper(SelfPlayFFStepper, one)
    sch1, (h1, a1) = _macs(one, i1)
    s1.initialize(*sch1, h1, a1)
    assert s1.describe_rollout()[0] == "ffsp-lds/tpw1" and s1.batch_size == 1
    # 5 agents per side: the tpw2 arm
    five = _ff_args(plan="medium_1h_4t")
    s5, i5 = _stepper(SelfPlayFFParallelStepper, five)
    sch5, (h5, a5) = _macs(five, i5)
    s5.initialize(*sch5, h5, a5)
    assert s5.describe_rollout()[0] == "ffsp-lds/tpw2"


def test_experiment_picks_the_registry_by_agent():
    """Selection order: mac 'distinct', else pi_logits, else agent 'dqn', else the recurrent Q steppers."""
    from maleague.runs.sp_ma_experiment import SelfPlayMultiAgentExperiment
    from maleague.steppers import (SelfPlayDistinctParallelStepper, SelfPlayFFParallelStepper, SelfPlayFFStepper,
                                   SelfPlayParallelStepper, SelfPlayPolicyParallelStepper)
    plain = dict(plan="small", device="cpu", runner="parallel")
    for args, cls in ((_ff_args(runner="parallel"), SelfPlayFFParallelStepper),
                      (_ff_args(B=1, runner="episode"), SelfPlayFFStepper),
                      (sp_args(4, 10, 1, **plain), SelfPlayParallelStepper),
                      (sp_args(4, 10, 1, agent="dqn", agent_output_type="pi_logits", **plain),
                       SelfPlayPolicyParallelStepper),
                      (sp_args(4, 10, 1, agent="dqn", mac="distinct", **plain), SelfPlayDistinctParallelStepper)):
        exp = SelfPlayMultiAgentExperiment.__new__(SelfPlayMultiAgentExperiment)
        exp.args, exp.logger = args, _Log()
        assert type(exp._build_stepper()) is cls


def test_evaluator_selection_and_refusals():
    from maleague.league.evaluation import (CrossPlayEvaluator, DistinctCrossPlayEvaluator, FFCrossPlayEvaluator,
                                            PolicyCrossPlayEvaluator, evaluator_for)
    ff = qmix_args(device="cpu", agent="dqn")
    q = qmix_args(device="cpu")
    ev = evaluator_for(ff, "cpu")
    assert type(ev) is FFCrossPlayEvaluator and issubclass(FFCrossPlayEvaluator, CrossPlayEvaluator)
    assert type(evaluator_for(q, "cpu")) is CrossPlayEvaluator
    with pytest.raises(NotImplementedError, match=r"agent='dqn'\) only, got agent='rnn'.*CrossPlayEvaluator"):
        FFCrossPlayEvaluator(q, "cpu")
    with pytest.raises(NotImplementedError, match="agent='entity_attend_rnn'.*CrossPlayEvaluator"):
        FFCrossPlayEvaluator(qmix_args(device="cpu", agent="entity_attend_rnn"), "cpu")
    # the old evaluators still refuse dqn, by the unchanged message
    msg = "agent='dqn' is not supported .agent='dqn' and the other non-DRQN agents in cross-play are out of scope"
    with pytest.raises(NotImplementedError, match=msg):
        CrossPlayEvaluator(ff, "cpu")
    with pytest.raises(NotImplementedError, match=msg):
        PolicyCrossPlayEvaluator(qmix_args(device="cpu", agent="dqn", agent_output_type="pi_logits"), "cpu")
    with pytest.raises(NotImplementedError, match=msg):
        DistinctCrossPlayEvaluator(qmix_args(device="cpu", agent="dqn", mac="distinct", obs_agent_id=False), "cpu")
    # COMA over dqn and dqn under mac: distinct stay refused through evaluator_for as well
    with pytest.raises(NotImplementedError, match=msg):
        evaluator_for(qmix_args(device="cpu", agent="dqn", agent_output_type="pi_logits"), "cpu")
    with pytest.raises(NotImplementedError, match=msg):
        evaluator_for(qmix_args(device="cpu", agent="dqn", mac="distinct", obs_agent_id=False), "cpu")
    with pytest.raises(NotImplementedError, match="agent_output_type='pi_logits'"):
        FFCrossPlayEvaluator(qmix_args(device="cpu", agent="dqn", agent_output_type="pi_logits"), "cpu")
    with pytest.raises(NotImplementedError, match="mac='distinct'"):
        FFCrossPlayEvaluator(qmix_args(device="cpu", agent="dqn", mac="distinct"), "cpu")
    # dims_of: one side's dims with the flags of args
    spec = FSP.spec_of("small")
    d = ev.dims_of(spec)
    assert (d.n_agents, d.obs_agent_id, d.d_in) == (3, 1, 8 * spec.U + spec.n_actions + 3)
    # the size hooks: the feed-forward block is the DRQN block without the GRU part
    from maleague import _native
    lib = _native.load()
    base = CrossPlayEvaluator(q, "cpu")
    assert 0 < ev._packed_size(lib, d) == lib.mlg_ff_packed_size(_native.byref(d)) < base._packed_size(lib, d)
    assert ev._workspace_floats(lib, d, 9, 20) == base._workspace_floats(lib, d, 9, 20) == 4


def test_league_instance_refuses_mixtures_with_dqn():
    from types import SimpleNamespace
    from maleague.league import DistributedLeague, LeagueInstance, league_instance_for
    lg = DistributedLeague(n_players=2, device="cpu", seed=0, player_id=0)
    ff = SimpleNamespace(matchmaking="pfsp", env_args={}, agent_output_type="q", agent="dqn")
    for make in (LeagueInstance, league_instance_for):
        with pytest.raises(NotImplementedError, match="mixtures with agent='dqn'"):
            make(ff, None, lg, experiment=object(), opponents_per_match=2)
    inst = league_instance_for(ff, None, lg, experiment=object())
    assert type(inst) is LeagueInstance and inst.opponents_per_match == 1


def test_agent_vector_of_a_feed_forward_mac():
    """A pool row is the four tensors flat in DQNAgentNetwork.PARAM_ORDER; a load leaves the packed block stale."""
    from maleague.learners.q_learner import FlatParams
    from maleague.modules.agents import DQNAgentNetwork
    from maleague.runs.sp_ma_experiment import agent_vector, load_agent_vector
    from maleague.steppers import SelfPlayFFParallelStepper
    args = _ff_args()
    _, info = _stepper(SelfPlayFFParallelStepper, args)
    _, (src, dst, flat_dst) = _macs(args, info, kinds=("dqn",) * 3)
    FlatParams(flat_dst.agent.parameters(), "cpu")  # as the experiment re-homes the away MAC's parameters
    sd = src.agent.state_dict()
    want = torch.cat([sd[k].reshape(-1) for k in DQNAgentNetwork.PARAM_ORDER])
    vec = agent_vector(src)
    H, A, d_in = args.rnn_hidden_dim, args.n_actions, src.input_shape
    assert vec.numel() == H * d_in + H + A * H + A and torch.equal(vec, want)
    for mac in (dst, flat_dst):
        # what packed() keys its repack on: the dirty counter (writes through a flat view) and the parameter versions
        key0 = (mac.agent._dirty, tuple(p._version for p in mac.agent.parameters()))
        load_agent_vector(mac, vec.clone())
        assert torch.equal(agent_vector(mac), want)
        assert (mac.agent._dirty, tuple(p._version for p in mac.agent.parameters())) != key0
        with pytest.raises(ValueError, match="parameter vector of"):
            load_agent_vector(mac, vec[:-1])


# ---- the oracle condition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", FSP.ORACLE_CASES)
def test_oracle_near_tie_share(cid):
    """The float64 oracle alone sees at most 0.5 % of its greedy picks within Q_TOL (scripts/dqn_selfplay_near_ties.py
    for every case)."""
    _, hidden, plan, la, ai, _, seed, scale = FSP.case(cid)
    picks, ties, draws = FSP.near_ties(plan, hidden, la, ai, seed, scale)
    print(f"{cid}: {ties} near ties of {picks} greedy picks ({draws} epsilon draws)")
    assert picks > 3000 and draws > 0
    assert ties <= 0.005 * picks
