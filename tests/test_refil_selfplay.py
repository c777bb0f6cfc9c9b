"""CPU: REFIL in self-play (DESIGN.md §3b', §4c'') without a GPU -- the canonical view is an involution, the
two-policy spec, the dispatch of mlg_refil_rollout_selfplay through its host query, the host and Python refusals and the
experiment's stepper choice. tests/test_gpu_refil_selfplay.py runs the kernel against the oracle."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import refil_selfplay_ref as SR
import refil_selfplay_shapes as SS
from helpers import refil_args


# ---- the canonical view -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", ["refil_8", "s5", "s1"])
def test_canonical_view_is_an_involution(cid):
    """Applied twice, the view returns the raw arrays and the raw action indices, along an oracle episode."""
    c = SS.case(cid)
    spec = SS.spec_for(c)
    S, A = spec.S, spec.n_actions
    r = SR.ref_envs_for(spec, 3, c.seed)[2]
    r.reset()
    rng = np.random.RandomState(3)
    assert np.array_equal(SR.view_actions(SR.view_actions(np.arange(A), S), S), np.arange(A))
    assert list(SR.view_actions([0, 1, 2, 3, 4, 5, 5 + S], S)) == [0, 1, 2, 4, 3, 5 + S, 5]
    done, seen_alive = False, False
    while not done:
        ent, om, em = r.entities()
        av = r.avail()
        v = SR.view_entities(ent, om, em, S, spec.grid)
        back = SR.view_entities(*v, S, spec.grid)
        for got, want in zip(back, (ent, om, em)):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        alive = ent[:, 0] == 1
        seen_alive |= bool(alive.any())
        idx = SR.view_index(S)
        # straight from §3b': living entity j' = unit (j' + S) mod U, x mirrored, team flipped, the rest kept
        P = np.float32(SR.pow2(spec.grid))
        for j in range(spec.U):
            u = idx[j]
            if alive[u]:
                x = r.x[u]
                want = [1, np.float32(spec.grid - 1 - x) / P, ent[u, 2], ent[u, 3], 1 - ent[u, 4], ent[u, 5], ent[u, 6],
                        ent[u, 7]]
                assert np.array_equal(v[0][j], np.array(want, np.float32)), (j, u)
            else:
                assert not v[0][j].any()
            assert v[2][j] == em[u]
            assert np.array_equal(v[1][j], om[u][idx])
        assert np.array_equal(SR.view_avail(SR.view_avail(av, S), S), av)
        va = SR.view_avail(av, S)
        assert np.array_equal(va[:, :3], av[:, :3]) and np.array_equal(va[:, 3], av[:, 4])
        for j in range(spec.U):
            assert np.array_equal(va[:, 5 + j], av[:, 5 + idx[j]])
        acts = [int(rng.choice(np.nonzero(row)[0])) for row in av]
        _, done, _ = r.step(acts)
    assert seen_alive


# ---- the spec -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", [c.id for c in SS.SP_CASES])
def test_spec_to_c(cid):
    c = SS.case(cid)
    sp, plain = SS.spec_for(c), SS.spec_for(c, self_play=False)
    S = sp.S
    cs = sp.to_c().base
    assert (cs.n_policy_teams, cs.policy_team, cs.n_agents, cs.U) == (2, 0, 2 * S, 2 * S)
    assert list(cs.scripted) == [0, 0]
    assert [cs.agent_unit[a] for a in range(2 * S)] == list(range(2 * S))
    assert [cs.team[u] for u in range(2 * S)] == [0] * S + [1] * S
    info = sp.env_info()
    assert info["n_agents"] == 2 * S and info["n_entities"] == 2 * S and info["n_actions"] == 5 + 2 * S
    assert sp.n_policy_teams == 2 and plain.n_policy_teams == 1
    # self_play=False: every byte of the C spec is what the default constructor gives, i.e. today's
    from maleague.envs.entity_env import EntityEnvSpec
    today = EntityEnvSpec.from_env_args(SS.env_args(c))
    assert not today.self_play and bytes(plain.to_c()) == bytes(today.to_c())
    p = plain.to_c().base
    assert (p.n_policy_teams, p.n_agents, list(p.scripted)) == (1, S, [0, 1])
    assert plain.env_info()["n_agents"] == S
    # and the two specs differ in exactly those fields
    a, b = plain.to_c(), sp.to_c()
    b.base.n_policy_teams, b.base.n_agents, b.base.scripted[1] = 1, S, 1
    for u in range(S, 2 * S):
        b.base.agent_unit[u] = 0
    assert bytes(a) == bytes(b)


# ---- dispatch -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", [c.id for c in SS.SP_CASES])
def test_dispatch_names(cid):
    from maleague import _native
    c = SS.case(cid)
    spec = SS.spec_for(c)
    name, lds = _native.refil_rollout_selfplay_describe(spec.to_c(), SS.side_dims(spec, c.la))
    assert name == c.arm
    assert 0 < lds <= 160 * 1024


def test_kc3_width_is_not_reachable_from_the_env():
    """Entity input width 33..48 (sp-ro2/kc3) would need more than the env's 8 features + <= 21 actions: dims with
    another entity_shape do not describe a side of the env and are refused."""
    from maleague import _native
    spec = SS.spec_for(SS.case("refil_8"))
    d = SS.side_dims(spec)
    d.entity_shape = 20
    with pytest.raises(_native.NativeError, match="refil_rollout_selfplay: dims .* do not describe one side"):
        _native.refil_rollout_selfplay_describe(spec.to_c(), d)


# ---- host refusals ---------------------------------------------------------------------------------------------------

def _describe_error(spec_c, dims):
    from maleague import _native
    with pytest.raises(_native.NativeError) as exc:
        _native.refil_rollout_selfplay_describe(spec_c, dims)
    return str(exc.value)


def test_host_refuses_a_scripted_spec():
    c = SS.case("s5")
    plain = SS.spec_for(c, self_play=False)
    msg = _describe_error(plain.to_c(), SS.side_dims(plain))
    assert "refil_rollout_selfplay: the spec is not the two-policy entity scenario" in msg
    assert "n_policy_teams=1" in msg and "scripted=[0, 1]" in msg


def test_host_refuses_dims_of_both_sides():
    c = SS.case("s5")
    spec = SS.spec_for(c)
    d = SS.side_dims(spec)
    d.n_agents = 2 * spec.S  # the env's agent count instead of one side's
    # (n_agents = 10 > 8 is caught by the agent dims check under this entry point's name)
    assert "refil_rollout_selfplay: " in _describe_error(spec.to_c(), d)
    c3 = SS.case("s3")
    spec3 = SS.spec_for(c3)
    d3 = SS.side_dims(spec3)
    d3.n_agents = 2 * spec3.S
    assert "refil_rollout_selfplay: dims (n_agents=6 n_entities=6" in _describe_error(spec3.to_c(), d3)
    d3 = SS.side_dims(spec3)
    d3.n_actions += 1
    assert "do not describe one side of the env (S=3, U=6)" in _describe_error(spec3.to_c(), d3)


def _entry_error(spec, dims, home, away, hb=None, ab=None):
    """The entry point itself with host-only arguments: every check below fails before anything is launched."""
    from maleague import _native
    lib = _native.load()
    st = _native.MlgEnvState()
    info = _native.MlgRunInfo()
    hb = hb if hb is not None else _native.MlgEntityBatch()
    ab = ab if ab is not None else _native.MlgEntityBatch()
    rc = lib.mlg_refil_rollout_selfplay(ctypes.byref(spec.to_c()), ctypes.byref(st), ctypes.byref(dims), home, away,
                                        ctypes.byref(hb), ctypes.byref(ab), ctypes.byref(info), 0.0, 0.0, 1, None)
    assert rc != 0
    return lib.mlg_last_error().decode()


def test_host_refuses_unaligned_blocks_and_null_tensors():
    c = SS.case("s5")
    spec = SS.spec_for(c)
    d = SS.side_dims(spec)
    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    assert "refil_rollout_selfplay: null argument" in _entry_error(spec, d, None, base)
    msg = _entry_error(spec, d, base, base + 4)
    assert "refil_rollout_selfplay: the packed weight blocks must be 16-byte aligned" in msg
    assert "16-byte aligned" in _entry_error(spec, d, base + 8, base)
    assert "refil_rollout_selfplay: home batch has null tensors" in _entry_error(spec, d, base, base)
    from maleague import _native
    full = _native.MlgEntityBatch()
    for f, _ in full._fields_:
        if f in ("entities", "obs_mask", "entity_mask", "actions", "avail", "reward", "terminated", "actions_onehot",
                 "filled"):
            setattr(full, f, base)
    assert "refil_rollout_selfplay: away batch has null tensors" in _entry_error(spec, d, base, base, hb=full)


# ---- Python refusals ---------------------------------------------------------------------------------------------------

class _Log:
    test_mode = False

    def log_stat(self, *a):
        pass

    def info(self, *a):
        pass


def _sp_args(cid="s5", B=8, **kw):
    c = SS.case(cid)
    return refil_args(batch_size_run=B, batch_size=B, seed=c.seed, env_args=SS.env_args(c), device="cpu", **kw)


def _stepper(cid="s5", **kw):
    from maleague.steppers import SELF_ENTITY_REGISTRY
    return SELF_ENTITY_REGISTRY["parallel"](_sp_args(cid, **kw), _Log())


def test_registry_and_exports():
    import maleague.steppers as st
    assert st.SELF_ENTITY_REGISTRY == {"episode": st.SelfPlayEntityStepper, "parallel": st.SelfPlayEntityParallelStepper}
    for n in ("SelfPlayEntityParallelStepper", "SelfPlayEntityStepper", "SELF_ENTITY_REGISTRY"):
        assert n in st.__all__
    assert issubclass(st.SelfPlayEntityStepper, st.SelfPlayEntityParallelStepper)


def test_stepper_spec_is_the_two_policy_env():
    s = _stepper()
    assert s.spec.self_play and s.get_env_info()["n_agents"] == 10 and s._cspec.base.n_policy_teams == 2
    assert "entities" in s._batch_keys and "obs" not in s._batch_keys


def test_stepper_refuses_a_non_entity_side():
    import torch
    from helpers import entity_scheme_for
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC, EntityMAC
    s = _stepper()
    args = _sp_args(n_agents=5, n_entities=10, n_actions=15)
    scheme, groups, pre = entity_scheme_for(SR.side_info(s.spec), torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=pre, device="cpu")
    mac = EntityMAC(proto.scheme, groups, args)

    class NotEntity(BasicMAC):
        def __init__(self):
            pass

    with pytest.raises(NotImplementedError, match="SelfPlayEntityParallelStepper drives two EntityMACs .* the away MAC "
                                                  "is a NotEntity"):
        s.initialize(scheme, groups, pre, mac, NotEntity())
    with pytest.raises(NotImplementedError, match="the home MAC is a NotEntity"):
        s.initialize(scheme, groups, pre, NotEntity(), mac)
    with pytest.raises(ValueError, match="needs an away MAC"):
        s.initialize(scheme, groups, pre, mac)
    other = EntityMAC(proto.scheme, groups, _sp_args(n_agents=5, n_entities=10, n_actions=15, entity_last_action=False))
    with pytest.raises(ValueError, match="same architecture"):
        s.initialize(scheme, groups, pre, mac, other)
    s.initialize(scheme, groups, pre, mac, EntityMAC(proto.scheme, groups, args))
    assert s.describe_rollout()[0] == "sp-ro2/kc2"


def test_stepper_refuses_mixtures_and_two_roster_plans():
    from maleague.envs.plans import team_from_codes
    from maleague.steppers import OpponentMix
    s = _stepper()
    s.set_opponent_mix(None)
    with pytest.raises(NotImplementedError, match="SelfPlayEntityParallelStepper.set_opponent_mix: opponent mixtures "
                                                  "over entity agents are not supported"):
        s.set_opponent_mix(OpponentMix(rows=None, group_opponent=[0]))
    codes = SS.case("s5").codes
    other = " ".join(reversed(codes.split()))
    assert other != codes
    with pytest.raises(NotImplementedError, match="set_match_build_plan: the plan's two teams differ"):
        s.set_match_build_plan([team_from_codes(codes, False), team_from_codes(other, False)])
    s.set_match_build_plan([team_from_codes(other, False), team_from_codes(other, False)])  # one roster: accepted
    assert s.spec.self_play and s._cspec.base.n_policy_teams == 2
    assert [s._cspec.base.role[u] for u in range(5)] == [s._cspec.base.role[u + 5] for u in range(5)]


def test_league_layers_refuse_entity_scheme_by_name():
    from maleague.league.evaluation import CrossPlayEvaluator, evaluator_for
    from maleague.league.instance import LeagueInstance, league_instance_for
    args = _sp_args()
    for fn, who in ((lambda: league_instance_for(args, _Log(), None), "league_instance_for"),
                    (lambda: LeagueInstance(args, _Log(), None), "LeagueInstance"),
                    (lambda: evaluator_for(args, "cpu"), "evaluator_for"),
                    (lambda: CrossPlayEvaluator(args, "cpu"), "CrossPlayEvaluator")):
        with pytest.raises(NotImplementedError) as exc:
            fn()
        msg = str(exc.value)
        assert msg.startswith(who + ": entity_scheme"), msg
        assert "SelfPlayEntityParallelStepper" in msg and "SelfPlayEntityStepper" in msg, msg
    from maleague.exceptions import refuse_entity_league
    refuse_entity_league(SimpleNamespace(entity_scheme=False), "x")
    with pytest.raises(NotImplementedError, match="league/main.py: entity_scheme"):
        refuse_entity_league(args, "league/main.py")


def test_league_main_refuses_entity_scheme():
    """league/main.py with the refil config: refused by name before any league object is built."""
    import inspect
    from maleague.league import main as LM
    src = inspect.getsource(LM.main)
    assert src.index('refuse_entity_league(args, "league/main.py")') < src.index("DistributedLeague(")


# ---- the experiment ------------------------------------------------------------------------------------------------------

def test_experiment_builds_the_entity_stepper_and_keeps_the_entity_keys():
    from maleague.runs.sp_ma_experiment import SelfPlayMultiAgentExperiment
    from maleague.steppers import SelfPlayEntityParallelStepper, SelfPlayEntityStepper, SelfPlayParallelStepper
    exp = SelfPlayMultiAgentExperiment.__new__(SelfPlayMultiAgentExperiment)
    exp.args, exp.logger = _sp_args(), _Log()
    st = exp._build_stepper()
    assert type(st) is SelfPlayEntityParallelStepper
    exp.stepper, exp.env_info = st, st.get_env_info()
    scheme = exp._integrate_env_info()
    assert scheme["n_agents"] == 5 and scheme["total_n_agents"] == 10
    assert scheme["n_entities"] == 10 and scheme["entity_shape"] == 8
    assert (exp.args.n_agents, exp.args.n_entities, exp.args.entity_shape, exp.args.n_actions) == (5, 10, 8, 15)
    exp.args = _sp_args(B=1)
    exp.args.runner = "episode"
    assert type(exp._build_stepper()) is SelfPlayEntityStepper
    from maleague.steppers import SELF_REGISTRY
    assert SELF_REGISTRY["parallel"] is SelfPlayParallelStepper  # the other registries are untouched


def test_agent_vector_roundtrip_for_an_entity_mac():
    import torch
    from helpers import entity_scheme_for
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import EntityMAC
    from maleague.runs.sp_ma_experiment import agent_vector, load_agent_vector
    args = _sp_args(n_agents=5, n_entities=10, n_actions=15)
    scheme, groups, pre = entity_scheme_for({"n_entities": 10, "entity_shape": 8, "n_actions": 15, "n_agents": 5}, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=pre, device="cpu")
    torch.manual_seed(1)
    a, b = EntityMAC(proto.scheme, groups, args), EntityMAC(proto.scheme, groups, args)
    v = agent_vector(a).clone()
    assert v.numel() == sum(p.numel() for p in a.agent.parameters())
    assert not torch.equal(v, agent_vector(b))
    dirty = b.agent._dirty
    load_agent_vector(b, v)
    assert torch.equal(agent_vector(b), v)
    assert b.agent._dirty > dirty or all(p._version > 0 for p in b.agent.parameters())  # the packed copy is refreshed
    with pytest.raises(ValueError, match="parameter vector"):
        load_agent_vector(b, v[:-1])
