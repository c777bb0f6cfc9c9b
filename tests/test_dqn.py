"""The feed-forward agent (agent: dqn) on the host: registry and module surface, the oracle tests/dqn_ref.py pinned to
the reference's goldens (tests/golden/make_dqn_golden.py), the dispatch table of mlg_rollout_ff through the host-only
query, and the refusals of the paths that do not run a feed-forward agent. No GPU needed.
"""
import os

import numpy as np
import pytest
import torch

import dqn_ref
import dqn_shapes as DS
import learner_ref
from helpers import drqn_dims, qmix_args, scheme_for, shape_plan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LDS_LIMIT = 160 * 1024


def _mac(device="cpu", **kw):
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    args = qmix_args(agent="dqn", device=device, **kw)
    info = {"state_shape": args.state_shape, "obs_shape": 80, "n_actions": args.n_actions, "n_agents": args.n_agents}
    scheme, groups, preprocess = scheme_for(info, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    return BasicMAC(proto.scheme, groups, args), args


# ---- 1. registry and module ---------------------------------------------------------------------------------------

def test_registry_and_module_surface():
    """Fails on the parent commit with a KeyError: 'dqn' was not registered."""
    from maleague.modules.agents import REGISTRY, DQNAgentNetwork
    assert REGISTRY["dqn"] is DQNAgentNetwork
    mac, args = _mac()
    agent = mac.agent
    assert isinstance(agent, DQNAgentNetwork)
    shapes = {k: tuple(v.shape) for k, v in agent.state_dict().items()}
    assert shapes == {"fc1.weight": (64, 100), "fc1.bias": (64,), "fc2.weight": (15, 64), "fc2.bias": (15,)}
    assert list(shapes) == [n for n, _ in agent.named_parameters()] == list(DQNAgentNetwork.PARAM_ORDER)
    d = agent.dims()
    assert (d.d_obs, d.n_actions, d.n_agents, d.hidden, d.d_in, d.obs_last_action, d.obs_agent_id) == \
        (80, 15, 5, 64, 100, 1, 1)
    for name in ("packed", "mark_dirty", "enable_autograd", "wants_grad", "_live_params"):
        assert callable(getattr(agent, name)), name
    # init_hidden: one cached zero [1, 1] tensor, expanded without a fill (the reference's shape cannot be expanded)
    h0 = agent.init_hidden()
    assert tuple(h0.shape) == (1, 1) and not h0.any() and agent.init_hidden() is h0
    mac.init_hidden(7)
    assert tuple(mac.hidden_states.shape) == (7, 5, 1)
    assert mac.hidden_states.untyped_storage().data_ptr() == h0.untyped_storage().data_ptr()


def test_reference_checkpoint_loads_and_marks_dirty():
    mac, args = _mac()
    before = mac.agent._dirty
    mac.load_models(os.path.join(GOLDEN, "ckpt_dqn", "100"), "home_")
    assert mac.agent._dirty > before
    g = np.load(os.path.join(GOLDEN, "dqn_mac_forward.npz"))
    for k, v in mac.agent.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), g[f"p.{k}"])


def test_wants_grad_routing():
    mac, args = _mac()
    x = torch.zeros(5, 100)
    assert not mac.agent.wants_grad(x)
    mac.enable_autograd()
    assert mac.agent.wants_grad(x)
    with torch.no_grad():
        assert not mac.agent.wants_grad(x)
    for p in mac.agent.parameters():
        p.requires_grad = False
    assert not mac.agent.wants_grad(x) and mac.agent.wants_grad(x.requires_grad_())


# ---- 2. the oracle, pinned to the reference ---------------------------------------------------------------------
# bounds: those tests/test_oracle_golden.py holds oracle/learner_ref.py to for the DRQN forward fixtures

def test_oracle_forward_matches_reference(golden):
    g = golden("dqn_forward.npz")
    p = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("p.")}
    assert list(p) == dqn_ref.AGENT_KEYS
    q = dqn_ref.dqn_forward(p, torch.from_numpy(g["inputs"]))
    np.testing.assert_allclose(q.numpy(), g["q"], rtol=1e-5, atol=1e-6)
    q64 = dqn_ref.dqn_forward({k: v.double() for k, v in p.items()}, torch.from_numpy(g["inputs"]).double())
    np.testing.assert_allclose(q64.numpy(), g["q"], rtol=1e-5, atol=1e-5)


def test_oracle_mac_unroll_matches_reference(golden):
    g = golden("dqn_mac_forward.npz")
    p = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("p.")}
    batch = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("b.")}
    q = dqn_ref.mac_unroll(p, batch, 5)  # [B, T, N, A]
    ref = np.transpose(g["q"], (1, 0, 2, 3))
    np.testing.assert_allclose(q.numpy(), ref, rtol=1e-5, atol=1e-6)


def test_oracle_is_pinned_to_the_reference_goldens(golden):
    """tests/dqn_ref.DQNLearnerRef against the two goldens on the CPU, with the bounds tests/test_oracle_golden.py holds
    oracle/learner_ref.py to for the DRQN fixtures (statistics rtol 1e-4 / atol 1e-6, parameters atol 2e-5)."""
    for tag, kw in (("dqn_qmix", {}), ("dqn_vdn", {"mixer": "vdn"})):
        d = golden(f"qlearner_{tag}.npz")
        args = qmix_args(agent="dqn", device="cpu", **kw)
        agent0 = {k[len("p0.agent."):]: np.array(d[k]) for k in d.files if k.startswith("p0.agent.")}
        mixer0 = {k[len("p0.mixer."):]: np.array(d[k]) for k in d.files if k.startswith("p0.mixer.")} or None
        ref = dqn_ref.DQNLearnerRef(agent0, mixer0, args)
        tb = learner_ref.batch_from_npz(d)
        for i, (t_env, ep) in enumerate(d["calls"]):
            got = ref.train({k: v.clone() for k, v in tb.items()}, int(t_env), int(ep))
            for k in ("loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean"):
                np.testing.assert_allclose(got[k], float(d[f"stat{i}.{k}"]), rtol=1e-4, atol=1e-6, err_msg=f"{tag} {i} {k}")
        last = len(d["calls"])
        for k, v in ref.agent_state().items():
            np.testing.assert_allclose(v.numpy(), d[f"p{last}.agent.{k}"], atol=2e-5, rtol=0, err_msg=f"{tag} {k}")
        assert ref.trained_steps == int(d["trained_steps"])



# ---- 3. dispatch, host only -------------------------------------------------------------------------------------

def describe(plan, hidden):
    from maleague import _native
    from maleague.envs.teams_env import TeamsEnvSpec
    spec = TeamsEnvSpec.from_env_args({"match_build_plan": shape_plan(plan), "grid_size": 20,
                                       "stochastic_spawns": True, "episode_limit": DS.EPISODE_LIMIT})
    return _native.rollout_ff_describe(spec.to_c(), drqn_dims(spec, hidden))


@pytest.mark.parametrize("cid,hidden,plan,arm,seed,scale", DS.CASES, ids=[c[0] for c in DS.CASES])
def test_rollout_ff_case_arm(cid, hidden, plan, arm, seed, scale):
    name, lds = describe(plan, hidden)
    assert name == arm
    assert 0 < lds <= LDS_LIMIT


def test_cases_cover_every_reachable_arm():
    """H 32 / 64 / 128, K = 1..4 and both arms appear; every arm a symmetric plan (K = 1..32), `large` or an asymmetric
    plan reaches has a case. ff-global/tpw1 is reached by none (dqn_shapes.py says why)."""
    arms = {c[3] for c in DS.CASES}
    assert {c[1] for c in DS.CASES} == {32, 64, 128}
    assert {a.split("/")[0] for a in arms} == {"ff-lds", "ff-global"}
    assert {a[-1] for a in arms if a.startswith("ff-lds")} == {"1", "2", "3", "4"}
    assert {a[-1] for a in arms if a.startswith("ff-global")} == {"2", "3", "4"}
    assert set(DS.RING_CASES) <= {c[0] for c in DS.CASES}
    assert {DS.case(c)[3][-1] for c in DS.RING_CASES} == {"1", "2", "3", "4"}
    plans = [f"{k}v{k}" for k in range(1, 33)] + ["large", "5v7", "3v5", "medium_1h_4t", "small"]
    for hidden in (32, 64, 128):
        for plan in plans:
            name, lds = describe(plan, hidden)
            assert name in arms, (plan, hidden, name)
            assert 0 < lds <= LDS_LIMIT


def test_lds_image_has_no_gru_blocks():
    """5v5 at H = 64: the feed-forward launch needs 37344 B (weights in LDS), the DRQN's generic kernel 138 KiB."""
    from maleague import _native
    from maleague.envs.teams_env import TeamsEnvSpec
    assert describe("medium_1h_4t", 64) == ("ff-lds/tpw1", 37344)
    spec = TeamsEnvSpec.from_env_args({"match_build_plan": "medium_1h_4t"})
    d = drqn_dims(spec, 64)
    n_ff = _native.load().mlg_ff_packed_size(_native.byref(d))
    # w1d [64][112] + w1o [64][80] + w1a [15][64] + w1n [5][64] + b1 + w2 [16][64] + b2 [16]
    assert n_ff == 64 * 112 + 64 * 80 + 15 * 64 + 5 * 64 + 64 + 16 * 64 + 16
    assert n_ff < _native.load().mlg_packed_agent_size(_native.byref(d))


def test_rollout_ff_refusals():
    from maleague import _native
    from maleague.envs.teams_env import TeamsEnvSpec
    spec = TeamsEnvSpec.from_env_args({"match_build_plan": "small"})
    for hidden in (16, 48, 96, 256):
        with pytest.raises(_native.NativeError, match=f"rnn_hidden_dim={hidden} unsupported"):
            _native.rollout_ff_describe(spec.to_c(), drqn_dims(spec, hidden))
        d = drqn_dims(spec, hidden)
        assert _native.load().mlg_ff_packed_size(_native.byref(d)) == -1
        assert f"rnn_hidden_dim={hidden}" in _native.load().mlg_last_error().decode()
    with pytest.raises(_native.NativeError, match="rollout_ff: agent dims do not match env spec"):
        _native.rollout_ff_describe(spec.to_c(), drqn_dims(spec, 64, self_play=True))
    # more than four tiles per wave: 16 x 33 rows = 33 tiles on 8 waves (33 agents against 31 scripted units)
    from maleague.envs.plans import team_from_codes
    codes = lambda k: " ".join(("TR", "AR", "HR", "TM")[i % 4] for i in range(k))  # noqa: E731
    big = TeamsEnvSpec.from_env_args({"match_build_plan": [team_from_codes(codes(31), True),
                                                           team_from_codes(codes(33), False)]})
    with pytest.raises(_native.NativeError, match="rollout_ff: 5 agent tiles per wave > 4"):
        _native.rollout_ff_describe(big.to_c(), drqn_dims(big, 64))
    assert describe("32v32", 64)[0] == "ff-global/tpw4"  # the largest symmetric plan


# ---- 4. refusals of the paths that run the recurrent agent only ---------------------------------------------------

def test_policy_rollout_refuses_dqn():
    from maleague.custom_logging import MainLogger
    from maleague.steppers import ParallelStepper
    args = qmix_args(agent="dqn", device="cpu", agent_output_type="pi_logits", action_selector="multinomial",
                     mask_before_softmax=True, test_greedy=True, batch_size_run=2)
    stepper = ParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"], info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(info, torch)
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device="cpu")
    mac = BasicMAC(proto.scheme, groups, args)
    stepper.initialize(scheme, groups, preprocess, mac)
    with pytest.raises(NotImplementedError, match="agent='dqn'"):
        stepper.describe_rollout()
    with pytest.raises(NotImplementedError, match="agent='dqn'"):
        stepper._rollout(None, None, 0.0, True)


def test_coma_learner_refuses_dqn():
    from maleague.custom_logging import MainLogger
    from maleague.learners.coma_learner import COMALearner
    mac, args = _mac(agent_output_type="pi_logits", action_selector="multinomial", mask_before_softmax=True,
                     critic_train_mode="seq", q_nstep=0)
    with pytest.raises(NotImplementedError, match="agent='dqn'"):
        COMALearner(mac, None, MainLogger(), args)


# ---- the fused learner's dispatch with agent = 1, host only ---------------------------------------------------------

@pytest.mark.parametrize("cid", DS.LEARNER_IDS)
def test_qlearner_describe_and_param_counts_with_agent_1(cid):
    import ctypes
    import learner_arm_shapes as LA
    from maleague import _native
    c = DS.learner_case(cid)
    cfg = DS.learner_cfg(c)
    assert _native.qlearner_describe(cfg) == c.arm
    N, A, S, d_obs = LA.dims(c)
    H, d_in = c.H, d_obs + A + N
    na, nm = ctypes.c_int64(0), ctypes.c_int64(0)
    total = _native.load().mlg_qlearner_param_counts(_native.byref(cfg), ctypes.byref(na), ctypes.byref(nm))
    assert na.value == d_in * H + H + A * H + A
    cfg0 = LA.learner_cfg(LA.case_args(c, "cpu"), d_obs)  # the same shape with the DRQN agent: the mixer part agrees
    na0, nm0 = ctypes.c_int64(0), ctypes.c_int64(0)
    _native.load().mlg_qlearner_param_counts(_native.byref(cfg0), ctypes.byref(na0), ctypes.byref(nm0))
    assert cfg0.agent == 0 and nm.value == nm0.value and total == na.value + nm.value
    assert na0.value == na.value + 6 * H * H + 6 * H
    assert _native.qlearner_describe(cfg0).startswith(f"h{H}/")
    # no GRU buffers in the feed-forward workspace
    ws, ws0 = (_native.load().mlg_qlearner_workspace_floats(_native.byref(x)) for x in (cfg, cfg0))
    assert 0 < ws < ws0


def test_qlearner_cases_cover_the_ranges():
    cases = [DS.learner_case(c) for c in DS.LEARNER_IDS]
    import learner_arm_shapes as LA
    assert {c.H for c in cases} == {32, 64, 128}
    assert {1, 5, 17} <= {LA.dims(c)[0] for c in cases}
    parts = {c.arm.split(" + ")[1] for c in cases}
    assert {"iql", "vdn-fast", "vdn", "qmix-generic", "qmix1-e32", "qmix-he32-e16"} <= parts


def test_qlearner_refuses_an_unknown_agent_value():
    from maleague import _native
    cfg = DS.learner_cfg(DS.learner_case("ff-qmix-h64-5v5"))
    cfg.agent = 2
    with pytest.raises(_native.NativeError, match="agent=2 unsupported"):
        _native.qlearner_describe(cfg)
    assert _native.load().mlg_qlearner_workspace_floats(_native.byref(cfg)) == -1


def test_qlearner_check_order_uses_the_agents_own_order():
    from maleague.custom_logging import MainLogger
    from maleague.learners.q_learner import QLearner
    mac, args = _mac()
    learner = QLearner(mac, None, MainLogger(), args)
    learner._check_order()
    assert learner._cfg(4, 7).agent == 1


def test_selfplay_and_crossplay_refuse_dqn():
    from maleague.custom_logging import MainLogger
    from maleague.envs.plans import builtin_plan
    from maleague.league.evaluation import CrossPlayEvaluator
    from maleague.steppers import SelfPlayParallelStepper
    args = qmix_args(agent="dqn", device="cpu", batch_size_run=2,
                     env_args={"match_build_plan": builtin_plan("small", self_play=True), "grid_size": 20,
                               "stochastic_spawns": True, "episode_limit": 5})
    stepper = SelfPlayParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for({**info, "n_agents": args.n_agents}, torch)
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device="cpu")
    home, away = BasicMAC(proto.scheme, groups, args), BasicMAC(proto.scheme, groups, args)
    with pytest.raises(NotImplementedError, match="agent='dqn'"):
        stepper.initialize(scheme, groups, preprocess, home, away)
    with pytest.raises(NotImplementedError, match="agent='dqn'"):
        CrossPlayEvaluator(args, "cpu")
    # every other non-DRQN agent is refused on both paths as well, by the same messages
    from types import SimpleNamespace
    args.agent = "entity_attend_rnn"
    with pytest.raises(NotImplementedError, match="agent='entity_attend_rnn' is not supported .agent='dqn'"):
        CrossPlayEvaluator(args, "cpu")
    other = SimpleNamespace(agent_output_type="q", agent=torch.nn.Linear(2, 2))
    with pytest.raises(NotImplementedError, match="the away MAC's Linear is not supported .agent='dqn'"):
        stepper.initialize(scheme, groups, preprocess, _rnn_mac(proto, groups, args), other)
    # the recurrent agent is taken as before
    args.agent = "rnn"
    CrossPlayEvaluator(args, "cpu")
    stepper.initialize(scheme, groups, preprocess, _rnn_mac(proto, groups, args), _rnn_mac(proto, groups, args))


def _rnn_mac(proto, groups, args):
    from maleague.controllers import BasicMAC
    saved, args.agent = args.agent, "rnn"
    try:
        return BasicMAC(proto.scheme, groups, args)
    finally:
        args.agent = saved
