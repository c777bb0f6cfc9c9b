"""CPU checks of distinct per-agent networks (mac: distinct): the registry, the refusals, parameters(), the dispatch
table of mlg_rollout_distinct through the host-only mlg_rollout_distinct_describe, checkpoint file names, and the
oracle of the GPU tests (tests/distinct_ref.py) pinned to the reference's own DistinctMAC.forward at batch_size 1
(tests/golden/make_distinct_golden.py)."""
import os

import numpy as np
import pytest
import torch

import distinct_ref as DR
import distinct_shapes as DS
from helpers import qmix_args, scheme_for

N, A, D_OBS, S, H = 3, 11, 48, 36, 32


def _mac(**kw):
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import REGISTRY
    a = dict(n_agents=N, n_actions=A, state_shape=S, rnn_hidden_dim=H, obs_agent_id=False, mac="distinct",
             device="cpu")
    a.update(kw)
    args = qmix_args(**a)
    info = {"state_shape": S, "obs_shape": D_OBS, "n_actions": A, "n_agents": args.n_agents}
    scheme, groups, preprocess = scheme_for(info, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device="cpu")
    return REGISTRY["distinct"](proto.scheme, groups, args), args, (scheme, groups, preprocess)


def _golden_params(g):
    return [{k: torch.from_numpy(g[f"p{i}.{k}"]) for k in DR.AGENT_KEYS} for i in range(N)]


def test_registry_key():
    from maleague.controllers import REGISTRY, BasicMAC, DistinctMAC
    assert REGISTRY["distinct"] is DistinctMAC and issubclass(DistinctMAC, BasicMAC)
    mac, _, _ = _mac()
    assert isinstance(mac.agents, torch.nn.ModuleList) and len(mac.agents) == N and not hasattr(mac, "agent")


def test_agent_id_refused_with_the_reference_message():
    with pytest.raises(NotImplementedError, match="Please deactivate agent id observation for distinct agents networks"):
        _mac(obs_agent_id=True)


def test_other_agents_and_pi_logits_refused_by_name():
    with pytest.raises(NotImplementedError, match="mac='distinct'.*agent='dqn'"):
        _mac(agent="dqn")
    with pytest.raises(NotImplementedError, match="mac='distinct'.*pi_logits"):
        _mac(agent_output_type="pi_logits")


def test_parameters_lists_every_network_in_order():
    mac, _, _ = _mac()
    params = mac.parameters()
    assert len(params) == N * 8
    for i, agent in enumerate(mac.agents):
        named = list(agent.named_parameters())
        assert [k for k, _ in named] == DR.AGENT_KEYS
        for j, (_, p) in enumerate(named):
            assert params[i * 8 + j] is p
    assert mac.agents[0].fc1.weight.data_ptr() != mac.agents[1].fc1.weight.data_ptr()


def test_load_state_and_trained_steps():
    mac, _, _ = _mac()
    other, _, _ = _mac()
    assert not torch.equal(mac.agents[1].fc1.weight, other.agents[1].fc1.weight)
    mac.load_state(other)
    for a, b in zip(mac.agents, other.agents):
        for (k, v), (_, w) in zip(a.state_dict().items(), b.state_dict().items()):
            assert torch.equal(v, w), k
    mac.update_trained_steps(7)
    mac.update_trained_steps(5)  # sets, as the reference does; BasicMAC's adds
    assert [a.trained_steps for a in mac.agents] == [5] * N
    mac.init_hidden(4)
    assert tuple(mac.hidden_states.shape) == (4, N, H)


class _Log:
    test_mode = False

    def info(self, *_a, **_k):
        pass

    def log_stat(self, *_a, **_k):
        pass


def test_paths_that_hold_mac_agent_refuse_by_name():
    from maleague.learners import COMALearner
    from maleague.league.evaluation import CrossPlayEvaluator
    from maleague.league.instance import LeagueInstance
    from maleague.steppers import SelfPlayParallelStepper, SelfPlayStepper
    from helpers import sp_args
    mac, args, (scheme, groups, preprocess) = _mac()
    pat = "mac='distinct'"
    with pytest.raises(NotImplementedError, match=pat):
        COMALearner(mac, None, _Log(), args)
    with pytest.raises(NotImplementedError, match=pat):
        CrossPlayEvaluator(args, "cpu")
    with pytest.raises(NotImplementedError, match=pat):
        LeagueInstance(args, _Log(), league=None)
    for cls, B in ((SelfPlayParallelStepper, 2), (SelfPlayStepper, 1)):
        sa = sp_args(B, 10, 1, plan="small", device="cpu")
        stepper = cls(sa, _Log())
        for home, away in ((mac, mac), (object(), mac)):
            with pytest.raises(NotImplementedError, match=pat):
                stepper.initialize(scheme, groups, preprocess, home, away)


def test_describe_table():
    from maleague import _native
    for cid, hidden, plan, la, arm, seed, _ in DS.CASES:
        spec = DS.spec_of(plan, seed)
        name, lds = _native.rollout_distinct_describe(spec.to_c(), DS.dims_of(spec, hidden, la))
        assert name == arm, cid
        assert 0 < lds <= 64 * 1024
    for (n_pol, n_scr), arm in DS.DESCRIBE:
        spec = DS.spec_of(DS.plan_of(n_pol, n_scr))
        assert spec.n_agents == n_pol
        if arm is None:
            with pytest.raises(_native.NativeError, match=r"33 agent tiles"):
                _native.rollout_distinct_describe(spec.to_c(), DS.dims_of(spec, 64))
        else:
            assert _native.rollout_distinct_describe(spec.to_c(), DS.dims_of(spec, 64))[0] == arm


def test_c_entry_points_refuse_agent_id():
    """dims.obs_agent_id = 1 fails the dims check of all three entry points before any pointer is read or anything
    is launched (no GPU needed)."""
    import ctypes
    from maleague import _native
    lib = _native.load()
    spec = DS.spec_of("small")
    d = DS.dims_of(spec, 64, agent_id=True)
    with pytest.raises(_native.NativeError, match="obs_agent_id must be 0"):
        _native.rollout_distinct_describe(spec.to_c(), d)
    st = _native.MlgEnvState(1, 1, 1, 1, 1, 4)  # never dereferenced: the dims are checked first
    cs = spec.to_c()
    rc = lib.mlg_rollout_distinct(ctypes.byref(cs), ctypes.byref(st), ctypes.byref(d), None, None, None, 0.0, 1, None)
    assert rc != 0 and "obs_agent_id must be 0" in lib.mlg_last_error().decode()
    rc = lib.mlg_mac_forward_distinct(ctypes.byref(d), None, None, 0, None, None, None, None)
    assert rc != 0 and "obs_agent_id must be 0" in lib.mlg_last_error().decode()


def test_oracle_matches_reference_golden(golden):
    """distinct_ref.mac_unroll against the reference's DistinctMAC.forward at batch_size 1 within 1e-6."""
    g = golden("distinct.npz")
    ps = _golden_params(g)
    tb = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("b.")}
    with torch.no_grad():
        q, h = DR.mac_unroll(ps, tb)
    want = np.transpose(g["q"], (1, 0, 2, 3))  # [T, B, N, A] -> [B, T, N, A]
    assert q.shape == want.shape == (1, 4, N, A)
    np.testing.assert_allclose(q.numpy(), want, rtol=0, atol=1e-6)
    np.testing.assert_allclose(h.numpy(), np.transpose(g["h"], (1, 0, 2)), rtol=0, atol=1e-6)
    # the networks differ: agent i's row is not what another network gives
    assert np.abs(want[0, :, 0] - want[0, :, 1]).max() > 1e-3


def test_checkpoint_names_and_golden_state_dicts(tmp_path, golden):
    """save_models writes {name}agent_{i}.th (the reference's names, one state dict per file, the reference's keys);
    files holding the golden's state dicts load, network by network."""
    g = golden("distinct.npz")
    mac, _, _ = _mac()
    mac.save_models(str(tmp_path), "home_")
    assert sorted(os.listdir(tmp_path)) == list(g["ckpt_names"]) == [f"home_agent_{i}.th" for i in range(N)]
    for i in range(N):
        sd = torch.load(os.path.join(str(tmp_path), f"home_agent_{i}.th"), weights_only=True)
        assert list(sd) == list(g["ckpt_keys"]) == DR.AGENT_KEYS
        assert all(torch.equal(v, mac.agents[i].state_dict()[k]) for k, v in sd.items())
    other, _, _ = _mac()
    other.load_models(str(tmp_path), "home_")
    for a, b in zip(mac.agents, other.agents):
        assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    ref_dir = tmp_path / "ref"
    ref_dir.mkdir()
    for i, p in enumerate(_golden_params(g)):  # the reference's files: torch.save of each network's state dict
        torch.save(p, str(ref_dir / f"home_agent_{i}.th"))
    other.load_models(str(ref_dir), "home_")
    for i, a in enumerate(other.agents):
        for k, v in a.state_dict().items():
            assert np.array_equal(v.numpy(), g[f"p{i}.{k}"]), (i, k)
