"""The REFIL learner's attention baselines on the CPU: the restatement (tests/refil_baseline_ref.py) pinned to the
reference's golden vectors, the config layers and experiment wiring of algs/attn_qmix and algs/attn_vdn, and the
combinations REFILLearner refuses (no kernel calls)."""
import numpy as np
import pytest
import torch

import refil_baseline_ref as BR
from helpers import entity_scheme_for, refil_args


def _pre(d, prefix):
    return {k[len(prefix):]: torch.from_numpy(np.array(d[k])) for k in d.files if k.startswith(prefix)}


def _scheme():
    """The entity scheme as the learner sees it (EpisodeBatch adds actions_onehot / filled)."""
    from maleague.components.episode_batch import EpisodeBatch
    info = {"n_agents": 8, "n_actions": 21, "n_entities": 16, "entity_shape": 8, "episode_limit": 5}
    scheme, groups, pre = entity_scheme_for(info, torch)
    eb = EpisodeBatch(scheme, groups, 1, 2, preprocess=pre, device="cpu")
    return eb.scheme, eb.groups


@pytest.mark.parametrize("mixer,fixture", [("flex_qmix", "refil_attn_qmix.npz"), ("vdn", "refil_attn_vdn.npz")])
def test_baseline_restatement_two_calls(golden, mixer, fixture):
    """Two reference train calls of entity_attend_rnn + flex_qmix / vdn; tolerances of
    test_refil_oracle.py::test_refil_learner_two_calls. Initial parameters: refil_learner.npz's (the vdn fixture
    repeats the agent's; they must be the same arrays)."""
    d, d0 = golden(fixture), golden("refil_learner.npz")
    a = refil_args(device="cpu", agent="entity_attend_rnn", mixer=mixer)
    batch = {k: v for k, v in _pre(d, "b.").items()}
    for k, v in _pre(d0, "b.").items():
        assert torch.equal(batch[k], v), k
    agent_p, mixer_p = _pre(d0, "p0.agent."), _pre(d0, "p0.mixer.")
    if mixer == "vdn":
        assert not [k for k in d.files if ".mixer." in k]  # VDNMixer.state_dict() is empty
        for k, v in _pre(d, "p0.agent.").items():
            assert torch.equal(v, agent_p[k]), k
    L = BR.REFILBaselineRef(agent_p, mixer_p, a)
    for call in range(2):
        st = L.train(batch, episode_num=call)
        assert set(st) == {k[len(f"c{call}.stat."):] for k in d.files if k.startswith(f"c{call}.stat.")}
        assert "im_loss" not in st
        for k, v in st.items():
            np.testing.assert_allclose(v, float(d[f"c{call}.stat.{k}"]), rtol=1e-4, atol=1e-6, err_msg=f"{call} {k}")
        for k, v in L.agent.items():
            np.testing.assert_allclose(v.detach().numpy(), d[f"c{call}.agent.{k}"], atol=2e-5, rtol=0, err_msg=k)
        for k, v in L.mixer.items():
            np.testing.assert_allclose(v.detach().numpy(), d[f"c{call}.mixer.{k}"], atol=2e-5, rtol=0, err_msg=k)
    assert len(L.mixer) == (0 if mixer == "vdn" else 28)


@pytest.mark.parametrize("alg,mixer,n_params", [("attn_qmix", "flex_qmix", 130645), ("attn_vdn", "vdn", 48853)])
def test_baseline_config_layers_and_experiment_wiring(alg, mixer, n_params):
    """algs/attn_qmix / algs/attn_vdn + envs/ma_entity resolve to the entity stepper, EntityMAC, the plain
    EntityAttentionRNNAgent and REFILLearner; the VDN learner's flat parameters are the agent alone."""
    from maleague.controllers import EntityMAC
    from maleague.custom_logging import MainLogger
    from maleague.learners import REFILLearner
    from maleague.modules.agents import EntityAttentionRNNAgent, ImagineEntityAttentionRNNAgent
    from maleague.modules.mixers import FlexQMixer, VDNMixer
    from maleague.runs import MultiAgentExperiment
    from maleague.steppers import EntityParallelStepper
    from maleague.utils.config import BUILTIN, build_config, to_args
    cfg = build_config(alg, "ma_entity", overrides=["batch_size_run=4", "runner=parallel", "buffer_size=8",
                                                    "buffer_cpu_only=True", "env_args.episode_limit=10"],
                       cuda_available=False)
    a = to_args(cfg)
    assert a.entity_scheme and a.mac == "entity" and a.learner == "refil" and a.mixer == mixer
    assert a.agent == "entity_attend_rnn" and a.name == alg
    base = {k: v for k, v in BUILTIN["algs/refil"].items() if k not in ("agent", "mixer", "name")}
    assert {k: BUILTIN[f"algs/{alg}"][k] for k in base} == base
    exp = MultiAgentExperiment(a, MainLogger(log_interval=10 ** 12))
    assert isinstance(exp.stepper, EntityParallelStepper)
    assert isinstance(exp.home_mac, EntityMAC) and isinstance(exp.home_learner, REFILLearner)
    assert type(exp.home_mac.agent) is EntityAttentionRNNAgent is not ImagineEntityAttentionRNNAgent
    L = exp.home_learner
    assert isinstance(L.mixer, VDNMixer if mixer == "vdn" else FlexQMixer) and type(L.target_mixer) is type(L.mixer)
    n = sum(p.numel() for p in L.parameters())
    assert n == n_params and L._flat.flat.numel() == n and L._tflat.flat.numel() == n
    assert sum(p.numel() for p in exp.home_mac.parameters()) == 48853
    assert len(L.mixer.state_dict()) == (0 if mixer == "vdn" else 32)
    L.update_targets()
    assert torch.equal(L._tflat.flat, L._flat.flat)


@pytest.mark.parametrize("agent,mixer", [("imagine_entity_attend_rnn", "vdn"), ("entity_attend_rnn", "lin_flex_qmix"),
                                         ("imagine_entity_attend_rnn", "lin_flex_qmix"),
                                         ("entity_attend_rnn", "qmix"), ("entity_attend_rnn", None),
                                         ("imagine_entity_attend_rnn", None), ("rnn", "flex_qmix")])
def test_unsupported_combinations_are_refused_by_name(agent, mixer):
    """ValueError naming both keys, at construction (before any launch)."""
    from maleague.controllers import EntityMAC
    from maleague.learners import REFILLearner
    a = refil_args(device="cpu", agent=agent, mixer=mixer)
    scheme, groups = _scheme()
    mac = EntityMAC(scheme, groups, refil_args(device="cpu", agent="entity_attend_rnn"))
    with pytest.raises(ValueError) as e:
        REFILLearner(mac, scheme, None, a)
    assert repr(agent) in str(e.value) and repr(mixer) in str(e.value)


def test_plain_agent_takes_no_groups():
    """train() on the plain agent refuses a groupA (nothing launched: the check precedes the library load)."""
    from maleague.controllers import EntityMAC
    from maleague.learners import REFILLearner
    a = refil_args(device="cpu", agent="entity_attend_rnn", mixer="vdn")
    scheme, groups = _scheme()
    L = REFILLearner(EntityMAC(scheme, groups, a), scheme, None, a)
    L.build_optimizer()
    with pytest.raises(ValueError, match="groupA"):
        L.train(None, 0, 0, groupA=torch.zeros(4, 16, dtype=torch.uint8))
    assert L.last_stats is None and L.train_calls == 0
