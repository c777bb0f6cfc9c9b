"""Host-side checks of the fused learner's mixer cases (no GPU): IQL (no mixer), one-layer hypernets and the QMixer
widths mlg_qlearner_train accepts, the iql config and the "q_learner" registry key, and QLearner's parameter-order
check for a one-layer mixer and for no mixer."""
import os

import pytest
import torch
import yaml

from helpers import qmix_args, scheme_for

N, A, S, H, D_OBS = 5, 15, 60, 64, 80
D_IN = D_OBS + A + N
ES, HES = (16, 32, 64), (32, 64, 128)
CASES = ([pytest.param(0, 2, 32, 64, id="iql")] +
         [pytest.param(2, 1, e, 64, id=f"h1-e{e}") for e in ES] +
         [pytest.param(2, 2, e, he, id=f"h2-e{e}-he{he}") for e in ES for he in HES])


def _cfg(mixer, layers, E, HE, B=4, T=7):
    from maleague import _native
    return _native.MlgLearnerCfg(B=B, T=T, N=N, A=A, d_obs=D_OBS, H=H, S=S, E=E, HE=HE, hypernet_layers=layers,
                                 mixer=mixer, double_q=1, obs_last_action=1, obs_agent_id=1, gamma=0.99, lr=5e-4,
                                 optim_alpha=0.99, optim_eps=1e-5, grad_norm_clip=10.0)


@pytest.mark.parametrize("mixer,layers,E,HE", CASES)
def test_param_counts_and_workspace(mixer, layers, E, HE):
    import ctypes

    from maleague import _native
    from maleague.modules.agents.drqn_agent import DRQNAgentNetwork
    from maleague.modules.mixers import QMixer
    lib = _native.load()
    cfg = _cfg(mixer, layers, E, HE)
    assert lib.mlg_qlearner_workspace_floats(_native.byref(cfg)) > 0, lib.mlg_last_error()
    na, nm = ctypes.c_int64(-1), ctypes.c_int64(-1)
    total = lib.mlg_qlearner_param_counts(_native.byref(cfg), ctypes.byref(na), ctypes.byref(nm))
    args = qmix_args(device="cpu", mixing_embed_dim=E, hypernet_embed=HE, hypernet_layers=layers)
    want_a = sum(p.numel() for p in DRQNAgentNetwork(D_IN, args).parameters())
    want_m = sum(p.numel() for p in QMixer(args).parameters()) if mixer == 2 else 0
    assert (na.value, nm.value) == (want_a, want_m)
    assert total == want_a + want_m
    if mixer == 0:
        assert nm.value == 0


@pytest.mark.parametrize("layers,E,HE,key", [(2, 24, 64, b"mixing_embed_dim"), (1, 24, 64, b"mixing_embed_dim"),
                                             (2, 32, 48, b"hypernet_embed"), (3, 32, 64, b"hypernet_layers")])
def test_refused_shapes_name_the_key(layers, E, HE, key):
    from maleague import _native
    lib = _native.load()
    cfg = _cfg(2, layers, E, HE)
    assert lib.mlg_qlearner_workspace_floats(_native.byref(cfg)) == -1
    assert key in lib.mlg_last_error()
    assert lib.mlg_qlearner_param_counts(_native.byref(cfg), None, None) == -1
    assert key in lib.mlg_last_error()


def test_iql_config_and_registry(tmp_path):
    from maleague import learners
    from maleague.utils.config import build_config
    cfg = build_config("iql", "ma", cuda_available=False)
    assert cfg["mixer"] is None and cfg["learner"] == "q_learner" and cfg["name"] == "iql"
    assert learners.REGISTRY[cfg["learner"]] is learners.QLearner
    assert learners.REGISTRY["q"] is learners.QLearner and learners.REGISTRY["refil"] is learners.REFILLearner
    vdn = build_config("vdn", "ma", cuda_available=False)
    for k, v in vdn.items():  # "the rest as VDN"
        if k not in ("mixer", "learner", "name"):
            assert cfg[k] == v, k
    (tmp_path / "algs").mkdir()
    (tmp_path / "algs" / "iql.yaml").write_text(
        'action_selector: "epsilon_greedy"\nepsilon_start: 1.0\nepsilon_finish: 0.05\nepsilon_anneal_time: 50000\n'
        'runner: "episode"\nbuffer_size: 5000\ntarget_update_interval: 200\nagent_output_type: "q"\n'
        'learner: "q_learner"\ndouble_q: True\nmixer: # Mixer becomes None\n\nname: "iql"')
    assert yaml.safe_load((tmp_path / "algs" / "iql.yaml").read_text())["mixer"] is None
    cfg2 = build_config("iql", "ma", config_dir=str(tmp_path), cuda_available=False)
    assert cfg2["mixer"] is None and cfg2["learner"] == "q_learner"
    assert learners.REGISTRY[cfg2["learner"]] is learners.QLearner


@pytest.mark.parametrize("kw", [{"mixer": "qmix", "hypernet_layers": 1}, {"mixer": None},
                                {"mixer": "qmix", "hypernet_layers": 2}, {"mixer": "vdn"}],
                         ids=["qmix-h1", "iql", "qmix-h2", "vdn"])
def test_check_order_accepts(kw):
    """Constructed on the CPU; train() is not called."""
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    from maleague.learners import QLearner
    from maleague.learners.q_learner import QMIX1_ORDER, QMIX_ORDER
    args = qmix_args(device="cpu", **kw)
    info = {"state_shape": S, "obs_shape": D_OBS, "n_actions": A, "n_agents": N}
    scheme, groups, preprocess = scheme_for(info, torch)
    eb = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device="cpu")
    learner = QLearner(BasicMAC(eb.scheme, groups, args), eb.scheme, None, args, name="home")
    learner._check_order()
    if kw["mixer"] is None:
        assert learner.mixer is None and len(learner.parameters()) == 8
    elif kw["mixer"] == "qmix":
        names = [n for n, _ in learner.mixer.named_parameters()]
        assert names == (QMIX1_ORDER if kw["hypernet_layers"] == 1 else QMIX_ORDER)
        assert len(QMIX1_ORDER) == 10


@pytest.mark.parametrize("name,kw", [("qlearner_qmix_h1.npz", {"hypernet_layers": 1}),
                                     ("qlearner_qmix_e64_he128.npz", {"mixing_embed_dim": 64, "hypernet_embed": 128})])
def test_oracle_reproduces_shape_goldens(golden, name, kw):
    """The CPU oracle on the reference's goldens of the new shapes (tests/golden/make_learner_shapes_golden.py), with
    the bounds test_oracle_golden.py uses for the default shape: the yardstick of the GPU tests covers these shapes."""
    import learner_ref as LR
    from test_oracle_golden import _check_learner
    _check_learner(name, qmix_args(device="cpu", **kw), True, golden, False)
    d = golden(name)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", name)) <= 1 << 20
    assert not any(k.startswith("p1.") for k in d.files), "non-full form"
    assert LR.batch_from_npz(d)["obs"].shape == (4, 7, 5, 80)


def test_oracle_reproduces_the_9v9_h128_golden(golden):
    """The reference's QLearner off the default agent shape (N = 9, A = 23, S = 108, d_obs = 144, H = 128; two files,
    tests/golden/make_learner_shapes_golden.py): the oracle, which the per-arm GPU tests are measured against,
    reproduces it within test_oracle_golden.py's bounds."""
    import learner_arm_shapes as LA
    import learner_ref as LR
    from test_oracle_golden import _check_learner
    d = LA.SplitGolden(golden)
    _check_learner("9v9-h128", qmix_args(device="cpu", **LA.GOLDEN_9V9_KW), True, lambda name: d, False)
    for name in LA.GOLDEN_9V9:
        assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", name)) <= 1 << 20
    assert not any(k.startswith("p1.") for k in d.files), "non-full form"
    assert LR.batch_from_npz(d)["obs"].shape == (4, 7, 9, 144)
    assert LR.batch_from_npz(d)["state"].shape == (4, 7, 108) and d["p0.agent.gru.weight_hh"].shape == (384, 128)
    assert LA.plan_dims("9v9") == (9, 23, 108, 144)
