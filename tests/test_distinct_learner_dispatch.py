"""The fused learner with distinct per-agent networks (MlgLearnerCfg.distinct = 1) through its host-only queries, no
GPU needed: parameter counts, workspace sizes, the dx- names mlg_qlearner_describe reports (the launches follow the same
host function), the refusals, and that distinct = 0 keeps every name tests/test_learner_dispatch.py pins.

The last test checks the cases of tests/distinct_learner_shapes.py against the oracles alone: over the three calls the
fp32 and the float64 oracle (tests/distinct_ref.py), each on its own trajectory, pick the same action at every live
(b, t, n) -- the double-Q argmax of the online Q at t + 1, or where double_q is off the argmax behind the masked max of
the target Q. A disagreement there would be a seed at which the GPU tests compare across a flipped pick; the cap is 0.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import distinct_learner_shapes as DLS
import distinct_ref as DR
import learner_arm_shapes as LA
from helpers import qmix_args

NAME = re.compile(r"^dx-h(32|64|128)/bwd-split/q([1-6]) \+ "
                  r"(iql|vdn-fast|vdn|qmix-generic|qmix1-e(16|32|64)|qmix-he(32|64|128)-e(16|32|64))$")
MIXERS = {"qmix": {}, "vdn": {"mixer": "vdn"}, "iql": {"mixer": None}}


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    for k in ("MLG_MIX_GENERIC", "MLG_LEARNER_FULL"):
        monkeypatch.delenv(k, raising=False)


def _cfg(N=5, A=15, S=60, d_obs=80, H=64, distinct=1, B=LA.B, T=LA.T_FILLED, **kw):
    kw.setdefault("obs_agent_id", False)
    args = qmix_args(n_agents=N, n_actions=A, state_shape=S, rnn_hidden_dim=H, device="cpu", **kw)
    cfg = LA.learner_cfg(args, d_obs, B=B, T=T)
    cfg.distinct = distinct
    return cfg


def _counts(cfg):
    from maleague import _native
    lib = _native.load()
    na, nm = ctypes.c_int64(-1), ctypes.c_int64(-1)
    total = lib.mlg_qlearner_param_counts(_native.byref(cfg), ctypes.byref(na), ctypes.byref(nm))
    assert total >= 0, lib.mlg_last_error()
    return na.value, nm.value, total


@pytest.mark.parametrize("mixer", list(MIXERS))
@pytest.mark.parametrize("N", [1, 3, 32])
def test_param_counts_are_n_networks_and_the_mixer(mixer, N):
    """n_agent = N x the count of one network without the agent id column block; the mixer's count is the shared
    learner's at the same N."""
    one = _counts(_cfg(N=1, distinct=0, **MIXERS[mixer]))
    shared = _counts(_cfg(N=N, distinct=0, **MIXERS[mixer]))
    na, nm, total = _counts(_cfg(N=N, **MIXERS[mixer]))
    assert na == N * one[0] and nm == shared[1] and total == na + nm
    assert (nm > 0) == (mixer == "qmix")
    from maleague.modules.agents.drqn_agent import DRQNAgentNetwork
    args = qmix_args(n_agents=N, n_actions=15, rnn_hidden_dim=64, device="cpu", obs_agent_id=False)
    assert one[0] == sum(p.numel() for p in DRQNAgentNetwork(80 + 15, args).parameters())


@pytest.mark.parametrize("mixer", list(MIXERS))
def test_workspace_is_positive_and_grows_with_n(mixer):
    from maleague import _native
    lib = _native.load()
    sizes = [lib.mlg_qlearner_workspace_floats(_native.byref(_cfg(N=N, **MIXERS[mixer]))) for N in (1, 2, 3, 5, 9, 32)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes


@pytest.mark.parametrize("H", [32, 64, 128])
def test_describe_names_the_distinct_branch(H):
    from maleague import _native
    for mixer, kw in MIXERS.items():
        name = _native.qlearner_describe(_cfg(H=H, **kw))
        assert NAME.match(name), name
        assert name.startswith(f"dx-h{H}/bwd-split/q1 + ")
    assert _native.qlearner_describe(_cfg(H=H)) == f"dx-h{H}/bwd-split/q1 + qmix-generic"  # no split form, no fused backward
    assert _native.qlearner_describe(_cfg(H=H, mixer="vdn")) == f"dx-h{H}/bwd-split/q1 + vdn-fast"
    assert _native.qlearner_describe(_cfg(H=H, N=9, A=17, mixer="vdn")) == f"dx-h{H}/bwd-split/q2 + vdn"
    assert _native.qlearner_describe(_cfg(H=H, mixer=None)) == f"dx-h{H}/bwd-split/q1 + iql"
    assert _native.qlearner_describe(_cfg(H=H, hypernet_layers=1, mixing_embed_dim=16)).endswith("+ qmix1-e16")
    assert _native.qlearner_describe(_cfg(H=H, mixing_embed_dim=64, hypernet_embed=128)).endswith("+ qmix-he128-e64")


@pytest.mark.parametrize("cid", DLS.IDS)
def test_case_arm(cid):
    from maleague import _native
    c = DLS.case(cid)
    name = _native.qlearner_describe(DLS.learner_cfg(c))
    assert name == c.arm and NAME.match(name)
    assert _native.load().mlg_qlearner_workspace_floats(_native.byref(DLS.learner_cfg(c))) > 0


def test_distinct_zero_keeps_todays_names(monkeypatch):
    """The strings tests/test_learner_dispatch.py pins, with the new field at 0 (and obs_agent_id as there)."""
    from maleague import _native
    d = dict(N=5, A=15, S=60, d_obs=80, distinct=0, obs_agent_id=True)
    assert _native.qlearner_describe(_cfg(H=64, **d)) == "h64/bwd-fused/q1 + qmix-split"
    assert _native.qlearner_describe(_cfg(H=64, hypernet_layers=1, mixing_embed_dim=16, **d)) == "h64/bwd-fused/q1 + qmix1-e16"
    assert _native.qlearner_describe(_cfg(H=32, mixing_embed_dim=64, hypernet_embed=128, **d)) == "h32/bwd-split/q1 + qmix-he128-e64"
    monkeypatch.setenv("MLG_MIX_GENERIC", "1")
    assert _native.qlearner_describe(_cfg(H=64, **d)) == "h64/bwd-fused/q1 + qmix-generic"
    assert _native.qlearner_describe(_cfg(H=64, mixer="vdn", **d)) == "h64/bwd-fused/q1 + vdn"
    assert _native.qlearner_describe(_cfg(H=64, mixer=None, **d)) == "h64/bwd-fused/q1 + iql"
    monkeypatch.delenv("MLG_MIX_GENERIC")
    for c in LA.CASES:  # every arm of the shared learner's table
        assert LA.describe(c) == c.arm


@pytest.mark.parametrize("kw,key", [(dict(agent=1), "agent=1"), (dict(obs_agent_id=1), "obs_agent_id=1"),
                                    (dict(N=33), "N=33"), (dict(H=48), "rnn_hidden_dim=48"),
                                    (dict(distinct=2), "distinct=2")],
                         ids=["agent=1", "obs_agent_id=1", "N=33", "H=48", "distinct=2"])
def test_refusals_name_their_key(kw, key):
    from maleague import _native
    lib = _native.load()
    cfg = _cfg()
    assert _native.qlearner_describe(cfg) == "dx-h64/bwd-split/q1 + qmix-generic"
    for k, v in kw.items():
        setattr(cfg, k, v)
    with pytest.raises(_native.NativeError, match=key):
        _native.qlearner_describe(cfg)
    assert lib.mlg_qlearner_workspace_floats(_native.byref(cfg)) == -1
    assert key.encode() in lib.mlg_last_error()
    assert lib.mlg_qlearner_param_counts(_native.byref(cfg), None, None) == -1
    assert key.encode() in lib.mlg_last_error()


def _picks(ref, ob, args, dtype):
    """The picks of the next call: [B, T - 1, N] argmax over the available actions at t + 1 of the online Q (double_q)
    or of the target Q (the index behind the masked max)."""
    ps = ref.agent_states() if args.double_q else [{k: v.detach().clone() for k, v in p.items()} for p in ref.target_states()]
    with torch.no_grad():
        q = DR.mac_unroll(ps, {k: ob[k].to(dtype) for k in ("obs", "actions_onehot")},
                          last_action=bool(args.obs_last_action))[0]
    q = q.masked_fill(ob["avail_actions"] == 0, -9999999)
    return q[:, 1:].argmax(dim=3).numpy()


@pytest.mark.parametrize("cid", DLS.IDS)
def test_oracles_agree_on_every_live_pick(cid):
    c, args, agents0, mixer0, tb = DLS.inputs(cid)   # seed: DLS.case(cid).seed, written beside the case
    ob = DLS.oracle_batch(tb)
    live = DLS.mask(tb) > 0
    assert live.any() and not live[2].any() and live[4].sum() == 1  # the never-filled and the one-transition episode
    r32, r64 = DLS.make_oracle(agents0, mixer0, args), DLS.make_oracle(agents0, mixer0, args, torch.float64)
    total = 0
    for t_env, ep in DLS.CALLS:
        p32, p64 = _picks(r32, ob, args, torch.float32), _picks(r64, ob, args, torch.float64)
        differ = int(((p32 != p64) & live[:, :, None]).sum())
        total += int(live.sum()) * c.N
        assert differ == 0, f"{cid} seed {c.seed}: {differ} live picks differ between the fp32 and the float64 oracle"
        for r in (r32, r64):
            r.train({k: v.clone() for k, v in ob.items()}, t_env, ep)
    print(f"  {cid} seed {c.seed}: 0 of {total} live picks differ")
