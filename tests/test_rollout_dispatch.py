"""The rollout dispatch table, pinned through the host-only query (mlg_rollout_describe; no GPU needed): which kernel
mlg_rollout / mlg_rollout_selfplay launch for a spec, agent dims and MLG_ROLLOUT_* environment. The entry points
launch what the query reports (one host function decides for both), so the GPU parity cases of
tests/test_gpu_rollout_shapes.py are named after arms this file pins.

Arm names: v7-static / v7 (split-bf16, H = 64; compile-time 5v5 or 3v3 shape / runtime shape), v2 (fp32 compacted,
H = 32 or 64), v1-lds/tpwK and v1-global/tpwK (the generic kernel, weights in LDS / read from global memory, K agent
tiles per wave), sp8 / sp7-static / sp7 / sp2 (two policies).

Arms that the default environment does not reach (found by the sweep in test_default_arms_all_have_a_gpu_case; the
160 KiB LDS limit decides most of them):
  * v1-lds at H = 128, and v1-lds/tpw2..4 at H = 64: one policy's weights plus the env arrays fit LDS only up to 7v7
    at H = 64 (one tile per wave) and never at H = 128. v1-lds/tpw1 at 5v5 / 3v3 is reached with
    MLG_ROLLOUT_KERNEL=v1 (test_rollout_v2_equals_v1, test_rollout_ring_mode_zero_copy_insert).
  * v2 at H = 64 for symmetric plans: up to 5v5 the v7 layout fits as well and wins, from 6v6 on neither fits. It is
    the default only for asymmetric plans such as 5 agents against 7 or 8 scripted units (case v2-default-5v7);
    MLG_ROLLOUT_KERNEL=v2 reaches it at 5v5 / 3v3.
  * sp2 at H = 64: wherever its layout fits, sp7 (or sp8) fits too. MLG_ROLLOUT_KERNEL=sp2 reaches it
    (test_selfplay_kernel_equals_v1).
  * sp7-static: sp8 takes the 5v5 / 3v3 self-play shapes first. MLG_ROLLOUT_KERNEL=sp7 reaches it
    (test_selfplay_sp7_split_bf16_matches_fp32).
  * v1 self-play with one tile per wave at H = 32 / 64 (sp2 / sp7 take every shape up to 7v7 / 5v5); H = 128 reaches
    it (case v1sp-h128-3v3).
"""
import pytest

import rollout_shapes as RS
from helpers import drqn_dims, shape_plan

LDS_LIMIT = 160 * 1024


def describe(plan, hidden, self_play=False):
    from maleague import _native
    from maleague.envs.teams_env import TeamsEnvSpec
    spec = TeamsEnvSpec.from_env_args({"match_build_plan": shape_plan(plan, self_play), "grid_size": 20,
                                       "stochastic_spawns": True, "episode_limit": RS.EPISODE_LIMIT})
    return _native.rollout_describe(spec.to_c(), drqn_dims(spec, hidden, self_play), self_play)


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    for k in ("MLG_ROLLOUT_KERNEL", "MLG_ROLLOUT_GENERIC", "MLG_ROLLOUT_GLOBAL_WEIGHTS"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("cid,hidden,plan,arm,seed", RS.ROLLOUT_CASES, ids=[c[0] for c in RS.ROLLOUT_CASES])
def test_rollout_case_arm(cid, hidden, plan, arm, seed):
    name, lds = describe(plan, hidden)
    assert name == arm
    assert 0 < lds <= LDS_LIMIT


@pytest.mark.parametrize("cid,hidden,plan,arm,seed", RS.SELFPLAY_CASES, ids=[c[0] for c in RS.SELFPLAY_CASES])
def test_selfplay_case_arm(cid, hidden, plan, arm, seed):
    name, lds = describe(plan, hidden, self_play=True)
    assert name == arm
    assert 0 < lds <= LDS_LIMIT


@pytest.mark.parametrize("plan", ["medium_1h_4t", "small"])
def test_existing_shapes_and_forcing_variables(plan, monkeypatch):
    """5v5 and 3v3 at H = 64: the compile-time instantiations by default, the runtime-shape kernels under
    MLG_ROLLOUT_GENERIC, and whatever MLG_ROLLOUT_KERNEL names (a name of the other entry point is ignored)."""
    assert describe(plan, 64)[0] == "v7-static"
    assert describe(plan, 64, True)[0] == "sp8"
    monkeypatch.setenv("MLG_ROLLOUT_GENERIC", "1")
    assert describe(plan, 64)[0] == "v7"
    assert describe(plan, 64, True)[0] == "sp7"
    monkeypatch.delenv("MLG_ROLLOUT_GENERIC")
    tpw_sp = {"medium_1h_4t": 2, "small": 1}[plan]  # 2 x ceil(16 x 5 / 16) = 10 tiles on 8 waves; 2 x 3 = 6 on 6
    for forced, single, selfplay in (("v1", "v1-lds/tpw1", f"v1-global/tpw{tpw_sp}"), ("v2", "v2", "sp8"),
                                     ("v7", "v7-static", "sp8"), ("sp2", "v7-static", "sp2"),
                                     ("sp7", "v7-static", "sp7-static")):
        monkeypatch.setenv("MLG_ROLLOUT_KERNEL", forced)
        assert describe(plan, 64)[0] == single, forced
        assert describe(plan, 64, True)[0] == selfplay, forced
    monkeypatch.setenv("MLG_ROLLOUT_GENERIC", "1")
    assert describe(plan, 64, True)[0] == "sp7"  # forced sp7, runtime shape
    monkeypatch.setenv("MLG_ROLLOUT_KERNEL", "v7")
    assert describe(plan, 64)[0] == "v7"
    monkeypatch.delenv("MLG_ROLLOUT_GENERIC")
    monkeypatch.delenv("MLG_ROLLOUT_KERNEL")
    monkeypatch.setenv("MLG_ROLLOUT_GLOBAL_WEIGHTS", "1")
    assert describe("7v7", 64)[0] == "v1-global/tpw1"  # v1-lds/tpw1 by default (case v1-h64-7v7)


def test_lds_bytes_follow_the_arm():
    """The reported dynamic LDS is the launch's: the v7 layout of the headline 5v5 plan is the largest that fits
    (163472 of 163840 bytes), v1 without weights in LDS needs a few KiB."""
    assert describe("medium_1h_4t", 64) == ("v7-static", 163472)
    assert describe("medium_1h_4t", 64, True) == ("sp8", 155808)
    name, lds = describe("large", 64)
    assert name == "v1-global/tpw4" and lds < 32 * 1024


def test_refused_shapes_report_the_entry_points_message():
    from maleague import _native
    from maleague.envs.teams_env import TeamsEnvSpec
    # more than 4 agent tiles per wave: 2 x ceil(16 x 17 / 16) = 34 tiles on 8 waves
    with pytest.raises(_native.NativeError, match="5 agent tiles per wave > 4"):
        describe("17v17", 64, self_play=True)
    with pytest.raises(_native.NativeError, match="agent tiles per wave > 4"):
        describe("large", 64, self_play=True)
    assert describe("16v16", 64, self_play=True)[0] == "v1-global/tpw4"  # the largest self-play shape
    assert describe("32v32", 64)[0] == "v1-global/tpw4"                 # and the largest plan (64 units)
    # rnn_hidden_dim outside 32 / 64 / 128
    spec = TeamsEnvSpec.from_env_args({"match_build_plan": "small"})
    for hidden in (16, 48, 96, 256):
        with pytest.raises(_native.NativeError, match=f"rnn_hidden_dim={hidden} unsupported"):
            _native.rollout_describe(spec.to_c(), drqn_dims(spec, hidden), False)
    # agent dims that do not belong to the env, and a scripted team in a self-play call
    with pytest.raises(_native.NativeError, match="agent dims do not match"):
        _native.rollout_describe(spec.to_c(), drqn_dims(spec, 64, self_play=True), False)
    with pytest.raises(_native.NativeError, match="symmetric two-team scenario"):
        _native.rollout_describe(spec.to_c(), drqn_dims(spec, 64, self_play=True), True)


def test_default_arms_all_have_a_gpu_case():
    """Every (entry point, H, arm) the default environment can reach with a symmetric K-vs-K plan (K = 1..32), the
    `large` plan or one of the asymmetric plans appears in a GPU parity case: the case tables, or the earlier suites
    for v7-static / sp8. The module docstring lists the arms this sweep never meets."""
    plans = [f"{k}v{k}" for k in range(1, 33)] + ["large", "5v7", "3v5", "medium_1h_4t", "small"]
    for self_play, cases in ((False, RS.ROLLOUT_CASES), (True, RS.SELFPLAY_CASES)):
        have = {(c[1], c[3]) for c in cases} | {(64, a) for a in RS.ARMS_COVERED_ELSEWHERE}
        names = {c[3] for c in cases} | RS.ARMS_COVERED_ELSEWHERE
        for hidden in (32, 64, 128):
            for plan in plans:
                if self_play and plan in ("5v7", "3v5"):
                    continue
                try:
                    name, _ = describe(plan, hidden, self_play)
                except Exception as e:  # refused shapes: only the tiles-per-wave limit
                    assert "agent tiles per wave > 4" in str(e), (plan, hidden, self_play)
                    continue
                assert name in names, (plan, hidden, self_play, name)
                if not name.startswith("v1"):  # the specialised kernels: per H as well
                    assert (hidden, name) in have, (plan, hidden, self_play, name)


def test_stepper_wrapper_declared():
    """The steppers expose the query (describe_rollout) for the entry point their run() calls."""
    from maleague.steppers import ParallelStepper, SelfPlayParallelStepper
    assert ParallelStepper._SELFPLAY is False and SelfPlayParallelStepper._SELFPLAY is True
    assert callable(ParallelStepper.describe_rollout)
