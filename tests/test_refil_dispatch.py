"""The dispatch of mlg_refil_rollout, pinned through the host-only query (mlg_refil_rollout_describe; no GPU needed):
which kernel the entry point launches for an entity env spec, agent dims and MLG_REFIL_* environment. The entry point
launches what the query reports (one host function decides for both), so the GPU parity cases of
tests/test_gpu_refil_shapes.py are named after arms this file pins (tests/refil_shapes.py holds the case table).
"""
import pytest

import refil_shapes as FS

LDS_LIMIT = 160 * 1024


def describe(cid):
    from maleague import _native
    spec = FS.spec_for(cid)
    return _native.refil_rollout_describe(spec.to_c(), FS.refil_dims(spec))


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    for k in FS.ENV_VARS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("cid", [c[0] for c in FS.REFIL_CASES])
def test_refil_case_arm(cid, monkeypatch):
    _, codes, kmin, kmax, env, arm, seed = FS.case(cid)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    name, lds = describe(cid)
    assert name == arm
    assert 0 < lds <= LDS_LIMIT


def test_every_slot_count_and_reachable_arm_has_a_case(monkeypatch):
    """Slots 1..8 under the default environment, MLG_REFIL_GENERIC=1 and MLG_REFIL_ROLLOUT=v1: every arm the sweep
    meets is in the case table, every slot count but 6 has a case of its default arm, and ro2/kc3 is never met."""
    from maleague import _native
    from maleague.envs.entity_env import EntityEnvSpec
    default_arms = {len(c[1].split()): c[5] for c in FS.REFIL_CASES if c[4] is None}
    names = {c[5] for c in FS.REFIL_CASES}
    met = set()
    for env in (None, FS.GENERIC, FS.V1):
        for k in FS.ENV_VARS:
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        for S in range(1, 9):
            spec = EntityEnvSpec.from_env_args({"match_build_plan": FS.plan(FS._codes(S)), "min_agents": 1})
            name, _ = _native.refil_rollout_describe(spec.to_c(), FS.refil_dims(spec))
            met.add(name)
            if env is None:  # 6 slots: no case of its own (the same ro4 paths as 5 and 7)
                assert default_arms.get(S, "ro4") == name, S
            if env is FS.V1:
                assert name == ("ro2/kc1" if S == 1 else "ro2/kc2"), S
    assert met == names == {"ro4-static", "ro4", "ro2/kc1", "ro2/kc2"}


def test_forcing_variables(monkeypatch):
    """refil_8 (16 units): the static instantiation by default, the runtime-shape one under MLG_REFIL_GENERIC, the
    two-env kernel under MLG_REFIL_ROLLOUT=v1 (where MLG_REFIL_GENERIC has nothing to select); one slot per team
    (entity input width 15 -> 16) runs the two-env kernel whatever the variables say."""
    assert describe("s8-ro4-static")[0] == "ro4-static"
    monkeypatch.setenv("MLG_REFIL_GENERIC", "1")
    assert describe("s8-ro4-static")[0] == "ro4"
    assert describe("s5-ro4")[0] == "ro4"
    monkeypatch.setenv("MLG_REFIL_ROLLOUT", "v1")
    assert describe("s8-ro4-static")[0] == "ro2/kc2"
    monkeypatch.delenv("MLG_REFIL_GENERIC")
    assert describe("s8-ro4-static")[0] == "ro2/kc2"
    monkeypatch.setenv("MLG_REFIL_ROLLOUT", "v4")
    assert describe("s8-ro4-static")[0] == "ro4-static"
    assert describe("s1-ro2-kc1")[0] == "ro2/kc1"


def test_lds_bytes_follow_the_arm():
    """The reported dynamic LDS is the launch's: four waves of four envs need more than four waves of two."""
    (n4, lds4), (n2, lds2) = describe("s5-ro4"), describe("s1-ro2-kc1")
    assert (n4, n2) == ("ro4", "ro2/kc1")
    assert lds2 < lds4 <= LDS_LIMIT
    assert describe("s8-ro4-static")[1] == lds4


def test_refused_shapes_report_the_entry_points_message():
    from maleague import _native
    spec = FS.spec_for("s5-ro4")
    good = FS.refil_dims(spec)
    assert _native.refil_rollout_describe(spec.to_c(), good)[0] == "ro4"
    # agent dims that do not belong to the env
    for field, value in (("n_agents", 4), ("n_entities", 12), ("n_actions", 21), ("entity_last_action", 0)):
        d = FS.refil_dims(spec)
        setattr(d, field, value)
        with pytest.raises(_native.NativeError, match="do not match the env"):
            _native.refil_rollout_describe(spec.to_c(), d)
    # widths the agent kernels do not have
    d = FS.refil_dims(spec)
    d.rnn_hidden_dim = 32
    with pytest.raises(_native.NativeError, match="rnn_hidden_dim=32"):
        _native.refil_rollout_describe(spec.to_c(), d)
    # team sizes outside the slots, an odd unit count, a scripted policy team
    c = spec.to_c()
    c.max_agents = 6
    with pytest.raises(_native.NativeError, match="min_agents=2 max_agents=6"):
        _native.refil_rollout_describe(c, good)
    c = spec.to_c()
    c.base.U = 9
    with pytest.raises(_native.NativeError, match="U=9 unsupported"):
        _native.refil_rollout_describe(c, good)
    c = spec.to_c()
    c.base.scripted[0] = 1
    with pytest.raises(_native.NativeError, match="policy team 0 and scripted team 1"):
        _native.refil_rollout_describe(c, good)
    # a name buffer that cannot hold the arm
    import ctypes
    lib = _native.load()
    name, lds = ctypes.create_string_buffer(3), ctypes.c_int64(0)
    cspec = spec.to_c()
    rc = lib.mlg_refil_rollout_describe(ctypes.byref(cspec), ctypes.byref(good), name, len(name), ctypes.byref(lds))
    assert rc != 0 and b"name buffer of 3 bytes too small" in lib.mlg_last_error()


def test_stepper_wrapper_declared():
    """EntityParallelStepper exposes the query for the entry point its run() calls; it needs the MAC's agent dims."""
    from maleague.custom_logging import MainLogger
    from maleague.exceptions import MultiAgentControllerNotInitialized
    from maleague.steppers import EntityParallelStepper
    from helpers import refil_args
    stepper = EntityParallelStepper(refil_args(batch_size_run=2, device="cpu", env_args=FS.env_args("s5-ro4")),
                                    MainLogger())
    with pytest.raises(MultiAgentControllerNotInitialized):
        stepper.describe_rollout()
