"""The committed counter evidence bench.py reads into its line (profiles/counters.json): every default-path rollout
kernel has an entry with HBM bytes, and the v7 entry keeps the one-env step cycles the line's latency floor
(roofline.latency_floor_ms) is computed from -- a counter re-collection must not drop them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counters(kernel):
    sys.path.insert(0, ROOT)
    import bench
    return bench.load_counters(kernel)


def test_rollout_counters_present():
    for k in ("rollout_v2_kernel<64, true, 5, 10>", "rollout_sp8_kernel<10, 10>", "refil_rollout4_kernel<2, 16>"):
        c = _counters(k)
        assert c.get("hbm_bytes_per_launch", 0) > 0, k
        assert c.get("commit"), k


def test_v7_latency_floor_annotation_present():
    c = _counters("rollout_v2_kernel<64, true, 5, 10>")
    assert c.get("one_env_step_cycles", 0) > 10000
    assert "stamps" in c.get("one_env_step_source", "")


V7_SOURCES = ("ma-league_amd/csrc/rollout.hip", "ma-league_amd/csrc/rollout_env_device.h",
              "ma-league_amd/csrc/mlg_device.h", "ma-league_amd/csrc/agent_device.h")


def test_v7_latency_floor_stamp_is_current():
    """the one-env step cycles behind roofline.latency_floor_ms must come from the v7 sources in the
    tree. The stamp records the sha256 of every v7 source file it was measured on (one_env_step_sources) next to the
    commit it was measured on top of, and the files in the tree must hash to the same: any edit of them, committed or
    not, with or without git history, fails until the step is re-measured. (The earlier form compared commit
    ancestry, which a change that edits a v7 source and re-measures in the same commit cannot satisfy: the stamp
    would have to name the hash of the commit that contains it.)"""
    import hashlib
    c = _counters("rollout_v2_kernel<64, true, 5, 10>")
    assert c.get("one_env_step_commit"), "the v7 one-env step cycles name the commit they were measured on top of"
    stamped = c.get("one_env_step_sources")
    assert stamped and set(stamped) == set(V7_SOURCES), "the v7 one-env step cycles list the sources they belong to"
    for path in V7_SOURCES:
        with open(os.path.join(ROOT, path), "rb") as f:
            now = hashlib.sha256(f.read()).hexdigest()
        assert now == stamped[path], (f"{path} changed after the one-env step stamp: re-measure with the stamps build "
                                      "(make -C ma-league_amd stamps; MLG_ROLLOUT_KERNEL=v7 MLG_LIB=<stamps library> "
                                      "python scripts/stamps_rollout.py) and update profiles/counters.json")
