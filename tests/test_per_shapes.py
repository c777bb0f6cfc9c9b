"""The conditions the GPU parity pass of tests/test_gpu_per_shapes.py rests on, checked on the CPU against the float64
oracle alone (tests/per_ref.py): no sampling case has a near tie, the case tables are what their comments say, the
dispatch names gain " + per" and nothing else, and every figure of per_shapes.ORACLE_F64 leaves the project's bounds in
force."""
import numpy as np
import pytest

import learner_arm_shapes as LA
import per_cases as PC
import per_ref as PR
import per_shapes as PS


# ---- 1. sampling -------------------------------------------------------------------------------------------------------
def test_sampling_table_covers_the_kernels_edges():
    from maleague import _native
    lib = _native.load()
    lds, top = lib.mlg_per_lds_slots(), lib.mlg_per_max_slots()
    assert (lds, top) == (6144, PS.MAX_SLOTS)
    live = {c.n for c in PS.SAMPLE_CASES}
    assert {1024, 1025, lds, lds + 1, top} == live
    assert {c.B for c in PS.SAMPLE_CASES} == {64, 1024, 1025, 4096}
    assert {c.beta for c in PS.SAMPLE_CASES} == {0.0, PC.BETA, 1.0}
    for c in PS.SAMPLE_CASES:
        assert 2e-9 * c.n * c.B < 2.2, f"{c.id}: too many near ties expected for a seed search"
        if c.B == 4096:
            assert c.n <= 65536
    assert len(set(PS.SAMPLE_IDS)) == len(PS.SAMPLE_IDS) and set(PS.SAMPLE_SEEDS) == set(PS.SAMPLE_IDS)
    assert not set(PS.SAMPLE_IDS) & set(PC.SAMPLE_IDS)
    for kind in PS.SAMPLE_KINDS:  # every live count and every batch with every kind of priorities
        assert {(c.n, c.B) for c in PS.SAMPLE_CASES if c.kind == kind} >= \
            {(n, B) for n in (1024, 1025, lds, lds + 1) for B in (1024, 1025, 4096)} | {(top, 64)}


@pytest.mark.parametrize("sid", PS.SAMPLE_IDS)
def test_gpu_sampling_inputs_have_no_near_tie(sid):
    p, n, B, seed, draw, beta = PS.sample_case(sid)
    rows, w, margin = PR.sample(p, n, B, seed, draw, beta)
    assert margin > PC.NEAR_TIE, f"{sid}: a draw lies {margin:.3e} of the total from a boundary; pick another seed"
    assert PS.sample_base_seed(sid) <= seed < PS.sample_base_seed(sid) + 64
    assert rows.min() >= 0 and rows.max() < n and w.max() == 1.0 and w.min() > 0.0 and np.all(np.isfinite(w))
    kind = sid.split("-")[0]
    if kind == "skewed":
        assert np.bincount(rows).max() >= 0.85 * B  # the heavy slot spans ~90 % of the strata
    if kind == "zeros":
        assert p[0] != 0 and p[-1] == 0 and 0.28 < float(np.mean(p == 0)) < 0.39
        assert np.all(p[rows] != 0)  # the rule never selects a slot of priority 0
    if beta == 0.0:
        assert np.all(w == 1.0)
    if B > 1024:
        assert len(set(PR.uniforms(seed, draw, B)[[0, 1024]])) == 2  # the passes draw from different counters


def test_index_field_of_the_counter_holds_the_last_draw():
    """i = 4095 is the largest index mlg_ctr's 12-bit field holds: draws 4095 and 0 of a call differ, and no draw of a
    4096-draw call aliases another."""
    ctrs = {PR.ctr(3, 0, PR.PER_PURPOSE, i) for i in range(4096)}
    assert len(ctrs) == 4096 and PR.ctr(3, 0, PR.PER_PURPOSE, 4096) == PR.ctr(3, 0, PR.PER_PURPOSE, 0)


@pytest.mark.parametrize("sid", ["zeros-n1025-b1025", "skewed-n1024-b4096", "flat-n1025-b1024"])
def test_neighbour_margin_is_the_full_minimum(sid):
    """per_ref.neighbour_margin (each draw's two neighbouring boundaries) against the minimum over every boundary."""
    p, n, B, seed, draw, _ = PS.sample_case(sid)
    cum = np.cumsum(np.asarray(p[:n], dtype=np.float64))
    s = PR.strata(cum[-1], PR.uniforms(seed, draw, B), B)
    full = float(np.min(np.abs(cum[None, :] - s[:, None])))
    assert PR.neighbour_margin(cum, s, PR.select(cum, s)) == full


# ---- 2. the arms -------------------------------------------------------------------------------------------------------
def test_arm_table_is_every_case_of_the_three_tables():
    import distinct_learner_shapes as DLS
    import dqn_shapes as DS
    assert PS.ARM_IDS == [f"rnn:{c}" for c in LA.IDS] + [f"dqn:{c}" for c in DS.LEARNER_IDS] + \
        [f"distinct:{c}" for c in DLS.IDS]
    assert len(PS.ARM_IDS) == 24 + 8 + 6


@pytest.mark.parametrize("aid", PS.ARM_IDS)
def test_arm_describe_gains_per(aid):
    from maleague import _native
    lib = _native.load()
    _, _, arm = PS.arm_case(aid)
    off, on = PS.arm_cfg(aid, 0), PS.arm_cfg(aid, 1)
    assert _native.qlearner_describe(off) == arm and _native.qlearner_describe(on) == arm + " + per"
    w0, w1 = (lib.mlg_qlearner_workspace_floats(_native.byref(c)) for c in (off, on))
    assert w0 > 0 and w1 == w0 + (off.B * (off.T - 1) + 3) // 4 * 4


@pytest.mark.parametrize("aid", PS.ARM_IDS)
def test_arm_weights(aid):
    w = PS.arm_weight(aid)
    assert w.dtype == np.float32 and w.max() == 1.0 and w.min() > 0.1 and len(np.unique(w)) == len(w)
    assert len(w) == PS.arm_cfg(aid, 1).B


# ---- 3. the reduce cases -----------------------------------------------------------------------------------------------
def _cfg(rid, T, per=1):
    rc, _, c = PS.reduce_case(rid)
    cfg = LA.learner_cfg(LA.case_args(c, "cpu"), LA.dims(c)[3], B=len(rc.rows or rc.lens), T=T)
    cfg.per = per
    return cfg


def test_reduce_table_is_the_issues():
    want = {"t65": (3, 65, (65, 64, 2)), "t66": (3, 66, (66, 65, 2)), "t130": (2, 131, (130, 40)), "b1": (1, 8, (6,)),
            "hole": (4, 12, (10, 10, 7, 3)), "view101": (6, 101, (100, 71, 65, 64, 2, 0))}
    for rc in PS.REDUCE_CASES:
        assert len(rc.lens) == rc.B and max(rc.lens) <= rc.T
        if rc.id in want:
            assert (rc.B, rc.T, rc.lens) == want[rc.id]
    b72 = next(c for c in PS.REDUCE_CASES if c.id == "b72")
    assert (b72.B, b72.T) == (72, 8) and b72.lens.count(0) == 4 and len(set(b72.lens)) >= 6
    assert [c.id for c in PS.REDUCE_CASES] == ["t65", "t66", "t130", "b1", "b72", "hole", "view101"]
    assert sorted(PS.REDUCE_IDS) == sorted([f"{c.id}-{m}" for c in PS.REDUCE_CASES for m in ("qmix", "iql")] + ["t66-vdn"])
    view = PS.REDUCE_CASES[-1]
    assert len(set(view.rows)) == view.B < len(view.rows)  # every stored episode, one of them twice


@pytest.mark.parametrize("rid", PS.REDUCE_IDS)
def test_reduce_case_reaches_what_it_is_for(rid):
    from maleague import _native
    rc, mix, c, args, _, _, stored, tb = PS.reduce_inputs(rid)
    assert LA.dims(c)[0] == 2 and c.H == 32
    m, mlen = PS.reduce_mask(tb), PS.reduce_mlen(tb)
    Te = m.shape[1] + 1
    assert Te == max(2, max(rc.lens))
    assert _native.qlearner_describe(_cfg(rid, Te)) == c.arm + " + per"  # the name at the trained length
    assert _native.qlearner_describe(_cfg(rid, rc.T)) == c.arm + " + per"  # and at the stored length the learner sees
    steps = m.sum(axis=1)
    if rc.id == "t65":
        assert mlen.max() == 64 == steps.max()
    if rc.id == "t66":
        assert mlen.max() == 65 == steps.max()
    if rc.id == "t130":
        assert mlen.max() == 129 and rc.T > 128
    if rc.id == "b1":
        assert tb["filled"].shape[0] == 1
    if rc.id == "b72":
        assert rc.B > 64 and int((steps == 0).sum()) == 4 and steps.max() == 5
    if rc.id == "hole":
        assert mlen.tolist() == [9, 9, 7, 3] and steps.tolist() == [8, 9, 6, 3]
        assert (mlen > steps).tolist() == [True, False, True, False]
    else:
        assert np.array_equal(mlen, steps)  # every other mask is a prefix
    if rc.id == "view101":
        assert mlen.max() == 99 and rc.T - 1 == 100 and tb["filled"].shape[0] == 7 and steps.min() == 0
        assert np.array_equal(tb["obs"][0].numpy(), tb["obs"][2].numpy())
    w = PS.reduce_weight(rid)
    assert len(w) == tb["filled"].shape[0] and w.max() == 1.0 and w.min() > 0.1
    n_av = tb["avail_actions"].sum(-1)
    assert bool((n_av > 0).all())


# ---- 4. the figures ----------------------------------------------------------------------------------------------------
def test_float64_distance_table_and_bounds():
    """Every case without a figure in learner_arm_shapes.ORACLE_F64 has one here, and ten times no distance exceeds a
    project bound: the bounds in force are the project's everywhere."""
    want = [a for a in PS.ARM_IDS if not a.startswith("rnn:")] + \
        [r for r in PS.REDUCE_IDS if r.split("-")[0] in PS.REDUCE_LONG]
    assert sorted(PS.ORACLE_F64) == sorted(want)
    for key in PS.ARM_IDS + PS.REDUCE_IDS:
        assert PS.bounds(key) == (LA.STAT_RTOL, LA.GRAD_RTOL, PS.OP_TOL), key


@pytest.mark.parametrize("key", ["dqn:ff-vdn-h32-3v3", "distinct:n2-h32-b17", "t130-iql"])
def test_float64_distance_figures_reproduce(key):
    """The recorded distance of the fp32 weighted oracle from its float64 run, measured again for three cases (the
    script's arithmetic; within a factor of two: BLAS thread counts move fp32 sums)."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "per_oracle_f64_distance.py")
    spec = importlib.util.spec_from_file_location("per_oracle_f64_distance", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if ":" in key:
        kind, _, args, agent0, mixer0, tb = PS.arm_inputs(key)
        w = PS.arm_weight(key)
    else:
        kind, (_, _, _, args, agent0, mixer0, _, tb), w = "rnn", PS.reduce_inputs(key), PS.reduce_weight(key)
    ds, dg, dt, _ = mod.distance(kind, args, agent0, mixer0, tb, w)
    for got, rec in zip((ds, dg, dt), PS.ORACLE_F64[key]):
        assert got <= 2 * rec + 1e-9 and 10 * got < LA.GRAD_RTOL, (key, got, rec)
