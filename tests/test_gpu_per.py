"""GPU parity of prioritized episode replay: mlg_per_sample / mlg_per_insert / mlg_per_update against
the float64 oracle (tests/per_ref.py, pinned to the reference's sum tree by tests/test_per.py), the fused learner's
per = 1 forms at one case per TD site and agent kind (tests/per_cases.py), and MultiAgentExperiment end to end.

Bounds. Rows: exact (tests/test_per.py checks on the CPU that no draw of a case is a near tie). Weights, priorities and
td_abs: the project's op bound 1e-4 max(1, max|ref|) against float64. First-call gradients: per tensor
max|g - g_ref| <= 1e-4 max(1, max|g_ref|) against the float64 weighted oracle before its clip, the bound of
tests/test_gpu_learner_arms.py. Everything else is bit equality.
"""
import numpy as np
import pytest
import torch

import learner_arm_shapes as LA
import per_cases as PC
import per_ref as PR
from helpers import scheme_for
from test_gpu_learner_shapes import _episode_batch, _learner

pytestmark = pytest.mark.gpu

OP_TOL = 1e-4  # the project's bar for op outputs against float64
SENTINEL = -7.0


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    for k in ("MLG_MIX_GENERIC", "MLG_LEARNER_FULL", "MLG_DISTINCT_LEARNER"):
        monkeypatch.delenv(k, raising=False)


def _close(got, ref, what):
    ref = np.asarray(ref, dtype=np.float64)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
    bound = OP_TOL * max(1.0, float(np.abs(ref).max()))
    assert err <= bound, f"{what}: max error {err:.3e} > {bound:.3e}"
    return err / bound


# ---- 1. mlg_per_sample -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", PC.SAMPLE_IDS)
def test_per_sample_vs_oracle(device, sid):
    from maleague import _native
    lib = _native.load(require_gpu=True)
    p, n, B, seed, draw = PC.sample_case(sid)
    want_rows, want_w, margin = PR.sample(p, n, B, seed, draw, PC.BETA)
    assert margin > PC.NEAR_TIE
    prio = torch.from_numpy(p).to(device)
    rows = torch.full((B + 2,), -5, dtype=torch.int32, device=device)  # a guard element on either side
    w = torch.full((B + 2,), SENTINEL, dtype=torch.float32, device=device)
    ws = torch.full((n,), float("nan"), dtype=torch.float64, device=device) if n > lib.mlg_per_lds_slots() else None
    _native.call("mlg_per_sample", prio.data_ptr(), n, B, seed, draw, PC.BETA, rows[1:].data_ptr(), w[1:].data_ptr(),
                 None if ws is None else ws.data_ptr(), 0 if ws is None else n, _native.stream_ptr(device))
    torch.cuda.synchronize()
    assert rows[0] == -5 and rows[-1] == -5 and w[0] == SENTINEL and w[-1] == SENTINEL
    assert np.array_equal(rows[1:-1].cpu().numpy().astype(np.int64), want_rows), sid
    worst = _close(w[1:-1].cpu().numpy(), want_w, f"{sid} is_weight")
    assert torch.equal(prio.cpu(), torch.from_numpy(p))
    print(f"  {sid}: margin {margin:.2e}, is_weight error / bound {100 * worst:.3f} %")


def test_device_and_host_buffers_draw_the_same_rows(device):
    """PrioritizedReplayBuffer on the device and on the host with the same priorities, seed and draw counter: the same
    rows and (to fp32 rounding) weights over several draws, beta annealed alike; the view never copies its rows."""
    from maleague.components.replay_buffer import PrioritizedReplayBuffer, PrioritizedSampledEpisodeBatch
    scheme, groups, pre = scheme_for({"state_shape": 4, "obs_shape": 3, "n_actions": 3, "n_agents": 2}, torch)
    p = torch.from_numpy(np.random.RandomState(4).uniform(0.05, 3.0, size=5000).astype(np.float32))
    bufs = []
    for dev in ("cpu", device):
        buf = PrioritizedReplayBuffer(scheme, groups, 5000, 3, preprocess=pre, device=dev, seed=21)
        buf.priorities.copy_(p)
        buf.episodes_in_buffer = 4000  # a partially filled buffer
        bufs.append(buf)
    for k in range(3):
        host = bufs[0].sample(32)
        view = bufs[1].sample(32, view=True)
        assert isinstance(view, PrioritizedSampledEpisodeBatch) and view.host_rows is None and view._data is None
        assert view.rows.is_cuda and view.rows.dtype == torch.int32 and view.is_weight.is_cuda
        want_rows, want_w, margin = PR.sample(p.numpy(), 4000, 32, 21, k, bufs[0].beta)
        assert margin > PC.NEAR_TIE
        assert np.array_equal(host.rows.numpy(), want_rows) and np.array_equal(view.rows.cpu().numpy(), want_rows)
        _close(view.is_weight.cpu().numpy(), want_w, "device weights")
        _close(host.is_weight.numpy(), want_w, "host weights")
        assert view._ep_ids is None and np.array_equal(view.ep_ids, want_rows)
    assert bufs[0].beta == bufs[1].beta == PR.BETA + 3 * PR.BETA_INCREMENT and bufs[1].draws == 3


# ---- 2. mlg_per_insert / mlg_per_update ------------------------------------------------------------------------------
def _prio_state(device, ring, max_p):
    return (torch.full((ring,), SENTINEL, dtype=torch.float32, device=device),
            torch.tensor([max_p], dtype=torch.float32, device=device))


def test_per_insert_wrapping_range(device):
    from maleague import _native
    ring, slot0, count = 37, 33, 9  # slots 33..36 and 0..4
    named = (slot0 + np.arange(count)) % ring
    rest = np.setdiff1d(np.arange(ring), named)
    # the maximum
    prio, mx = _prio_state(device, ring, 2.5)
    _native.call("mlg_per_insert", prio.data_ptr(), ring, slot0, count, None, PR.E, PR.A, mx.data_ptr(),
                 _native.stream_ptr(device))
    got = prio.cpu().numpy()
    assert np.all(got[named] == np.float32(2.5)) and np.all(got[rest] == np.float32(SENTINEL)) and float(mx) == 2.5
    # errors: err = 0 among them, and one that raises the maximum
    err = np.asarray([0.0, 0.3, -1.2, 40.0, 0.01, 2.0, 0.0, 0.5, 7.0], np.float32)
    prio, mx = _prio_state(device, ring, 2.5)
    e = torch.from_numpy(err).to(device)
    _native.call("mlg_per_insert", prio.data_ptr(), ring, slot0, count, e.data_ptr(), PR.E, PR.A, mx.data_ptr(),
                 _native.stream_ptr(device))
    got = prio.cpu().numpy()
    want = PR.priority(err)
    _close(got[named], want, "insert priorities")
    assert got[named][0] == got[named][6] == np.float32(PR.E ** PR.A)
    assert np.all(got[rest] == np.float32(SENTINEL))
    assert float(mx) == got[named].max() > 2.5
    # an insert that does not reach the maximum leaves it
    prio, mx = _prio_state(device, ring, 50.0)
    _native.call("mlg_per_insert", prio.data_ptr(), ring, slot0, count, e.data_ptr(), PR.E, PR.A, mx.data_ptr(),
                 _native.stream_ptr(device))
    assert float(mx) == 50.0


def test_per_update_duplicates_maximum_and_zero_error(device):
    from maleague import _native
    n = 300
    rows = np.asarray([5, 299, 5, 0, 17, 5, 299, 64], np.int32)  # slots 5 and 299 repeat
    td_u = {5: 0.7, 299: 0.0, 0: 12.5, 17: 1e-4, 64: 3.0}
    td = np.asarray([td_u[int(r)] for r in rows], np.float32)
    prio, mx = _prio_state(device, n, 1.0)
    r, t = torch.from_numpy(rows).to(device), torch.from_numpy(td).to(device)
    _native.call("mlg_per_update", prio.data_ptr(), n, r.data_ptr(), t.data_ptr(), len(rows), PR.E, PR.A, mx.data_ptr(),
                 _native.stream_ptr(device))
    got = prio.cpu().numpy()
    ref = np.full(n, SENTINEL)
    new_max = PR.update(ref, 1.0, rows, td)
    named = np.unique(rows)
    _close(got[named], ref[named], "update priorities")
    assert got[299] == np.float32(PR.E ** PR.A)  # err = 0
    rest = np.setdiff1d(np.arange(n), named)
    assert np.all(got[rest] == np.float32(SENTINEL))
    assert float(mx) == got[named].max() and abs(float(mx) - new_max) <= OP_TOL * new_max and float(mx) > 1.0
    # identity rows, a maximum that stays
    prio, mx = _prio_state(device, n, 99.0)
    _native.call("mlg_per_update", prio.data_ptr(), n, None, t.data_ptr(), len(rows), PR.E, PR.A, mx.data_ptr(),
                 _native.stream_ptr(device))
    got = prio.cpu().numpy()
    _close(got[:len(rows)], PR.priority(td), "identity update")
    assert np.all(got[len(rows):] == np.float32(SENTINEL)) and float(mx) == 99.0


# ---- 3. the fused learner with per = 1 ---------------------------------------------------------------------------------
def _build(pid, eb):
    pc, args, agent0, mixer0, _ = PC.learner_inputs(pid)
    if pc.kind == "distinct":
        from test_gpu_distinct_learner_fused import _distinct_learner
        return _distinct_learner(eb, args, agent0, mixer0)[0]
    return _learner(eb, agent0, mixer0, args)[0]


def _env(pid, monkeypatch):
    for k, v in PC.learner_case(pid).env.items():
        monkeypatch.setenv(k, v)


def _batch(pid, device, weights=None):
    eb = _episode_batch(PC.learner_inputs(pid)[4], device)
    if weights is not None:
        eb.is_weight = torch.as_tensor(weights)
    return eb


def _snap(learner):
    torch.cuda.synchronize()
    out = {"stats": learner._stats.cpu().numpy().copy(), "grads": learner._grads.cpu().numpy().copy(),
           "params": learner._flat.flat.cpu().numpy().copy(), "sq": learner._sq.cpu().numpy().copy()}
    if learner.last_td_abs is not None:
        out["td_abs"] = learner.last_td_abs.cpu().numpy().copy()
    return out


def _same(a, b, what, keys=("stats", "grads", "params", "sq")):
    for k in keys:
        x, y = (a[k][:7], b[k][:7]) if k == "stats" else (a[k], b[k])
        assert np.array_equal(x, y), f"{what}: {k} differ at {np.flatnonzero(x != y)[:8]}"


def _describe(learner, eb, per):
    from maleague import _native
    return _native.qlearner_describe(learner._cfg(LA.B, LA.T_FILLED, per=per))


@pytest.mark.parametrize("pid", PC.LEARNER_IDS)
def test_unit_weights_are_the_unweighted_call(device, monkeypatch, pid):
    """(a) is_weight = 1 everywhere: parameters, gradients, RMSprop state and statistics bit-identical to the per = 0
    call over two calls (target a copy, then stale); td_abs averages to the call's td_error_abs."""
    _env(pid, monkeypatch)
    pc = PC.learner_case(pid)
    plain_b, per_b = _batch(pid, device), _batch(pid, device, np.ones(LA.B, np.float32))
    plain, per = _build(pid, plain_b), _build(pid, per_b)
    assert _describe(plain, plain_b, 0) == pc.case.arm and _describe(per, per_b, 1) == pc.case.arm + " + per"
    for call, ep in enumerate([0, 200]):
        plain.train(plain_b, 0, ep)
        per.train(per_b, 0, ep)
        a, b = _snap(plain), _snap(per)
        _same(a, b, f"{pid} call {call}")
        assert plain.last_td_abs is None and b["td_abs"].shape == (LA.B,) and np.all(np.isfinite(b["td_abs"]))
        m = _mask_sums(pid)
        mean = float((b["td_abs"].astype(np.float64) * m).sum() / m.sum())
        np.testing.assert_allclose(mean, b["stats"][2], rtol=2e-4)
        assert np.all(b["td_abs"][m == 0] == 0.0)


def _mask_sums(pid):
    tb = PC.learner_inputs(pid)[4]
    f = tb["filled"][:, :LA.T_FILLED - 1, 0].numpy().astype(np.float64)
    t = tb["terminated"][:, :LA.T_FILLED - 1, 0].numpy().astype(np.float64)
    m = f.copy()
    m[:, 1:] *= 1 - t[:, :-1]
    return m.sum(axis=1)


@pytest.mark.parametrize("pid", PC.LEARNER_IDS)
def test_weighted_gradients_and_errors_vs_float64_oracle(device, monkeypatch, pid):
    """(b) random weights in (0.1, 1]: the first call's gradients per tensor (scaled back by the clip factor) and
    td_abs against the float64 PERLearnerRef; the weighted loss and the unweighted statistics against its."""
    _env(pid, monkeypatch)
    g64, td64, s64 = PC.oracle_f64(pid)
    eb = _batch(pid, device, PC.is_weight(pid))
    learner = _build(pid, eb)
    learner.train(eb, 0, 0)
    got = _snap(learner)
    norm = float(got["stats"][1])
    np.testing.assert_allclose(norm, s64["grad_norm"], rtol=LA.STAT_RTOL)
    coef = min(1.0, learner.args.grad_norm_clip / (norm + 1e-6))  # clip_grad_norm_
    views = learner._flat.views
    assert len(views) == len(g64)
    grads = torch.from_numpy(got["grads"])
    worst = 0.0
    for (q, off, k), ref in zip(views, g64):
        assert tuple(q.shape) == tuple(ref.shape)
        mine = grads[off:off + k].view_as(q).to(torch.float64) / coef
        err, scale = float((mine - ref).abs().max()), max(1.0, float(ref.abs().max()))
        worst = max(worst, err / (LA.GRAD_RTOL * scale))
        assert err <= LA.GRAD_RTOL * scale, f"{pid} tensor at {off} {tuple(q.shape)}: {err:.3e} > {LA.GRAD_RTOL * scale:.3e}"
    wt = _close(got["td_abs"], td64.numpy(), f"{pid} td_abs")
    for i, k in ((0, "loss"), (2, "td_error_abs"), (3, "q_taken_mean"), (4, "target_mean")):
        np.testing.assert_allclose(got["stats"][i], s64[k], rtol=LA.STAT_RTOL, atol=LA.STAT_ATOL, err_msg=f"{pid} {k}")
    print(f"  {pid}: grad_norm {norm:.6g} (clip {coef:.4g}), gradient error / bound {100 * worst:.2f} %, "
          f"td_abs error / bound {100 * wt:.3f} %")


@pytest.mark.parametrize("pid", PC.LEARNER_IDS)
def test_slot_maps_with_duplicated_rows(device, monkeypatch, pid):
    """(c) the case's episodes sampled with a duplicated row as an in-place view of a device replay ring: through the
    kernel-argument map (host_rows), the device map (rows), a map that exists on the device only (the prioritized
    sample) and as a gathered copy (identity) the call gives the same bits, td_abs included; the two copies of the
    duplicated episode report one error."""
    from maleague import _native
    from maleague.components.replay_buffer import PrioritizedSampledEpisodeBatch, ReplayBuffer, SampledEpisodeBatch
    _env(pid, monkeypatch)
    pc, args, _, _, tb = PC.learner_inputs(pid)
    N, A, S, d_obs = LA.dims(pc.case)
    scheme, groups, pre = scheme_for({"state_shape": S, "obs_shape": d_obs, "n_actions": A, "n_agents": N}, torch)
    buf = ReplayBuffer(scheme, groups, LA.B + 3, LA.T_STORED, preprocess=pre, device=device)
    buf.insert_episode_batch(_episode_batch({k: v[:3] for k, v in tb.items()}, device))  # slots 0..2: other episodes
    buf.insert_episode_batch(_episode_batch(tb, device))
    for k, v in tb.items():  # the insert recomputes actions_onehot: restore the steps past the episodes' ends
        buf.data.transition_data[k][3:3 + LA.B].copy_(v)
    ids = 3 + np.asarray([2, 0, 2, 4, 1])
    w = torch.from_numpy(PC.is_weight(pid)).to(device)
    lib = _native.load(require_gpu=True)

    def view_host():
        v = SampledEpisodeBatch(buf, ids)
        v.is_weight = w
        return v

    def view_device():
        return PrioritizedSampledEpisodeBatch(buf, torch.from_numpy(ids.astype(np.int32)).to(device), w)

    def gathered():
        c = buf[ids]
        c.is_weight = w
        return c

    snaps = {}
    for tag, make in (("host_rows", view_host), ("rows", view_host), ("device rows", view_device), ("copy", gathered)):
        batch = make()
        learner = _build(pid, gathered())
        with monkeypatch.context() as m:
            if tag == "rows":
                m.setattr(lib, "mlg_qlearner_inline_rows", lambda: 0)
            out = []
            for ep in (0, 200):
                learner.train(batch, 0, ep)
                out.append(_snap(learner))
        if tag == "host_rows":
            assert batch._rows is None  # the slot map travelled as a kernel argument
        elif tag != "copy":
            assert batch._rows is not None and batch._data is None
        snaps[tag] = out
    for tag in ("host_rows", "rows", "device rows"):
        for call in range(2):
            _same(snaps[tag][call], snaps["copy"][call], f"{pid} {tag} call {call}", keys=("stats", "grads", "params", "sq", "td_abs"))
    td = snaps["copy"][0]["td_abs"]
    assert td[0] == td[2] and np.all(np.isfinite(td))


@pytest.mark.parametrize("pid", PC.LEARNER_IDS)
def test_two_calls_from_a_nan_workspace_give_the_same_bits(device, monkeypatch, pid):
    """(d) a NaN-filled workspace of exactly mlg_qlearner_workspace_floats(per = 1) floats: no kernel reads an element
    the call did not write, and two fresh learners agree bit for bit (the per-episode reduce has a fixed order)."""
    from maleague import _native
    _env(pid, monkeypatch)
    runs = []
    for _ in range(2):
        eb = _batch(pid, device, PC.is_weight(pid))
        learner = _build(pid, eb)
        need = _native.load().mlg_qlearner_workspace_floats(_native.byref(learner._cfg(eb.batch_size, eb.max_seq_length, per=True)))
        assert need > 0
        learner._ws = torch.empty(int(need), dtype=torch.float32, device=device)
        out = []
        for ep in (0, 200):
            learner._ws.fill_(float("nan"))
            learner.train(eb, 0, ep)
            assert learner._ws.numel() == need
            out.append(_snap(learner))
        runs.append(out)
    for call in range(2):
        for k in ("stats", "grads", "params", "sq", "td_abs"):
            assert np.all(np.isfinite(runs[0][call][k])), f"{pid} call {call}: {k} not finite"
        _same(runs[0][call], runs[1][call], f"{pid} call {call}", keys=("stats", "grads", "params", "sq", "td_abs"))
        assert np.array_equal(runs[0][call]["stats"], runs[1][call]["stats"])


def test_unrolled_distinct_branch_applies_the_weights(device, monkeypatch):
    """MLG_DISTINCT_LEARNER=unrolled with a weighted batch: the torch branch's loss, gradients and td_abs against the
    fused call's (the bound of the fused-against-unrolled test: the float64 oracle's, for both)."""
    pid = "distinct"
    g64, td64, s64 = PC.oracle_f64(pid)
    monkeypatch.setenv("MLG_DISTINCT_LEARNER", "unrolled")
    eb = _batch(pid, device, PC.is_weight(pid))
    learner = _build(pid, eb)
    learner.train(eb, 0, 0)
    got = _snap(learner)
    np.testing.assert_allclose(got["stats"][0], s64["loss"], rtol=LA.STAT_RTOL, atol=LA.STAT_ATOL)
    _close(got["td_abs"], td64.numpy(), "unrolled td_abs")
    coef = min(1.0, learner.args.grad_norm_clip / (float(got["stats"][1]) + 1e-6))
    grads = torch.from_numpy(got["grads"])
    for (q, off, k), ref in zip(learner._flat.views, g64):
        mine = grads[off:off + k].view_as(q).to(torch.float64) / coef
        assert float((mine - ref).abs().max()) <= LA.GRAD_RTOL * max(1.0, float(ref.abs().max()))


# ---- 4. end to end -----------------------------------------------------------------------------------------------------
def _experiment(tmp_path, cpu_buffer):
    from maleague.custom_logging import MainLogger
    from maleague.runs import MultiAgentExperiment
    from maleague.utils.config import build_config, to_args
    cfg = build_config("qmix", "ma", overrides=[
        "runner=parallel", "batch_size_run=64", "batch_size=32", f"buffer_cpu_only={cpu_buffer}", "buffer_size=160",
        "env_args.match_build_plan=small", "env_args.episode_limit=20", "seed=3", "prioritized_replay=True",
        "show_exp_parameters=False", "t_max=1000000", "test_interval=100000000", f"local_results_path={tmp_path}"])
    np.random.seed(0)
    torch.manual_seed(0)
    return MultiAgentExperiment(to_args(cfg), MainLogger(log_interval=10 ** 12))


def _three_iterations(exp):
    """-> per iteration (rows, priorities after the insert, priorities after the update, td_abs, maximum at insert)."""
    from maleague.components.replay_buffer import PrioritizedReplayBuffer
    buf = exp.home_buffer
    assert isinstance(buf, PrioritizedReplayBuffer) and buf.seed == 3
    exp._init_stepper()
    drawn = []
    sample = buf.sample
    buf.sample = lambda *a, **kw: drawn.append(sample(*a, **kw)) or drawn[-1]
    out = []
    for i in range(3):
        batch, info = exp.stepper.run(test_mode=False)
        slot0, max0 = buf.buffer_index, float(buf.max_priority)
        buf.insert_episode_batch(batch)
        after_insert = buf.priorities.cpu().numpy().copy()
        new = (slot0 + np.arange(64)) % 160
        assert np.all(after_insert[new] == np.float32(max0)), f"iteration {i}: new slots hold the maximum"
        exp._train_home(i * 64)
        s = drawn[-1]
        out.append({"rows": s.rows.cpu().numpy().astype(np.int64), "w": s.is_weight.cpu().numpy(),
                    "after_insert": after_insert, "after_update": buf.priorities.cpu().numpy().copy(),
                    "td_abs": exp.home_learner.last_td_abs.cpu().numpy().copy(), "live": buf.episodes_in_buffer,
                    "max": float(buf.max_priority)})
    assert len(drawn) == 3 and exp.home_learner.train_calls == 3
    exp.stepper.close_env()
    return out


def test_experiment_end_to_end(device, tmp_path):
    """Three iterations of MultiAgentExperiment on the `small` plan, 64 envs into a 160-slot device ring (the third
    rollout wraps), prioritized_replay on: after each train the sampled slots hold (td_abs + e)^a, every other slot is
    unchanged, new slots took the maximum; the same run with a host buffer draws the same rows."""
    from maleague.components.replay_buffer import PrioritizedSampledEpisodeBatch
    exp = _experiment(tmp_path / "dev", False)
    assert str(exp.home_buffer.device) == str(exp.args.device)
    dev = _three_iterations(exp)
    assert [d["live"] for d in dev] == [64, 128, 160]
    for i, d in enumerate(dev):
        rows = d["rows"]
        assert rows.shape == (32,) and rows.min() >= 0 and rows.max() < d["live"]
        assert np.all(np.isfinite(d["td_abs"])) and d["td_abs"].max() > 0 and d["w"].max() == 1.0
        _close(d["after_update"][rows], PR.priority(d["td_abs"]), f"iteration {i} sampled slots")
        rest = np.setdiff1d(np.arange(160), rows)
        assert np.array_equal(d["after_update"][rest], d["after_insert"][rest]), f"iteration {i}: untouched slots"
        assert d["max"] == max(1.0, max(x["after_update"].max() for x in dev[:i + 1]))
    assert np.all(dev[0]["w"] == 1.0)  # flat priorities at the first draw
    assert len(np.unique(dev[2]["w"])) > 1  # then the weights differ
    host = _three_iterations(_experiment(tmp_path / "host", True))
    for i, (d, h) in enumerate(zip(dev, host)):
        assert np.array_equal(d["rows"], h["rows"]), f"iteration {i}: host buffer drew other rows"
        _close(h["w"], d["w"], f"iteration {i} weights")
        _close(h["after_update"], d["after_update"], f"iteration {i} priorities")
    assert PrioritizedSampledEpisodeBatch.device_rows_only
