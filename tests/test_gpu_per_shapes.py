"""GPU parity of prioritized episode replay off the fixture shapes of tests/test_gpu_per.py: the cases,
seeds and measured figures are tests/per_shapes.py's, the conditions they rest on tests/test_per_shapes.py's (CPU).

  1. mlg_per_sample at the scan's chunk carry (1024 / 1025 live slots), at the LDS-to-workspace switch (6144 / 6145), at
     the maximum 2^20, with draw passes q = 1..3 (1025 / 4096 draws), priorities of exactly 0, beta 0 and 1
  2. mlg_per_insert / mlg_per_update past one pass of their 256 threads, count == ring_size, slots outside the buffer
  3. the learner with per = 1 on every dispatch arm of the three arm tables
  4. per_reduce_kernel along time (64 / 65 / 129 / 99 transitions) and batch (1 / 72 episodes), a mask with a hole, the
     workload's stored length 101 read in place
  5. the self-play home learner end to end

Bounds. Rows and everything called bit-identical: exact. Weights, priorities and td_abs: the project's op bound
1e-4 max(1, max|ref|) against float64. Gradients per tensor 1e-4 max(1, max|g_ref|) and statistics rtol 2e-4 / atol 1e-6
against the float64 weighted oracle (per_shapes.bounds: ten times the fp32 oracle's own distance from float64 would
replace a bound where larger; it is nowhere). Every comparison prints its error as a share of its bound
(profiles/per/README.md records them).
"""
import numpy as np
import pytest
import torch

import learner_arm_shapes as LA
import per_cases as PC
import per_ref as PR
import per_shapes as PS
from helpers import scheme_for
from test_gpu_learner_shapes import _episode_batch, _learner
from test_gpu_per import OP_TOL, SENTINEL, _close, _prio_state, _same, _snap

pytestmark = pytest.mark.gpu

ALL_KEYS = ("stats", "grads", "params", "sq", "td_abs")


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    for k in ("MLG_MIX_GENERIC", "MLG_LEARNER_FULL", "MLG_DISTINCT_LEARNER"):
        monkeypatch.delenv(k, raising=False)


# ---- 1. mlg_per_sample -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", PS.SAMPLE_IDS)
def test_per_sample_edges_vs_oracle(device, sid):
    from maleague import _native
    lib = _native.load(require_gpu=True)
    p, n, B, seed, draw, beta = PS.sample_case(sid)
    want_rows, want_w, margin = PR.sample(p, n, B, seed, draw, beta)
    assert margin > PC.NEAR_TIE
    prio = torch.from_numpy(p).to(device)
    rows = torch.full((B + 2,), -5, dtype=torch.int32, device=device)  # a guard element on either side
    w = torch.full((B + 2,), SENTINEL, dtype=torch.float32, device=device)
    ws = torch.full((n,), float("nan"), dtype=torch.float64, device=device) if n > lib.mlg_per_lds_slots() else None
    assert (ws is None) == (n <= 6144)
    _native.call("mlg_per_sample", prio.data_ptr(), n, B, seed, draw, beta, rows[1:].data_ptr(), w[1:].data_ptr(),
                 None if ws is None else ws.data_ptr(), 0 if ws is None else n, _native.stream_ptr(device))
    torch.cuda.synchronize()
    assert rows[0] == -5 and rows[-1] == -5 and w[0] == SENTINEL and w[-1] == SENTINEL
    got_rows, got_w = rows[1:-1].cpu().numpy().astype(np.int64), w[1:-1].cpu().numpy()
    differ = np.flatnonzero(got_rows != want_rows)
    assert differ.size == 0, f"{sid}: {differ.size} rows differ, first at draw {differ[:4]}: {got_rows[differ[:4]]} " \
                             f"for {want_rows[differ[:4]]}"
    worst = _close(got_w, want_w, f"{sid} is_weight")
    assert torch.equal(prio.cpu(), torch.from_numpy(p))
    if ws is not None:  # the scan went through the workspace: every element written, the last one the total
        scan = ws.cpu().numpy()
        assert np.all(np.isfinite(scan))
        total = float(np.asarray(p, dtype=np.float64).sum())
        assert abs(scan[-1] - total) <= 1e-12 * total
    if sid.startswith("zeros"):
        assert np.all(p[got_rows] != 0) and np.all(np.isfinite(got_w))
    if beta == 0.0:
        assert np.all(got_w == 1.0)
    print(f"  {sid}: margin {margin:.2e}, is_weight error / bound {100 * worst:.3f} %")


# ---- 2. mlg_per_insert / mlg_per_update ------------------------------------------------------------------------------
# (ring, slot0, count): count == ring_size from the last slot; a wrap in the middle that leaves one slot; 257 slots (one
# thread's second pass) across the end; from the last slot of an odd ring
INSERTS = [(600, 599, 600), (601, 300, 600), (600, 500, 257), (601, 600, 257)]


def _insert(device, prio, mx, ring, slot0, count, errors):
    from maleague import _native
    _native.call("mlg_per_insert", prio.data_ptr(), ring, slot0, count, None if errors is None else errors.data_ptr(),
                 PR.E, PR.A, mx.data_ptr(), _native.stream_ptr(device))
    torch.cuda.synchronize()
    return prio.cpu().numpy(), float(mx)


@pytest.mark.parametrize("ring,slot0,count", INSERTS)
def test_per_insert_past_one_pass(device, ring, slot0, count):
    named = (slot0 + np.arange(count)) % ring
    rest = np.setdiff1d(np.arange(ring), named)
    assert len(np.unique(named)) == count and len(rest) == ring - count and named.min() == 0 and named.max() == ring - 1
    # the maximum
    prio, mx = _prio_state(device, ring, 2.5)
    got, m = _insert(device, prio, mx, ring, slot0, count, None)
    assert np.all(got[named] == np.float32(2.5)) and np.all(got[rest] == np.float32(SENTINEL)) and m == 2.5
    # errors: the largest at an index a thread reaches in its second pass or later, zeros and a negative among them
    rs = np.random.RandomState(ring + count)
    err = rs.uniform(0.0, 3.0, size=count).astype(np.float32)
    big = 256 + (count - 257) // 2
    err[big], err[3], err[200], err[7] = 40.0, 0.0, 0.0, -2.0
    assert 256 <= big < count and int(np.argmax(np.abs(err))) == big
    e = torch.from_numpy(err).to(device)
    prio, mx = _prio_state(device, ring, 2.5)
    got, m = _insert(device, prio, mx, ring, slot0, count, e)
    ref = np.full(ring, SENTINEL, dtype=np.float64)
    new_max = PR.insert(ref, 2.5, slot0, count, err)
    worst = _close(got[named], ref[named], "insert priorities")
    assert got[named[3]] == got[named[200]] == np.float32(PR.E ** PR.A)
    assert np.all(got[rest] == np.float32(SENTINEL))
    assert m == got[named].max() == got[named[big]] > 2.5 and abs(m - new_max) <= OP_TOL * new_max
    # an insert that does not reach the maximum leaves it
    prio, mx = _prio_state(device, ring, 50.0)
    got, m = _insert(device, prio, mx, ring, slot0, count, e)
    assert m == 50.0 and got[named].max() < 50.0
    print(f"  insert ring {ring} slot0 {slot0} count {count}: priority error / bound {100 * worst:.3f} %")


def _update(device, prio, mx, n, rows, td):
    from maleague import _native
    r = None if rows is None else torch.from_numpy(rows).to(device)
    t = torch.from_numpy(td).to(device)
    _native.call("mlg_per_update", prio.data_ptr(), n, None if r is None else r.data_ptr(), t.data_ptr(), len(td), PR.E,
                 PR.A, mx.data_ptr(), _native.stream_ptr(device))
    torch.cuda.synchronize()
    return prio.cpu().numpy(), float(mx)


@pytest.mark.parametrize("B", [300, 1025])
def test_per_update_past_one_pass_with_rows_outside_the_buffer(device, B):
    """Duplicated slots, the largest valid error past index 256, and rows at -1, n_slots and n_slots + 5 whose errors
    are the largest of the call: they write nothing and do not raise the maximum."""
    n = 700
    rs = np.random.RandomState(B)
    rows = rs.randint(0, n, size=B).astype(np.int32)
    rows[5], rows[B - 1] = rows[2], rows[0]  # duplicates whatever the draw
    per_slot = rs.uniform(0.0, 2.0, size=n).astype(np.float32)
    big = B - 3
    per_slot[rows[big]] = 30.0
    td = per_slot[rows]  # duplicated slots carry one error
    bad = {1: -1, 100: n, 257: n + 5, 299: -1, B - 2: n}
    for i, r in bad.items():
        rows[i], td[i] = r, 1000.0
    valid = (rows >= 0) & (rows < n)
    assert big > 256 and valid[big] and int(valid.sum()) == B - len(bad) and len(np.unique(rows[valid])) < valid.sum()
    prio, mx = _prio_state(device, n, 1.0)
    got, m = _update(device, prio, mx, n, rows, td)
    ref = np.full(n, SENTINEL, dtype=np.float64)
    new_max = PR.update(ref, 1.0, rows[valid], td[valid])
    named = np.unique(rows[valid])
    rest = np.setdiff1d(np.arange(n), named)
    worst = _close(got[named], ref[named], "update priorities")
    assert np.all(got[rest] == np.float32(SENTINEL)) and len(rest) > 0
    assert m == got[named].max() == got[rows[big]] and abs(m - new_max) <= OP_TOL * new_max
    assert 1.0 < m < float(PR.priority(1000.0))
    # the rows outside alone: nothing written, the maximum stays
    prio, mx = _prio_state(device, n, 1.0)
    outside = np.asarray([-1, n, n + 5] * 100, np.int32)
    got, m = _update(device, prio, mx, n, outside, np.full(300, 1000.0, np.float32))
    assert np.all(got == np.float32(SENTINEL)) and m == 1.0
    print(f"  update B {B}: priority error / bound {100 * worst:.3f} %")


@pytest.mark.parametrize("B", [300, 1025])
def test_per_update_identity_rows_over_the_whole_buffer(device, B):
    rs = np.random.RandomState(40 + B)
    td = rs.uniform(0.0, 2.0, size=B).astype(np.float32)
    td[B - 2], td[0] = 25.0, 0.0
    prio, mx = _prio_state(device, B, 1.0)
    got, m = _update(device, prio, mx, B, None, td)  # B == n_slots
    want = PR.priority(td)
    worst = _close(got, want, "identity update")
    assert got[0] == np.float32(PR.E ** PR.A) and m == got.max() == got[B - 2] > 1.0
    assert abs(m - float(want.max())) <= OP_TOL * float(want.max())
    print(f"  identity update B {B}: priority error / bound {100 * worst:.3f} %")


# ---- 3. the learner with per = 1 on every dispatch arm ---------------------------------------------------------------
def _build(kind, eb, args, agent0, mixer0):
    if kind == "distinct":
        from test_gpu_distinct_learner_fused import _distinct_learner
        return _distinct_learner(eb, args, agent0, mixer0)[0]
    return _learner(eb, agent0, mixer0, args)[0]


def _weighted(tb, device, w):
    eb = _episode_batch(tb, device)
    if w is not None:
        eb.is_weight = torch.as_tensor(w)
    return eb


def _check_first_call(key, learner, got, oracle, mask):
    """A first call's gradients (scaled back by the clip factor), td_abs and statistics against the float64 weighted
    oracle within per_shapes.bounds(key); an episode without a masked step reports exactly 0.
    -> (gradient, td_abs) error / bound."""
    g64, td64, s64 = oracle
    stat_rtol, grad_rtol, td_tol = PS.bounds(key)
    norm = float(got["stats"][1])
    np.testing.assert_allclose(norm, s64["grad_norm"], rtol=stat_rtol, err_msg=f"{key} grad_norm")
    coef = min(1.0, learner.args.grad_norm_clip / (norm + 1e-6))  # clip_grad_norm_
    views = learner._flat.views
    assert len(views) == len(g64)
    grads = torch.from_numpy(got["grads"])
    worst = 0.0
    for (q, off, k), ref in zip(views, g64):
        assert tuple(q.shape) == tuple(ref.shape)
        mine = grads[off:off + k].view_as(q).to(torch.float64) / coef
        err, scale = float((mine - ref).abs().max()), max(1.0, float(ref.abs().max()))
        worst = max(worst, err / (grad_rtol * scale))
        assert err <= grad_rtol * scale, f"{key} tensor at {off} {tuple(q.shape)}: {err:.3e} > {grad_rtol * scale:.3e}"
    td_ref = td64.numpy()
    assert got["td_abs"].shape == td_ref.shape
    td_err = float(np.abs(got["td_abs"].astype(np.float64) - td_ref).max())
    td_bound = td_tol * max(1.0, float(np.abs(td_ref).max()))
    assert td_err <= td_bound, f"{key} td_abs: max error {td_err:.3e} > {td_bound:.3e}"
    for i, k in ((0, "loss"), (2, "td_error_abs"), (3, "q_taken_mean"), (4, "target_mean")):
        np.testing.assert_allclose(got["stats"][i], s64[k], rtol=stat_rtol, atol=LA.STAT_ATOL, err_msg=f"{key} {k}")
    steps = mask.sum(axis=1)
    div = learner.args.n_agents if learner.args.mixer is None else 1  # IQL expands the mask over the agents
    assert float(got["stats"][5]) == float(steps.sum()) * div
    assert np.all(got["td_abs"][steps == 0] == 0.0) and np.all(td_ref[steps == 0] == 0.0)
    assert np.all(got["td_abs"][steps > 0] > 0.0)
    return worst, td_err / td_bound


@pytest.mark.parametrize("aid", PS.ARM_IDS)
def test_arm_weighted_gradients_and_errors_vs_float64_oracle(device, aid):
    from maleague import _native
    kind, c, args, agent0, mixer0, tb = PS.arm_inputs(aid)
    eb = _weighted(tb, device, PS.arm_weight(aid))
    learner = _build(kind, eb, args, agent0, mixer0)
    assert _native.qlearner_describe(learner._cfg(eb.batch_size, LA.T_FILLED, per=1)) == c.arm + " + per"
    learner.train(eb, 0, 0)
    got = _snap(learner)
    wg, wt = _check_first_call(aid, learner, got, PS.arm_oracle_f64(aid), PS.reduce_mask(tb))
    print(f"  {aid}: grad_norm {got['stats'][1]:.6g}, gradient error / bound {100 * wg:.2f} %, "
          f"td_abs error / bound {100 * wt:.3f} %")


@pytest.mark.parametrize("aid", PS.ARM_IDS)
def test_arm_unit_weights_are_the_unweighted_call(device, aid):
    """is_weight = 1 everywhere: parameters, gradients, RMSprop state and statistics bit-identical to the per = 0 call
    over two calls (target a copy, then stale); td_abs averages to the call's td_error_abs."""
    from maleague import _native
    kind, c, args, agent0, mixer0, tb = PS.arm_inputs(aid)
    B = int(tb["filled"].shape[0])
    plain_b, per_b = _weighted(tb, device, None), _weighted(tb, device, np.ones(B, np.float32))
    plain, per = _build(kind, plain_b, args, agent0, mixer0), _build(kind, per_b, args, agent0, mixer0)
    assert _native.qlearner_describe(plain._cfg(B, LA.T_FILLED, per=0)) == c.arm
    assert _native.qlearner_describe(per._cfg(B, LA.T_FILLED, per=1)) == c.arm + " + per"
    steps = PS.reduce_mask(tb).sum(axis=1)
    for call, ep in enumerate([0, 200]):
        plain.train(plain_b, 0, ep)
        per.train(per_b, 0, ep)
        a, b = _snap(plain), _snap(per)
        _same(a, b, f"{aid} call {call}")
        assert plain.last_td_abs is None and b["td_abs"].shape == (B,) and np.all(np.isfinite(b["td_abs"]))
        mean = float((b["td_abs"].astype(np.float64) * steps).sum() / steps.sum())
        np.testing.assert_allclose(mean, b["stats"][2], rtol=2e-4)
        assert np.all(b["td_abs"][steps == 0] == 0.0)


# ---- 4. the time and batch axes of the per-episode reduce ------------------------------------------------------------
def _reduce_batches(rid, device):
    """-> (the batch the learner trains on, a gathered copy of it): the same EpisodeBatch for the plain cases; for a
    case with a slot map the episodes sit in a device ReplayBuffer behind two other episodes and are read in place
    through a PrioritizedSampledEpisodeBatch."""
    from maleague.components.replay_buffer import PrioritizedSampledEpisodeBatch, ReplayBuffer
    rc, _, c, _, _, _, stored, tb = PS.reduce_inputs(rid)
    w = torch.from_numpy(PS.reduce_weight(rid)).to(device)
    if rc.rows is None:
        eb = _episode_batch(tb, device)
        eb.is_weight = w
        return eb, eb
    N, A, S, d_obs = LA.dims(c)
    scheme, groups, pre = scheme_for({"state_shape": S, "obs_shape": d_obs, "n_actions": A, "n_agents": N}, torch)
    buf = ReplayBuffer(scheme, groups, rc.B + 2, rc.T, preprocess=pre, device=device)
    buf.insert_episode_batch(_episode_batch({k: v[:2] for k, v in stored.items()}, device))  # slots 0, 1: other episodes
    buf.insert_episode_batch(_episode_batch(stored, device))
    for k, v in stored.items():  # the insert recomputes actions_onehot: restore the steps past the episodes' ends
        buf.data.transition_data[k][2:2 + rc.B].copy_(v)
    ids = 2 + np.asarray(rc.rows)
    view = PrioritizedSampledEpisodeBatch(buf, torch.from_numpy(ids.astype(np.int32)).to(device), w)
    assert view.max_seq_length == rc.T and view.host_rows is None
    copy = buf[ids]
    copy.is_weight = w
    for k, v in tb.items():
        assert torch.equal(copy.data.transition_data[k].cpu(), v), k
    return view, copy


def _reduce_learner(rid, copy):
    _, _, _, args, agent0, mixer0, _, _ = PS.reduce_inputs(rid)
    return _learner(copy, agent0, mixer0, args)[0]


def _exact_workspace(learner, batch, device):
    from maleague import _native
    need = _native.load().mlg_qlearner_workspace_floats(
        _native.byref(learner._cfg(batch.batch_size, batch.max_seq_length, per=True)))
    assert need > 0
    learner._ws = torch.empty(int(need), dtype=torch.float32, device=device)
    return int(need)


def _two_calls(rid, device, batch_of=lambda view, copy: view, nan_ws=False):
    view, copy = _reduce_batches(rid, device)
    batch = batch_of(view, copy)
    learner = _reduce_learner(rid, copy)
    need = _exact_workspace(learner, batch, device) if nan_ws else None
    out = []
    for ep in (0, 200):  # target a copy, then stale
        if nan_ws:
            learner._ws.fill_(float("nan"))
        learner.train(batch, 0, ep)
        assert need is None or learner._ws.numel() == need
        out.append(_snap(learner))
    return out


@pytest.mark.parametrize("rid", PS.REDUCE_IDS)
def test_reduce_first_call_vs_float64_oracle(device, rid):
    from maleague import _native
    rc, _, c, _, _, _, _, tb = PS.reduce_inputs(rid)
    view, copy = _reduce_batches(rid, device)
    learner = _reduce_learner(rid, copy)
    assert view.max_seq_length == rc.T and int(copy.max_t_filled()) == max(rc.lens)
    assert _native.qlearner_describe(learner._cfg(view.batch_size, view.max_seq_length, per=1)) == c.arm + " + per"
    learner.train(view, 0, 0)
    got = _snap(learner)
    mask = PS.reduce_mask(tb)
    wg, wt = _check_first_call(rid, learner, got, PS.reduce_oracle_f64(rid), mask)
    if rc.rows is not None:  # the two copies of the duplicated episode report one error
        first, second = (i for i, r in enumerate(rc.rows) if r == rc.rows[0])
        assert got["td_abs"][first] == got["td_abs"][second]
    print(f"  {rid}: grad_norm {got['stats'][1]:.6g}, gradient error / bound {100 * wg:.2f} %, "
          f"td_abs error / bound {100 * wt:.3f} %, longest episode {int(mask.sum(axis=1).max())} masked steps")


@pytest.mark.parametrize("rid", PS.REDUCE_IDS)
def test_reduce_two_calls_from_a_nan_workspace_give_the_same_bits(device, rid):
    """A NaN-filled workspace of exactly mlg_qlearner_workspace_floats(per = 1) floats: no kernel reads an element the
    call did not write (tdrow past an episode's live rows among them), and two fresh learners agree bit for bit."""
    runs = [_two_calls(rid, device, nan_ws=True) for _ in range(2)]
    for call in range(2):
        for k in ALL_KEYS:
            assert np.all(np.isfinite(runs[0][call][k])), f"{rid} call {call}: {k} not finite"
        _same(runs[0][call], runs[1][call], f"{rid} call {call}", keys=ALL_KEYS)
        assert np.array_equal(runs[0][call]["stats"], runs[1][call]["stats"])


@pytest.mark.parametrize("rid", PS.REDUCE_IDS)
def test_reduce_full_path_equals_default_path(device, monkeypatch, rid):
    """MLG_LEARNER_FULL=1 (mlen = t_eff - 1 everywhere: the reduce then reads every row up to the batch's length)
    against the default path under ==, td_abs included."""
    got = _two_calls(rid, device)
    monkeypatch.setenv("MLG_LEARNER_FULL", "1")
    want = _two_calls(rid, device)
    monkeypatch.delenv("MLG_LEARNER_FULL")
    for call in range(2):
        for k in ALL_KEYS:
            assert np.all(np.isfinite(got[call][k])), f"{rid} call {call}: {k} not finite"
        _same(got[call], want[call], f"{rid} call {call}", keys=ALL_KEYS)
    assert got[0]["stats"][7] <= want[0]["stats"][7]  # the default path planned no more forward blocks


@pytest.mark.parametrize("rid", ["view101-qmix", "view101-iql"])
def test_reduce_view_equals_gathered_copy(device, rid):
    """The stored length 101 read in place through the device slot map against the gathered copy of the same rows."""
    view = _two_calls(rid, device)
    copy = _two_calls(rid, device, batch_of=lambda view, copy: copy)
    for call in range(2):
        _same(view[call], copy[call], f"{rid} call {call}", keys=ALL_KEYS)


# ---- 5. the self-play home learner -----------------------------------------------------------------------------------
def test_selfplay_home_learner_end_to_end(device, tmp_path):
    """Three iterations of SelfPlayMultiAgentExperiment (QMIX, the `small` plan on both sides, episode_limit 20, 64 envs
    into a 160-slot device ring: the third rollout wraps) with prioritized_replay on: the home buffer is prioritized,
    after each train the sampled slots hold (td_abs + e)^a, every other slot is unchanged, new slots took the maximum;
    no other buffer of the experiment is prioritized."""
    from maleague.components.replay_buffer import PrioritizedReplayBuffer, ReplayBuffer
    from maleague.custom_logging import MainLogger
    from maleague.envs.plans import builtin_plan
    from maleague.runs import SelfPlayMultiAgentExperiment
    from maleague.utils.config import build_config, to_args
    cfg = build_config("qmix", "ma", overrides=[
        "runner=parallel", "batch_size_run=64", "batch_size=32", "buffer_cpu_only=False", "buffer_size=160",
        "env_args.episode_limit=20", "seed=3", "prioritized_replay=True", "show_exp_parameters=False",
        "t_max=1000000", "test_interval=100000000", f"local_results_path={tmp_path}"])
    cfg["env_args"]["match_build_plan"] = builtin_plan("small", self_play=True)
    np.random.seed(0)
    torch.manual_seed(0)
    exp = SelfPlayMultiAgentExperiment(to_args(cfg), MainLogger(log_interval=10 ** 12))
    buf = exp.home_buffer
    assert isinstance(buf, PrioritizedReplayBuffer) and buf.seed == 3 and str(buf.device) == str(exp.args.device)
    assert exp.args.n_agents == 3 and exp.args.total_n_agents == 6
    away0 = {k: v.clone() for k, v in exp.away_mac.agent.state_dict().items()}
    exp._init_stepper()
    drawn = []
    sample = buf.sample
    buf.sample = lambda *a, **kw: drawn.append(sample(*a, **kw)) or drawn[-1]
    out = []
    for i in range(3):
        home_batch, away_batch, _ = exp.stepper.run(test_mode=False)
        slot0, max0 = buf.buffer_index, float(buf.max_priority)
        buf.insert_episode_batch(home_batch)
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
    assert [d["live"] for d in out] == [64, 128, 160]
    for i, d in enumerate(out):
        rows = d["rows"]
        assert rows.shape == (32,) and rows.min() >= 0 and rows.max() < d["live"]
        assert np.all(np.isfinite(d["td_abs"])) and d["td_abs"].max() > 0 and d["w"].max() == 1.0
        _close(d["after_update"][rows], PR.priority(d["td_abs"]), f"iteration {i} sampled slots")
        rest = np.setdiff1d(np.arange(160), rows)
        assert np.array_equal(d["after_update"][rest], d["after_insert"][rest]), f"iteration {i}: untouched slots"
        assert d["max"] == max(1.0, max(x["after_update"].max() for x in out[:i + 1]))
    assert np.all(out[0]["w"] == 1.0)  # flat priorities at the first draw
    assert len(np.unique(out[2]["w"])) > 1  # then the weights differ
    # the away side: frozen, and no buffer of it (or of the stepper) is prioritized
    for k, v in exp.away_mac.agent.state_dict().items():
        assert torch.equal(v, away0[k]), k
    others = [v for holder in (exp, exp.stepper) for v in vars(holder).values()
              if isinstance(v, ReplayBuffer) and v is not buf]
    assert not any(isinstance(v, PrioritizedReplayBuffer) for v in others)
    assert not isinstance(away_batch, PrioritizedReplayBuffer) and not hasattr(away_batch, "is_weight")
    exp.stepper.close_env()
