"""GPU parity of the REFIL learner (mlg_refil_train) off the refil_8 shape: the cases of tests/refil_learner_shapes.py,
one per branch of csrc/refil_learner.hip the other REFIL learner suites do not reach (NA 1 to 8, NE 1 to 16, entity
input widths 8 to 48 with and without the last-action columns, one and two action waves, the mask scan by episode count
and by length, mix_len on either side of the live-bit words, a clipped gradient, the plain agent with FlexQMixer and
VDN). tests/test_refil_learner_shapes.py checks the table's own conditions on the CPU.

Yardsticks. Three-call trajectories (episode_num 0 / 100 / 200: the target equals the online network, is stale, is
stale and the call ends with the target sync): the fp32 CPU oracle, statistics rtol 2e-4 / atol 1e-5 and parameters
atol 2e-5, this learner's bounds in tests/test_gpu_refil_learner.py. First-call gradients: the float64 oracle before
its clip, per tensor max|g - g64| <= max(1e-4 max|g64|, 10 d32) with d32 the fp32 oracle's own distance from float64 on
that tensor (refil_learner_shapes.GRAD_D32). The first RMSprop step moves every weight by about 10 lr whatever the
gradient's size, so the parameter bound alone checks little more than signs; max|g| per tensor runs from 3e-4 to 1e-1
here, so the bound is relative to the tensor's own scale. Each bound would be ten times the fp32 oracle's distance
from float64 (refil_learner_shapes.ORACLE_F64) where that were larger: it is not for any statistic or parameter, and
the 10 d32 term governs no gradient tensor (d32 / max|g64| <= 1.8e-6).

Everything here rests on the CPU oracle; no timing is taken.
"""
import functools

import numpy as np
import pytest
import torch

import refil_learner_shapes as RS
from helpers import entity_scheme_for
from test_gpu_refil_learner import _batch_from, _learner

pytestmark = pytest.mark.gpu

STAT_KEYS = ["loss", "im_loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean"]


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = RS.case(cid)
    arrs = RS.case_arrays(c)
    agent_p, mixer_p = RS.case_weights(c)
    return c, arrs, agent_p, mixer_p, RS.case_groups(c)


@functools.lru_cache(maxsize=None)
def _oracle32(cid):
    """Computed once per case: the fp32 oracle's three calls (statistics per call, the oracle after them)."""
    stats, ref, _, _ = RS.run_oracle(RS.case(cid), torch.float32, arrs=_inputs(cid)[1])
    return stats, ref


@functools.lru_cache(maxsize=None)
def _oracle64(cid):
    """The float64 oracle's first call: its statistics and its gradients before the clip, in flat parameter order."""
    stats, ref, grads, _ = RS.run_oracle(RS.case(cid), torch.float64, calls=RS.CALLS[:1], arrs=_inputs(cid)[1])
    return stats[0], grads, list(ref.agent) + list(ref.mixer)


def _set_env(monkeypatch, c, one_stream=False):
    monkeypatch.delenv("MLG_REFIL_GENERIC", raising=False)
    monkeypatch.delenv("MLG_REFIL_ONE_STREAM", raising=False)
    for k, v in RS.case_env(c).items():
        monkeypatch.setenv(k, v)
    if one_stream:
        monkeypatch.setenv("MLG_REFIL_ONE_STREAM", "1")


def _fresh(cid, device, eb=None):
    c, arrs, agent_p, mixer_p, _ = _inputs(cid)
    if eb is None:
        eb = _batch_from(arrs, device, NE=c.NE, ED=c.ED, NA=c.NA, A=c.A)
    learner, log = _learner(eb, agent_p, mixer_p, RS.case_args(c))
    assert eb.batch_size == c.B and eb.max_seq_length == c.T and int(eb.max_t_filled()) == RS.t_filled(arrs) < c.T
    return learner, eb, log


def _run(cid, device, workspace="zero"):
    """A fresh learner's three calls. ``workspace``: "zero" -- zeroed once, as train() allocates it; "garbage" --
    filled with seeded uniform +-1e3 values before every call (finite: padded rows are multiplied by exact zeros,
    which a NaN would turn into a false alarm and stale finite data would not)."""
    from maleague import _native
    c, arrs, _, _, groups = _inputs(cid)
    learner, eb, log = _fresh(cid, device)
    need = _native.load(require_gpu=True).mlg_refil_workspace_floats(_native.byref(learner._cfg(c.B, c.T)))
    assert need > 0
    learner._ws = torch.zeros(int(need * 1.1) + 1024, dtype=torch.float32, device=device)  # train()'s own size
    gen = torch.Generator(device=device).manual_seed(1234 + c.seed)
    out = {"calls": [], "learner": learner, "log": log}
    for i, ep in enumerate(RS.CALLS):
        if workspace == "garbage":
            learner._ws.uniform_(-1e3, 1e3, generator=gen)
        ws = learner._ws
        learner.train(eb, 0, episode_num=ep, groupA=None if groups[i] is None else groups[i].to(device))
        torch.cuda.synchronize()
        assert learner._ws is ws  # the workspace prepared above is the one the call used
        out["calls"].append({"stats": learner._stats.cpu().numpy().copy(), "named": dict(learner.last_stats),
                             "grads": learner._grads.cpu().clone(), "params": learner._flat.flat.cpu().clone(),
                             "sq": learner._sq.cpu().clone()})
    out["target_is_online"] = bool(torch.equal(learner._flat.flat, learner._tflat.flat))
    return out


_RUNS = {}


def _shared_run(cid, device, monkeypatch):
    """The case's default run (zeroed workspace, side stream), shared by the tests below."""
    if cid not in _RUNS:
        _set_env(monkeypatch, RS.case(cid))
        _RUNS[cid] = _run(cid, device)
    return _RUNS[cid]


def _assert_bitwise(a, b, tag):
    for i, (x, y) in enumerate(zip(a["calls"], b["calls"])):
        assert np.array_equal(x["stats"], y["stats"]), f"{tag} call {i}: stats {x['stats']} vs {y['stats']}"
        for k in ("grads", "params", "sq"):
            assert bool(torch.isfinite(x[k]).all()) and bool(torch.isfinite(y[k]).all()), f"{tag} call {i}: {k}"
            assert torch.equal(x[k], y[k]), \
                f"{tag} call {i}: {k} differ at {torch.nonzero(x[k] != y[k]).flatten()[:8].tolist()}"


# ---- a. three-call trajectory against the fp32 oracle ----------------------------------------------------------------
@pytest.mark.parametrize("cid", RS.IDS)
def test_three_call_trajectory_vs_oracle(device, monkeypatch, cid):
    """No case needed a bound widened by the fp32 oracle's own distance from float64 (RS.bounds)."""
    c, arrs, _, _, _ = _inputs(cid)
    want, ref = _oracle32(cid)
    got = _shared_run(cid, device, monkeypatch)
    learner = got["learner"]
    rtol, atol, patol = RS.bounds(cid)
    assert (rtol, atol, patol) == (RS.STAT_RTOL, RS.STAT_ATOL, RS.PARAM_ATOL)
    keys = [k for k in STAT_KEYS if k != "im_loss" or c.agent == RS.IMAGINE]  # im_loss exactly for the imagine agent
    for i in range(len(RS.CALLS)):
        named = got["calls"][i]["named"]
        assert set(named) == set(want[i]) == set(keys), f"{cid} call {i}"
        print(f"  {cid} call {i}: " + ", ".join(f"{k} {named[k]:.7g}/{want[i][k]:.7g}" for k in keys))
    assert set(got["log"].stats) == set(keys)
    for i in range(len(RS.CALLS)):
        for k in keys:
            v = got["calls"][i]["named"][k]
            assert np.isfinite(v), f"{cid} call {i} {k}"
            np.testing.assert_allclose(v, want[i][k], rtol=rtol, atol=atol, err_msg=f"{cid} call {i} {k}")
    assert learner.last_target_update_episode == ref.last_target_update_episode == 200
    assert got["target_is_online"]  # the third call ended with the sync: bit-identical on the device
    pairs = [("agent", dict(learner.mac.agent.named_parameters()), ref.agent),
             ("target agent", dict(learner.target_mac.agent.named_parameters()), ref.t_agent),
             ("mixer", dict(learner.mixer.named_parameters()), ref.mixer),
             ("target mixer", dict(learner.target_mixer.named_parameters()), ref.t_mixer)]
    errs = {}
    for name, g, w in pairs:
        assert list(g) == list(w), name
        for k, v in g.items():
            errs[f"{name} {k}"] = float(np.abs(v.detach().cpu().numpy() - w[k].detach().numpy()).max())
    assert len(errs) == (26 if c.mixer == "vdn" else 82)
    worst = max(errs, key=errs.get)
    print(f"  {cid}: max parameter error {errs[worst]:.3e} at {worst} (bound {patol:.1e})")
    for k, e in errs.items():
        assert e <= patol, f"{cid} {k}: {e:.3e} > {patol:.1e}"
    n = RS.mask_sum(arrs)
    assert all(float(call["stats"][6]) == n for call in got["calls"])
    assert learner.mac.agent.trained_steps == len(RS.CALLS) * int(n) and learner.train_calls == len(RS.CALLS)


# ---- b. first-call gradients against the float64 oracle --------------------------------------------------------------
@pytest.mark.parametrize("cid", RS.IDS)
def test_first_call_gradients_vs_float64_oracle(device, monkeypatch, cid):
    """learner._grads after the first call, scaled back by the clip factor clip_grad_norm_ applied (from the call's
    own grad_norm), per tensor of the flat vector against the float64 oracle's .grad before its clip."""
    c = RS.case(cid)
    s64, g64, names = _oracle64(cid)
    got = _shared_run(cid, device, monkeypatch)
    learner, first = got["learner"], got["calls"][0]
    norm = float(first["stats"][2])
    np.testing.assert_allclose(norm, s64["grad_norm"], rtol=RS.bounds(cid)[0])
    clip = float(RS.case_args(c).grad_norm_clip)
    assert clip == RS.CLIP and (norm > clip) == RS.clips(cid) == (cid in RS.CLIPPED), norm
    coef = min(1.0, clip / (norm + 1e-6))  # clip_grad_norm_
    assert len(g64) == len(learner._flat.views) == len(names)
    assert names == [k for k, _ in learner.mac.agent.named_parameters()] + \
        [k for k, _ in learner.mixer.named_parameters()]
    bounds = RS.grad_bounds(cid, g64)
    worst, where, fails = 0.0, None, []
    for (q, off, k), ref, bound, name in zip(learner._flat.views, g64, bounds, names):
        assert tuple(q.shape) == tuple(ref.shape)
        mine = first["grads"][off:off + k].view_as(q).to(torch.float64) / coef
        err = float((mine - ref).abs().max())
        if err / bound > worst:
            worst, where = err / bound, name
        if err > bound:
            fails.append(f"{name} at {off} {tuple(q.shape)}: max error {err:.3e} > {bound:.3e} "
                         f"(max|g64| {float(ref.abs().max()):.3e})")
    print(f"  {cid}: grad_norm {norm:.6g} (clip factor {coef:.4g}), "
          f"largest gradient error / bound {worst:.3f} at {where}")
    assert not fails, f"{cid}: " + "; ".join(fails)


# ---- c. no dependence on workspace contents ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", RS.IDS)
def test_result_does_not_depend_on_workspace_contents(device, monkeypatch, cid):
    """Three calls from a workspace refilled with finite garbage before each, from a zeroed workspace, and from a
    zeroed workspace again: bit-identical statistics, gradients, parameters and square_avg after every call."""
    zero = _shared_run(cid, device, monkeypatch)
    _set_env(monkeypatch, RS.case(cid))
    garbage = _run(cid, device, workspace="garbage")
    again = _run(cid, device)
    _assert_bitwise(zero, again, f"{cid} zero vs zero")
    _assert_bitwise(zero, garbage, f"{cid} zero vs garbage")
    assert garbage["target_is_online"] and again["target_is_online"]


# ---- d. one stream equals side stream ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["na1-ne1", "k48-a32", "attn-qmix-nola-a16", "attn-vdn-na1-ne1"])
def test_one_stream_equals_side_stream(device, monkeypatch, cid):
    side = _shared_run(cid, device, monkeypatch)
    _set_env(monkeypatch, RS.case(cid), one_stream=True)
    one = _run(cid, device)
    _assert_bitwise(side, one, f"{cid} side vs one stream")


# ---- e. sampled view equals gathered copy -----------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["na1-ne1", "k48-a32"])
def test_sampled_view_equals_gathered_copy(device, monkeypatch, cid):
    """The case's episodes sampled, in reverse order, as an in-place view of a device replay buffer (the slot map
    travels as a kernel argument, MlgRefilLearnerBufs.host_rows) train bit for bit like the gathered copy, as
    test_refil_learner_sampled_view_matches_copy holds the refil_8 shape to."""
    from maleague.components.replay_buffer import ReplayBuffer, SampledEpisodeBatch
    c, arrs, _, _, groups = _inputs(cid)
    _set_env(monkeypatch, c)
    eb = _batch_from(arrs, device, NE=c.NE, ED=c.ED, NA=c.NA, A=c.A)
    info = {"n_agents": c.NA, "n_actions": c.A, "n_entities": c.NE, "entity_shape": c.ED, "episode_limit": c.T - 1}
    scheme, groups_, pre = entity_scheme_for(info, torch)
    buf = ReplayBuffer(scheme, groups_, c.B + 2, c.T, preprocess=pre, device=device)
    buf.insert_episode_batch(eb)
    ids = np.arange(c.B)[::-1].copy()
    view = SampledEpisodeBatch(buf, ids)
    copy_ = buf[ids]
    assert view.host_rows is not None and view.host_rows.dtype == np.int32 and copy_.batch_size == c.B
    for k, v in copy_.data.transition_data.items():
        assert torch.equal(v.cpu(), torch.from_numpy(arrs[k][ids].copy()).to(v.dtype)), k
    L1, _, _ = _fresh(cid, device)
    L2, _, _ = _fresh(cid, device)
    for i, ep in enumerate(RS.CALLS):
        g = groups[i][torch.from_numpy(ids)].to(device)
        L1.train(view, 0, episode_num=ep, groupA=g)
        L2.train(copy_, 0, episode_num=ep, groupA=g)
        torch.cuda.synchronize()
        assert L1.last_stats == L2.last_stats, (i, L1.last_stats, L2.last_stats)
        assert torch.equal(L1._stats, L2._stats) and torch.equal(L1._grads, L2._grads), i
        assert torch.equal(L1._flat.flat, L2._flat.flat) and torch.equal(L1._sq, L2._sq), i
    assert view._rows is None  # the slot map never went to the device
    assert torch.equal(L1._tflat.flat, L1._flat.flat) and torch.equal(L2._tflat.flat, L2._flat.flat)


# ---- f. the reference's fixture without the last-action columns -------------------------------------------------------
def test_no_last_action_call_matches_golden(device, golden, monkeypatch):
    """One REFILLearner.train call of the reference with entity_last_action False at NA 5, NE 9, ED 8, A 16
    (tests/golden/refil_learner_nola.npz), at the bounds of test_refil_learner_two_calls_match_golden."""
    from helpers import refil_args
    from test_gpu_refil_learner import _pre
    _set_env(monkeypatch, RS.case("nola-a16"))
    d, after = golden("refil_learner_nola.npz"), golden("refil_learner_nola_after.npz")
    na, ne, ed, A = (int(x) for x in d["dims"])
    a = refil_args(device="cuda", n_agents=na, n_entities=ne, n_actions=A, entity_shape=ed, entity_last_action=False)
    eb = _batch_from(_pre(d, "b."), device, NE=ne, ED=ed, NA=na, A=A)
    L, log = _learner(eb, _pre(d, "p0.agent."), _pre(d, "p0.mixer."), a)
    assert L._cfg(eb.batch_size, eb.max_seq_length).entity_last_action == 0
    L.train(eb, 0, episode_num=0, groupA=torch.from_numpy(d["c0.groupA"]))
    st = L.last_stats
    assert set(st) == set(STAT_KEYS) == set(log.stats)
    for k, v in st.items():
        np.testing.assert_allclose(v, float(d[f"c0.stat.{k}"]), rtol=2e-4, atol=1e-6, err_msg=k)
    for k, v in L.mac.agent.named_parameters():
        np.testing.assert_allclose(v.detach().cpu().numpy(), after[f"c0.agent.{k}"], atol=2e-5, rtol=0,
                                   err_msg=f"agent {k}")
    for k, v in L.mixer.named_parameters():
        np.testing.assert_allclose(v.detach().cpu().numpy(), after[f"c0.mixer.{k}"], atol=2e-5, rtol=0,
                                   err_msg=f"mixer {k}")
