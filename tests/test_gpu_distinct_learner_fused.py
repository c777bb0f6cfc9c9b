"""GPU parity of the fused learner with distinct per-agent networks (mlg_qlearner_train with cfg.distinct = 1, the
default of QLearner.train with a DistinctMAC) at the cases of tests/distinct_learner_shapes.py: the smallest shapes at
which the per-agent instances' indexing can go wrong (one row past a 16-row tile, three tiles, N = 32 on five episodes,
two action tiles, N = 1). tests/test_distinct_learner_dispatch.py pins on the CPU the arm each case runs and that the
fp32 and float64 oracles agree on every live pick at the cases' seeds.

Tolerances are tests/learner_arm_shapes.py's: statistics rtol 2e-4 / atol 1e-6, parameters atol 5e-5, gradients 1e-4 of
the float64 tensor's largest element. Every comparison prints its largest error as a share of its bound
(profiles/distinct/README.md records them).

Batches (distinct_learner_shapes.batch): 8 stored steps, filled prefixes 6 / 5 / 0 / 3 / 1 / 2 / 6 / 4 cyclically -- a
never-filled and a one-transition episode in every batch -- and terminated flags; the learner reads all 8 stored
steps, the oracle trains on the copy truncated to max_t_filled = 6.
"""
import numpy as np
import pytest
import torch

import distinct_learner_shapes as DLS
import distinct_ref as DR
import learner_arm_shapes as LA
import learner_ref as LR
from helpers import scheme_for
from test_gpu_learner_shapes import STAT_KEYS, _episode_batch, _Log

pytestmark = pytest.mark.gpu

F64 = torch.float64
LOSS_KEYS = ("loss", "td_error_abs", "q_taken_mean", "target_mean")


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    for k in ("MLG_MIX_GENERIC", "MLG_LEARNER_FULL", "MLG_DISTINCT_LEARNER"):
        monkeypatch.delenv(k, raising=False)


def _distinct_learner(eb, args, agents0, mixer0):
    from maleague.controllers import DistinctMAC
    from maleague.learners import QLearner
    mac = DistinctMAC(eb.scheme, eb.groups, args)
    DR.load_agents(mac, agents0)
    log = _Log()
    learner = QLearner(mac, eb.scheme, log, args, name="home")
    if args.mixer == "qmix":
        msd = {k: torch.as_tensor(np.asarray(v)) for k, v in mixer0.items()}
        learner.mixer.load_state_dict(msd)
        learner.target_mixer.load_state_dict(msd)
    learner.build_optimizer()
    return learner, log


def _fresh(cid, device, tb=None):
    c, args, agents0, mixer0, tb0 = DLS.inputs(cid)
    eb = _episode_batch(tb0 if tb is None else tb, device)
    assert eb.max_seq_length == DLS.T_STORED and int(eb.max_t_filled()) == DLS.T_FILLED and eb.batch_size == c.B
    learner, log = _distinct_learner(eb, args, agents0, mixer0)
    from maleague import _native
    assert _native.qlearner_describe(learner._cfg(eb.batch_size, eb.max_seq_length)) == c.arm
    return learner, log, eb


def _snap(learner):
    torch.cuda.synchronize()
    return {"stats": learner._stats.cpu().numpy().copy(), "grads": learner._grads.cpu().numpy().copy(),
            "params": learner._flat.flat.cpu().numpy().copy(), "tparams": learner._tflat.flat.cpu().numpy().copy(),
            "sq": learner._sq.cpu().numpy().copy()}


def _same(a, b, what, keys=("grads", "params", "tparams", "sq")):
    assert np.array_equal(a["stats"][:7], b["stats"][:7]), f"{what}: stats {a['stats']} vs {b['stats']}"
    for k in keys:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differ at {np.flatnonzero(a[k] != b[k])[:8]}"


def _grad_check(views, grads, coef, g64, what, skip=()):
    """grads (flat, after the clip) / coef per tensor of ``views`` against the float64 list; -> worst error / bound."""
    assert len(views) == len(g64)
    worst = 0.0
    for j, ((q, off, k), ref) in enumerate(zip(views, g64)):
        if j in skip:
            continue
        assert tuple(q.shape) == tuple(ref.shape)
        mine = grads[off:off + k].view_as(q).to(F64) / coef
        err, scale = float((mine - ref).abs().max()), float(ref.abs().max())
        worst = max(worst, err / (LA.GRAD_RTOL * scale))
        assert err <= LA.GRAD_RTOL * scale, f"{what} tensor {j} {tuple(q.shape)}: max error {err:.3e} > {LA.GRAD_RTOL * scale:.3e}"
    return worst


_RUNS = {}


def _run(cid, device):
    """A fresh learner's three calls, shared by the tests of a case."""
    if cid in _RUNS:
        return _RUNS[cid]
    learner, log, eb = _fresh(cid, device)
    out = {"stats": [], "learner": learner, "log": log, "snaps": []}
    for t_env, ep in DLS.CALLS:
        learner.train(eb, t_env, ep)
        out["stats"].append(dict(learner.last_stats))
        out["snaps"].append(_snap(learner))
    _RUNS[cid] = out
    return out


# ---- 1. first-call gradients against the float64 oracle ----------------------------------------------------------------
@pytest.mark.parametrize("cid", DLS.IDS)
def test_first_call_gradients_vs_float64_oracle(device, cid):
    """The gradient vector after the first call, scaled back by the factor clip_grad_norm_ applied (from the call's own
    grad_norm), per agent and tensor against the float64 oracle's .grad before its clip."""
    c, args, _, _, _ = DLS.inputs(cid)
    _, _, g64, s64 = DLS.oracle(cid)
    got = _run(cid, device)
    norm = float(got["snaps"][0]["stats"][1])
    np.testing.assert_allclose(norm, s64["grad_norm"], rtol=LA.STAT_RTOL)
    coef = min(1.0, args.grad_norm_clip / (norm + 1e-6))
    views = got["learner"]._flat.views
    assert len(views) >= 8 * c.N
    worst = _grad_check(views, torch.from_numpy(got["snaps"][0]["grads"]), coef, g64, cid)
    print(f"  {cid}: grad_norm {norm:.6g} (clip factor {coef:.4g}), largest gradient error / bound {100 * worst:.2f} %")


# ---- 2. three-call trajectory against the fp32 oracle ------------------------------------------------------------------
@pytest.mark.parametrize("cid", DLS.IDS)
def test_three_call_trajectory_vs_oracle(device, cid):
    """Target equal to online, stale, then stale ending with the sync: statistics, the N networks, their targets, the
    mixer and its target, targets equal to online after the sync, every network's trained_steps."""
    c, args, _, _, tb = DLS.inputs(cid)
    want, ref, _, _ = DLS.oracle(cid)
    got = _run(cid, device)
    learner = got["learner"]
    worst_s = 0.0
    for i in range(len(DLS.CALLS)):
        print(f"  {cid} call {i}: " + ", ".join(f"{k} {got['stats'][i][k]:.7g}/{want[i][k]:.7g}" for k in STAT_KEYS))
        for k in STAT_KEYS:
            g, w = got["stats"][i][k], want[i][k]
            assert np.isfinite(g), f"{cid} call {i} {k}"
            worst_s = max(worst_s, abs(g - w) / (LA.STAT_ATOL + LA.STAT_RTOL * abs(w)))
            np.testing.assert_allclose(g, w, rtol=LA.STAT_RTOL, atol=LA.STAT_ATOL, err_msg=f"{cid} call {i} {k}")
    assert set(got["log"].stats) == {"home_qlearner_" + k for k in STAT_KEYS}
    assert learner.last_target_update_episode == ref.last_target_update_episode == 200
    pairs = []
    for i in range(c.N):
        pairs.append((f"agent {i}", learner.mac.agents[i].state_dict(), ref.agent_states()[i]))
        pairs.append((f"target agent {i}", learner.target_mac.agents[i].state_dict(), ref.target_states()[i]))
    if args.mixer == "qmix":
        pairs += [("mixer", learner.mixer.state_dict(), ref.mixer_state()),
                  ("target mixer", learner.target_mixer.state_dict(), ref.tmp)]
    errs = {}
    for name, g, w in pairs:
        assert list(g.keys()) == list(w.keys())
        for k, v in g.items():
            errs[f"{name} {k}"] = float(np.abs(v.cpu().numpy() - w[k].detach().numpy()).max())
    worst = max(errs, key=errs.get)
    print(f"  {cid}: largest statistic error / bound {100 * worst_s:.2f} %, largest parameter error {errs[worst]:.3e} at "
          f"{worst} ({100 * errs[worst] / LA.PARAM_ATOL:.2f} % of {LA.PARAM_ATOL:.1e})")
    for k, e in errs.items():
        assert e <= LA.PARAM_ATOL, f"{cid} {k}: {e:.3e} > {LA.PARAM_ATOL:.1e}"
    for a, t in zip(learner.mac.agents, learner.target_mac.agents):  # the third call ended with the sync
        assert all(torch.equal(v, t.state_dict()[k]) for k, v in a.state_dict().items())
    assert np.array_equal(got["snaps"][2]["params"], got["snaps"][2]["tparams"])
    n = DLS.mask(tb).sum() * (c.N if args.mixer is None else 1)  # IQL expands the mask over the agents
    assert float(got["snaps"][0]["stats"][5]) == n and float(got["snaps"][0]["stats"][6]) == n
    assert [a.trained_steps for a in learner.mac.agents] == [ref.trained_steps] * c.N
    assert ref.trained_steps == len(DLS.CALLS) * int(n)


# ---- 3, 4, 6. workspace contents, MLG_LEARNER_FULL, determinism --------------------------------------------------------
def _three(cid, device, monkeypatch, ws=None, full=False):
    """Three calls (target a copy, stale then synced, a copy again) from a fresh learner. ws: "nan" = a workspace of
    exactly the queried size, NaN-filled before every call; None = the learner's own (zeroed, larger)."""
    from maleague import _native
    if full:
        monkeypatch.setenv("MLG_LEARNER_FULL", "1")
    learner, _, eb = _fresh(cid, device)
    if ws == "nan":
        need = _native.load().mlg_qlearner_workspace_floats(_native.byref(learner._cfg(eb.batch_size, eb.max_seq_length)))
        assert need > 0
        learner._ws = torch.empty(int(need), dtype=torch.float32, device=device)
    out = []
    for i, ep in enumerate([0, 200, 200]):
        if ws == "nan":
            learner._ws.fill_(float("nan"))
        learner.train(eb, i, ep)
        if ws == "nan":
            assert learner._ws.numel() == need  # train() kept the exact-size buffer
        out.append(_snap(learner))
    monkeypatch.delenv("MLG_LEARNER_FULL", raising=False)
    return out


@pytest.mark.parametrize("cid", DLS.IDS)
def test_workspace_contents_full_path_and_rerun_are_bit_identical(device, monkeypatch, cid):
    """A NaN-filled workspace of exactly mlg_qlearner_workspace_floats (no kernel reads an element the call did not
    write, none writes past the end that the next call's fill would hide), a zeroed one, a second run from the same
    state, and MLG_LEARNER_FULL=1 (every row to max_t_filled, both nets) all give the same bits."""
    nan = _three(cid, device, monkeypatch, ws="nan")
    zero = _three(cid, device, monkeypatch)
    again = _three(cid, device, monkeypatch)
    full = _three(cid, device, monkeypatch, full=True)
    for i in range(3):
        for k in ("stats", "grads", "params", "sq"):
            assert np.all(np.isfinite(nan[i][k])), f"call {i}: {k} not finite"
        _same(nan[i], zero[i], f"{cid} call {i} NaN vs zeroed workspace")
        _same(zero[i], again[i], f"{cid} call {i} two runs")
        assert np.array_equal(zero[i]["stats"], again[i]["stats"])
        _same(zero[i], full[i], f"{cid} call {i} skip vs full")
    assert zero[0]["stats"][7] < full[0]["stats"][7]  # the default path planned fewer forward blocks


# ---- 5. sampled views ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", DLS.IDS)
def test_sampled_view_equals_gathered_copy(device, monkeypatch, cid):
    """The case's episodes sampled (in a shuffled order) as an in-place view of a device replay ring with three spare
    slots, through the kernel-argument slot map (host_rows) and the device map (rows; taken when the batch exceeds the
    inline-row capacity, set to 0 here), train bit for bit like the gathered copy of the same episodes."""
    from maleague import _native
    from maleague.components.replay_buffer import ReplayBuffer, SampledEpisodeBatch
    c, args, agents0, mixer0, tb = DLS.inputs(cid)
    N, A, S, d_obs = DLS.dims(c)
    scheme, groups, pre = scheme_for({"state_shape": S, "obs_shape": d_obs, "n_actions": A, "n_agents": N}, torch)
    buf = ReplayBuffer(scheme, groups, c.B + 3, DLS.T_STORED, preprocess=pre, device=device)
    buf.insert_episode_batch(_episode_batch({k: v[:3] for k, v in tb.items()}, device))  # slots 0..2: other episodes
    buf.insert_episode_batch(_episode_batch(tb, device))
    for k, v in tb.items():  # the insert recomputes actions_onehot: restore the steps past the episodes' ends
        buf.data.transition_data[k][3:3 + c.B].copy_(v)
    ids = 3 + np.random.RandomState(1).permutation(c.B)
    view = SampledEpisodeBatch(buf, ids)
    assert view.host_rows is not None and list(view.host_rows) == list(ids) and view.max_seq_length == DLS.T_STORED
    copy_ = buf[ids]
    assert torch.equal(copy_["obs"].cpu(), tb["obs"][ids - 3])
    Lh, Lr, Lc = [_distinct_learner(copy_, args, agents0, mixer0)[0] for _ in range(3)]
    lib = _native.load(require_gpu=True)
    for call, ep in enumerate([0, 200]):
        Lh.train(view, 0, ep)
        assert view._rows is None  # the slot map travelled as a kernel argument
        Lc.train(copy_, 0, ep)
        with monkeypatch.context() as m:
            m.setattr(lib, "mlg_qlearner_inline_rows", lambda: 0)
            view_r = type(view)(buf, ids)
            Lr.train(view_r, 0, ep)
            assert view_r._rows is not None and view_r._data is None
        sc = _snap(Lc)
        for tag, L in (("host_rows", Lh), ("rows", Lr)):
            _same(_snap(L), sc, f"{cid} call {call} {tag}")
            assert np.array_equal(_snap(L)["stats"], sc["stats"])
        assert np.all(np.isfinite(sc["stats"]))


# ---- equal networks against the shared agent ----------------------------------------------------------------------------
def _shared_learner(eb, args, agent0, mixer0):
    from test_gpu_learner_shapes import _learner
    return _learner(eb, agent0, mixer0, LR.clone_args(args, mac="basic", device="cuda"))[0]


def test_equal_networks_against_the_shared_agent(device):
    """n5-h64-b32 with network 0's weights in every slot against mac=basic (obs_agent_id off) on the same batch and
    weights, first call: the four loss statistics agree within the statistics tolerance, and the pre-clip gradients of
    the N networks sum to the shared agent's gradient per tensor, within 1e-4 of the float64 tensor's largest element
    (oracle/learner_ref.py's shared-agent restatement in float64)."""
    cid = "n5-h64-b32"
    c, args, agents0, mixer0, tb = DLS.inputs(cid)
    eq = [agents0[0]] * c.N
    eb = _episode_batch(tb, device)
    dl, _ = _distinct_learner(eb, args, eq, mixer0)
    sl = _shared_learner(eb, args, agents0[0], mixer0)
    dl.train(eb, 0, 0)
    sl.train(eb, 0, 0)
    ds, ss = dict(dl.last_stats), dict(sl.last_stats)
    worst_s = 0.0
    for k in LOSS_KEYS:
        worst_s = max(worst_s, abs(ds[k] - ss[k]) / (LA.STAT_ATOL + LA.STAT_RTOL * abs(ss[k])))
        np.testing.assert_allclose(ds[k], ss[k], rtol=LA.STAT_RTOL, atol=LA.STAT_ATOL, err_msg=k)
    ref64 = LR.QLearnerRef(agents0[0], mixer0, LR.clone_args(args, mac="basic", device="cpu"), dtype=F64)
    ref64.train({k: v.clone() for k, v in DLS.oracle_batch(tb).items()}, 0, 0)
    g64 = ref64.last_grads
    coef_d = min(1.0, args.grad_norm_clip / (ds["grad_norm"] + 1e-6))
    coef_s = min(1.0, args.grad_norm_clip / (ss["grad_norm"] + 1e-6))
    dg, sg = dl._grads.cpu().to(F64) / coef_d, sl._grads.cpu().to(F64) / coef_s
    worst = 0.0
    for j in range(8):
        _, off_s, k = sl._flat.views[j]
        total = sum(dg[dl._flat.views[8 * i + j][1]:dl._flat.views[8 * i + j][1] + k] for i in range(c.N))
        scale = float(g64[j].abs().max())
        err = float((total - sg[off_s:off_s + k]).abs().max())
        err64 = float((total - g64[j].reshape(-1)).abs().max())
        worst = max(worst, err / (LA.GRAD_RTOL * scale), err64 / (LA.GRAD_RTOL * scale))
        assert err <= LA.GRAD_RTOL * scale and err64 <= LA.GRAD_RTOL * scale, (DR.AGENT_KEYS[j], err, err64, scale)
    print(f"  equal networks: largest statistic error / bound {100 * worst_s:.2f} %, largest summed-gradient error / "
          f"bound {100 * worst:.2f} %")


def test_one_network_against_the_shared_learner(device):
    """n1-h64-b16: one slot, one network, against the shared fused learner (mac=basic, obs_agent_id off) on the same
    weights and batch: parameters, gradients and square averages after the three calls are bit-identical. An instance of
    the distinct layout is the shared agent's problem at N = 1, R = B, row for row and chunk for chunk; the shared
    learner runs the H = 64 fused forms here (qmix-split, bwd-fused), which are the generic forms' arithmetic in the
    same order."""
    cid = "n1-h64-b16"
    c, args, agents0, mixer0, tb = DLS.inputs(cid)
    eb = _episode_batch(tb, device)
    dl, _ = _distinct_learner(eb, args, agents0, mixer0)
    sl = _shared_learner(eb, args, agents0[0], mixer0)
    for t_env, ep in DLS.CALLS:
        dl.train(eb, t_env, ep)
        sl.train(eb, t_env, ep)
    a, b = dl._flat.flat.cpu().numpy(), sl._flat.flat.cpu().numpy()
    err = float(np.abs(a - b).max())
    print(f"  n = 1 against the shared learner: largest parameter difference {err:.3e} "
          f"({100 * err / LA.PARAM_ATOL:.2f} % of {LA.PARAM_ATOL:.1e}), bit-identical: {np.array_equal(a, b)}")
    assert a.shape == b.shape and err <= LA.PARAM_ATOL
    assert np.array_equal(a, b) and torch.equal(dl._grads, sl._grads) and torch.equal(dl._sq, sl._sq)
    assert np.array_equal(dl._stats.cpu().numpy()[:7], sl._stats.cpu().numpy()[:7])
    assert dl.mac.agents[0].trained_steps == sl.mac.agent.trained_steps > 0


# ---- dead slots ---------------------------------------------------------------------------------------------------------
def _kill(tb, slot):
    """Only the no-op (action 0) is ever available to ``slot``, and taken."""
    tb = {k: v.clone() for k, v in tb.items()}
    tb["avail_actions"][:, :, slot] = 0
    tb["avail_actions"][:, :, slot, 0] = 1
    tb["actions"][:, :, slot] = 0
    tb["actions_onehot"][:, :, slot] = 0
    tb["actions_onehot"][:, :, slot, 0] = 1
    return tb


def _dead_case(device, tb, dead, mixer=None):
    """One call on ``tb`` at n2-h32-b17's shape: (learner, parameters before, float64 oracle, its statistics)."""
    c, args, agents0, mixer0, _ = DLS.inputs("n2-h32-b17")
    if mixer is not None:
        args = LR.clone_args(args, **mixer)
        mixer0 = mixer0 if args.mixer == "qmix" else None
    eb = _episode_batch(tb, device)
    learner, _ = _distinct_learner(eb, args, agents0, mixer0)
    before = learner._flat.flat.clone()
    learner.train(eb, 0, 0)
    ref64 = DLS.make_oracle(agents0, mixer0, args, F64)
    want = ref64.train({k: v.clone() for k, v in DLS.oracle_batch(tb).items()}, 0, 0)
    for k in LOSS_KEYS:  # a dead slot's chosen Q keeps its value in the mix, the loss and the statistics
        np.testing.assert_allclose(learner.last_stats[k], want[k], rtol=LA.STAT_RTOL, atol=LA.STAT_ATOL, err_msg=k)
    return learner, before, ref64, args


def _slot_untouched(learner, before, slot):
    for j in range(8 * slot, 8 * slot + 8):
        p, off, k = learner._flat.views[j]
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0 and float(learner._grads[off:off + k].abs().max()) == 0.0
        assert torch.equal(learner._flat.flat[off:off + k], before[off:off + k])


def test_dead_slot_zero_gradient_and_unmoved_network(device):
    """Slot 0 of n2-h32-b17 dead in every stored step: exact zeros in every tensor of network 0, its parameters bit for
    bit where they were; grad_norm is the float64 norm without the slot's share and the other tensors' gradients match
    float64. Decided on the device: the call has no host sync to decide it on."""
    _, _, _, _, tb = DLS.inputs("n2-h32-b17")
    learner, before, ref64, args = _dead_case(device, _kill(tb, 0), 0)
    _slot_untouched(learner, before, 0)
    g64 = ref64.last_grads
    assert max(float(g.abs().max()) for g in g64[:8]) > 1e-3  # the plain arithmetic would have moved it
    norm64 = float(torch.sqrt(sum((g ** 2).sum() for g in g64[8:])))
    norm = learner.last_stats["grad_norm"]
    np.testing.assert_allclose(norm, norm64, rtol=LA.STAT_RTOL)
    coef = min(1.0, args.grad_norm_clip / (norm + 1e-6))
    worst = _grad_check(learner._flat.views, learner._grads.cpu(), coef, g64, "dead slot 0", skip=range(8))
    print(f"  slot 0 dead: grad_norm {norm:.6g} / float64 without the slot {norm64:.6g}, largest live gradient error / "
          f"bound {100 * worst:.2f} %")
    assert not torch.equal(learner._flat.flat[learner._flat.views[8][1]:], before[learner._flat.views[8][1]:])


@pytest.mark.parametrize("mixer", [LA.VDN, LA.QMIX], ids=["vdn", "qmix"])
def test_every_slot_dead(device, mixer):
    """Both slots of n2-h32-b17's shape dead. With VDN the networks are all the parameters there are: no parameter
    moves, grad_norm == 0, the loss is finite. With QMIX the rule cuts the path into the networks only (a
    dead slot's chosen Q keeps its value in the mix), so the hypernetworks still receive the float64 oracle's gradient
    and grad_norm is its norm; no network parameter moves."""
    _, _, _, _, tb = DLS.inputs("n2-h32-b17")
    learner, before, ref64, args = _dead_case(device, _kill(_kill(tb, 0), 1), None, mixer)
    _slot_untouched(learner, before, 0)
    _slot_untouched(learner, before, 1)
    assert np.isfinite(learner.last_stats["loss"]) and learner.last_stats["loss"] > 0
    assert [a.trained_steps for a in learner.mac.agents] == [int(DLS.mask(tb).sum())] * 2  # counted all the same
    if args.mixer != "qmix":
        assert torch.equal(learner._flat.flat, before) and learner.last_stats["grad_norm"] == 0.0
        assert float(learner._grads.abs().max()) == 0.0
        return
    g64 = ref64.last_grads
    norm64 = float(torch.sqrt(sum((g ** 2).sum() for g in g64[16:])))
    np.testing.assert_allclose(learner.last_stats["grad_norm"], norm64, rtol=LA.STAT_RTOL)
    coef = min(1.0, args.grad_norm_clip / (learner.last_stats["grad_norm"] + 1e-6))
    _grad_check(learner._flat.views, learner._grads.cpu(), coef, g64, "all dead", skip=range(16))


def test_slot_alive_in_one_stored_step_trains(device):
    """Slot 0 of n2-h32-b17 dead everywhere but the last stored step of episode 1, where one more action is available
    (not taken): the slot is alive and trains on all its rows; every gradient matches the float64 oracle, which knows no
    dead-slot rule."""
    _, _, _, _, tb = DLS.inputs("n2-h32-b17")
    tb = _kill(tb, 0)
    assert int(tb["filled"][1].sum()) == 5
    tb["avail_actions"][1, 4, 0, 3] = 1
    learner, before, ref64, args = _dead_case(device, tb, None)
    norm = learner.last_stats["grad_norm"]
    np.testing.assert_allclose(norm, float(torch.sqrt(sum((g ** 2).sum() for g in ref64.last_grads))), rtol=LA.STAT_RTOL)
    coef = min(1.0, args.grad_norm_clip / (norm + 1e-6))
    worst = _grad_check(learner._flat.views, learner._grads.cpu(), coef, ref64.last_grads, "alive once")
    assert all(float(learner._flat.views[j][0].grad.abs().max()) > 0 for j in range(8))
    print(f"  slot 0 alive in one stored step: largest gradient error / bound {100 * worst:.2f} %")


# ---- fused against unrolled ---------------------------------------------------------------------------------------------
def test_fused_against_unrolled_and_switching(device, monkeypatch):
    """n2-h32-b17, first call: the default (fused) call against MLG_DISTINCT_LEARNER=unrolled on equal learners:
    statistics within the statistics tolerance, gradients within 1e-4 of the float64 tensor's largest element. Then each
    learner takes a second call on the other branch (the optimiser state is shared between the branches): both end
    within the parameter tolerance of each other, with equal step counts in the optimiser's state dict."""
    cid = "n2-h32-b17"
    c, args, _, _, _ = DLS.inputs(cid)
    _, _, g64, _ = DLS.oracle(cid)
    fl, _, eb = _fresh(cid, device)
    ul, _, _ = _fresh(cid, device)
    fl.train(eb, 0, 0)
    monkeypatch.setenv("MLG_DISTINCT_LEARNER", "unrolled")
    ul.train(eb, 0, 0)
    fs, us = dict(fl.last_stats), dict(ul.last_stats)
    worst_s = 0.0
    for k in STAT_KEYS:
        worst_s = max(worst_s, abs(fs[k] - us[k]) / (LA.STAT_ATOL + LA.STAT_RTOL * abs(us[k])))
        np.testing.assert_allclose(fs[k], us[k], rtol=LA.STAT_RTOL, atol=LA.STAT_ATOL, err_msg=k)
    cf = min(1.0, args.grad_norm_clip / (fs["grad_norm"] + 1e-6))
    cu = min(1.0, args.grad_norm_clip / (us["grad_norm"] + 1e-6))
    fg, ug = fl._grads.cpu().to(F64) / cf, ul._grads.cpu().to(F64) / cu
    worst = 0.0
    for (q, off, k), ref in zip(fl._flat.views, g64):
        err, scale = float((fg[off:off + k] - ug[off:off + k]).abs().max()), float(ref.abs().max())
        worst = max(worst, err / (LA.GRAD_RTOL * scale))
        assert err <= LA.GRAD_RTOL * scale, (off, err, scale)
    print(f"  fused vs unrolled: largest statistic difference / bound {100 * worst_s:.2f} %, largest gradient difference "
          f"/ bound {100 * worst:.2f} %")
    fl.train(eb, 0, 100)   # unrolled, on the fused call's state
    monkeypatch.delenv("MLG_DISTINCT_LEARNER")
    ul.train(eb, 0, 100)   # fused, on the unrolled call's state
    err = float((fl._flat.flat - ul._flat.flat).abs().max())
    assert err <= LA.PARAM_ATOL, err
    for L in (fl, ul):
        steps = {float(s["step"]) for s in L.optimiser.state_dict()["state"].values()}
        assert steps == {2.0}
    assert [a.trained_steps for a in fl.mac.agents] == [a.trained_steps for a in ul.mac.agents]
    monkeypatch.setenv("MLG_DISTINCT_LEARNER", "both")
    with pytest.raises(ValueError, match="MLG_DISTINCT_LEARNER"):
        fl.train(eb, 0, 100)


# ---- checkpoint ---------------------------------------------------------------------------------------------------------
def test_checkpoint_after_two_fused_calls_resumes_bit_for_bit(device, tmp_path):
    """n3-h128-a17: after two calls (the second ends with the target sync, which is what load_models restores) the
    learner is saved; a fresh learner that loads it takes the third call to the same bits as the uninterrupted one."""
    cid = "n3-h128-a17"
    learner, _, eb = _fresh(cid, device)
    for ep in (0, 200):
        learner.train(eb, 0, ep)
    assert torch.equal(learner._flat.flat, learner._tflat.flat)
    path = str(tmp_path)
    learner.save_models(path, learner.name)
    import os
    assert "home_qlearner_opt.th" in os.listdir(path)
    opt = torch.load(f"{path}/home_qlearner_opt.th", weights_only=True)
    assert len(opt["state"]) == len(learner._flat.views) and all(float(s["step"]) == 2.0 for s in opt["state"].values())
    fresh, _, _ = _fresh(cid, device)
    fresh.load_models(path)
    fresh.last_target_update_episode = learner.last_target_update_episode  # not part of a checkpoint
    assert torch.equal(fresh._flat.flat, learner._flat.flat) and torch.equal(fresh._sq, learner._sq)
    learner.train(eb, 0, 200)
    fresh.train(eb, 0, 200)
    _same(_snap(fresh), _snap(learner), "third call after the reload")
    assert float(fresh._step) == float(learner._step) == 3.0
