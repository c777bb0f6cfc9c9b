"""Prioritized episode replay on the CPU: the oracle (tests/per_ref.py) pinned to the reference's own
BinarySumTree / Memory through tests/golden/per.npz, the weighted learner oracle against QLearnerRef, the host path of
PrioritizedReplayBuffer against the oracle, the near-tie condition on the inputs of the GPU sampling test, and the
dispatch names, workspace sizes, struct layout and refusals. None of this exists without the feature."""
import ctypes

import numpy as np
import pytest
import torch

import learner_arm_shapes as LA
import learner_ref as LR
import per_cases as PC
import per_ref as PR
from helpers import qmix_args, refil_args, scheme_for

CAPS = (8, 64, 1024)


# ---- the oracle against the reference's recorded data ----------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("tag", ["", ".part"])
def test_selection_rule_is_the_sum_trees(golden, cap, tag):
    """The first slot in slot order whose inclusive cumulative priority is >= s is the leaf BinarySumTree.get(s)
    returned, for seeded draws, exact ties on cumulative boundaries, s = 0 and s = total; full and partially filled."""
    d = golden("per.npz")
    filled = int(d[f"c{cap}{tag}.filled"])
    prio = d[f"c{cap}.prio"][:filled]
    cum = np.cumsum(prio)
    s = d[f"c{cap}{tag}.s"]
    assert np.any(np.isin(s, cum)) and s.min() == 0.0 and s.max() == cum[-1]  # the ties are in the data
    rows = PR.select(cum, s)
    assert np.array_equal(rows, d[f"c{cap}{tag}.slot"])
    assert np.array_equal(prio[rows], d[f"c{cap}{tag}.p"])


@pytest.mark.parametrize("cap", CAPS)
def test_weight_formula_and_beta_step_are_memorys(golden, cap):
    d = golden("per.npz")
    prio = d[f"c{cap}.prio"]
    cum = np.cumsum(prio)
    assert cum[-1] == float(d[f"c{cap}.mem.total"]) and int(d[f"c{cap}.mem.n_entries"]) == cap
    rows = PR.select(cum, d[f"c{cap}.mem.s"])
    assert np.array_equal(rows, d[f"c{cap}.mem.slot"])
    assert len(set(rows.tolist())) < len(rows)  # the heavy slot spans several strata: duplicates
    beta = min(1.0, float(d[f"c{cap}.mem.beta0"]) + float(d[f"c{cap}.mem.increment"]))
    assert beta == float(d[f"c{cap}.mem.beta"])
    w = PR.weights(cap, prio[rows], cum[-1], beta)
    np.testing.assert_allclose(w, d[f"c{cap}.mem.is_weight"], rtol=1e-13, atol=0)
    assert w.max() == 1.0


def test_defaults_and_priority_rule_are_memorys(golden):
    d = golden("per.npz")
    assert (PR.E, PR.A, PR.BETA, PR.BETA_INCREMENT) == tuple(d["defaults"])
    np.testing.assert_allclose(PR.priority(d["prio_rule.err"]), d["prio_rule.p"], rtol=1e-15)


def test_rng_stream_is_the_projects():
    """per_ref's restatement of mlg_rng / mlg_ctr / mlg_u01 against the C oracle's, and the package's host stream."""
    import envref
    from maleague.components.replay_buffer import PER_PURPOSE, per_uniforms
    assert PER_PURPOSE == PR.PER_PURPOSE == 6
    for seed, draw, i in [(0, 0, 0), (7, 3, 31), (2 ** 40 + 5, 2 ** 31 + 1, 4095), (123456789, 17, 100)]:
        c = PR.ctr(draw, 0, PR.PER_PURPOSE, i)
        assert c == envref.ctr(draw, 0, PR.PER_PURPOSE, i)
        assert PR.rng(seed, c) == envref.rng(seed, c)
        assert PR.u01(PR.rng(seed, c)) == envref.u01(envref.rng(seed, c))
    u = PR.uniforms(11, 5, 64)
    assert np.array_equal(per_uniforms(11, 5, 64).numpy(), u) and 0.0 <= u.min() and u.max() < 1.0


# ---- the inputs of the GPU sampling test: no near tie ----------------------------------------------------------------
@pytest.mark.parametrize("sid", PC.SAMPLE_IDS)
def test_gpu_sampling_inputs_have_no_near_tie(sid):
    p, n, B, seed, draw = PC.sample_case(sid)
    rows, w, margin = PR.sample(p, n, B, seed, draw, PC.BETA)
    assert margin > PC.NEAR_TIE, f"{sid}: a draw lies {margin:.3e} of the total from a boundary; pick another seed"
    assert rows.min() >= 0 and rows.max() < n and w.max() == 1.0 and w.min() > 0.0
    if sid.startswith("skewed") and n > 1 and B >= 32:
        assert np.bincount(rows).max() >= 0.85 * B  # the heavy slot spans ~90 % of the strata


# ---- the weighted learner oracle ---------------------------------------------------------------------------------------
def _mask(ob):
    """mask = filled[:, :-1] * (1 - terminated shifted) of a truncated sample, [B, T - 1]."""
    m = ob["filled"][:, :-1, 0].double()
    m[:, 1:] = m[:, 1:] * (1 - ob["terminated"][:, :-2, 0].double())
    return m


@pytest.mark.parametrize("cid", ["split-h64-3v3", "vdn-fast-h32-3v3", "iql-h128-2v2"])
def test_weighted_oracle_with_unit_weights_is_qlearner_ref(cid):
    """PERLearnerRef with every weight 1 (and with none given) against QLearnerRef on learner_arm_shapes' fixture:
    statistics, gradients and parameters bit for bit over two calls; td_abs against its definition."""
    c = LA.case(cid)
    args = LA.case_args(c, "cpu")
    agent0, mixer0 = LA.case_weights(c, args)
    ob = LA.oracle_batch(LA.case_batch(c))
    for w in (None, np.ones(LA.B, np.float32)):
        ref = PR.PERLearnerRef(agent0, mixer0, LR.clone_args(args))
        ref.is_weight = w
        plain = LR.QLearnerRef(agent0, mixer0, LR.clone_args(args))
        for t_env, ep in LA.CALLS[:2]:
            want = plain.train({k: v.clone() for k, v in ob.items()}, t_env, ep)
            got = ref.train({k: v.clone() for k, v in ob.items()}, t_env, ep)
            assert got == want
            assert all(torch.equal(a, b) for a, b in zip(ref.last_grads, plain.last_grads))
        assert all(torch.equal(ref.p[k], plain.p[k]) for k in plain.p)
        n_mask = _mask(ob).sum(dim=1) * (args.n_agents if args.mixer is None else 1)
        assert ref.last_td_abs.shape == (LA.B,) and bool((n_mask > 0).all())
        mean = float((ref.last_td_abs * n_mask).sum() / n_mask.sum())
        np.testing.assert_allclose(mean, got["td_error_abs"], rtol=1e-5)


def test_weighted_oracle_scales_an_episodes_gradient():
    """Weights (1, 0, 0, 0, 0) leave the gradient of a batch holding only episode 0, scaled by the mask sums."""
    c = LA.case("vdn-fast-h32-3v3")
    args = LA.case_args(c, "cpu")
    agent0, _ = LA.case_weights(c, args)
    ob = LA.oracle_batch(LA.case_batch(c))
    ref = PR.PERLearnerRef(agent0, None, LR.clone_args(args), dtype=torch.float64)
    ref.is_weight = np.asarray([1, 0, 0, 0, 0], np.float64)
    ref.train({k: v.clone() for k, v in ob.items()}, 0, 0)
    one = LR.QLearnerRef(agent0, None, LR.clone_args(args), dtype=torch.float64)
    one.train({k: v[:1].clone() for k, v in ob.items()}, 0, 0)
    m = _mask(ob).sum(dim=1)
    for g, h in zip(ref.last_grads, one.last_grads):
        np.testing.assert_allclose(g.numpy(), h.numpy() * float(m[0] / m.sum()), rtol=1e-9, atol=1e-12)
    assert float(ref.last_td_abs[0]) > 0


# ---- the host path of PrioritizedReplayBuffer against the oracle -----------------------------------------------------
INFO = {"state_shape": 6, "obs_shape": 4, "n_actions": 3, "n_agents": 2}


def _buffer(size, seed=5, T=4):
    from maleague.components.replay_buffer import PrioritizedReplayBuffer
    scheme, groups, pre = scheme_for(INFO, torch)
    return PrioritizedReplayBuffer(scheme, groups, size, T, preprocess=pre, device="cpu", seed=seed)


def _episodes(n, T=4, seed=0):
    from maleague.components.episode_batch import EpisodeBatch
    scheme, groups, pre = scheme_for(INFO, torch)
    eb = EpisodeBatch(scheme, groups, n, T, preprocess=pre, device="cpu")
    g = torch.Generator().manual_seed(seed)
    eb.update({"state": torch.rand(n, T, 6, generator=g), "obs": torch.rand(n, T, 2, 4, generator=g),
               "actions": torch.randint(0, 3, (n, T, 2, 1), generator=g), "avail_actions": torch.ones(n, T, 2, 3, dtype=torch.int),
               "reward": torch.rand(n, T, 1, generator=g), "terminated": torch.zeros(n, T, 1, dtype=torch.uint8)})
    return eb


def test_constructor_signature_and_attributes():
    import inspect
    from maleague.components import PrioritizedReplayBuffer, ReplayBuffer
    names = list(inspect.signature(PrioritizedReplayBuffer.__init__).parameters)
    assert names[:7] == ["self", "scheme", "groups", "buffer_size", "max_seq_length", "preprocess", "device"]
    buf = _buffer(8)
    assert isinstance(buf, ReplayBuffer)
    assert (buf.e, buf.a, buf.beta, buf.beta_increment_per_sampling) == (PR.E, PR.A, PR.BETA, PR.BETA_INCREMENT)
    assert buf.priorities.dtype == torch.float32 and buf.priorities.shape == (8,) and float(buf.max_priority) == 1.0


def test_host_insert_sample_update_follow_the_oracle():
    """A partially filled buffer, inserts with and without errors, a wrapping insert, draws with duplicates, updates
    that raise the maximum: priorities, maximum, rows and weights against per_ref at every step."""
    size, B = 10, 4
    buf = _buffer(size, seed=9)
    prio, max_p, index, live = np.zeros(size), 1.0, 0, 0
    rs = np.random.RandomState(3)
    beta, draws = PR.BETA, 0
    steps = [(3, None), (3, "err"), (3, None), (3, "err"), (2, None)]  # 6 live, then wraps at 9 + 3 and 2 + ...
    for k, (n, kind) in enumerate(steps):
        errors = None if kind is None else rs.uniform(0.0, 3.0, size=n).astype(np.float32)
        buf.insert_episode_batch(_episodes(n, seed=k), errors=errors)
        room = size - index
        if n > room:  # the wrapping insert: both halves
            max_p = PR.insert(prio, max_p, index, room, None if errors is None else errors[:room])
            max_p = PR.insert(prio, max_p, 0, n - room, None if errors is None else errors[room:])
        else:
            max_p = PR.insert(prio, max_p, index, n, errors)
        live = min(size, max(live, index + n))
        index = (index + n) % size
        assert (buf.buffer_index, buf.episodes_in_buffer) == (index, live)
        np.testing.assert_array_equal(buf.priorities.numpy(), prio.astype(np.float32))
        assert float(buf.max_priority) == np.float32(max_p)
        if live > B:
            sample = buf.sample(B)
            beta = min(1.0, beta + PR.BETA_INCREMENT)
            rows, w, margin = PR.sample(prio.astype(np.float32), live, B, 9, draws, beta)
            draws += 1
            assert margin > PC.NEAR_TIE
            assert buf.beta == beta and buf.draws == draws
            assert sample.rows.dtype == torch.int32 and np.array_equal(sample.rows.numpy(), rows)
            assert np.array_equal(sample.ep_ids, rows)
            np.testing.assert_allclose(sample.is_weight.numpy(), w, rtol=1e-6)
            assert torch.equal(sample["obs"], buf["obs"][rows])
            td = rs.uniform(0.0, 40.0 if k == 3 else 1.0, size=B).astype(np.float32)
            td = td[np.unique(rows, return_inverse=True)[1]]  # duplicated slots carry one error
            buf.update_priorities(sample, torch.from_numpy(td))
            max_p = PR.update(prio, max_p, rows, td)
            np.testing.assert_array_equal(buf.priorities.numpy(), prio.astype(np.float32))
            assert float(buf.max_priority) == np.float32(max_p)
    assert max_p > 1.0 and draws >= 3 and live == size


def test_host_whole_buffer_shortcut():
    buf = _buffer(8)
    buf.insert_episode_batch(_episodes(4), errors=np.asarray([0.5, 0.0, 2.0, 1.0], np.float32))
    before = buf.priorities.clone()
    s = buf.sample(4)
    assert s.rows.tolist() == [0, 1, 2, 3] and s.is_weight.tolist() == [1.0] * 4 and list(s.ep_ids) == [0, 1, 2, 3]
    assert buf.beta == PR.BETA and buf.draws == 0  # no draw, no annealing, as the reference returns first
    assert torch.equal(buf.priorities, before)
    buf.update_priorities(s, torch.tensor([0.0, 1.0, 0.0, 3.0]))
    np.testing.assert_allclose(buf.priorities[:4].numpy(), PR.priority([0.0, 1.0, 0.0, 3.0]).astype(np.float32))
    assert float(buf.max_priority) == np.float32(PR.priority(3.0))


def test_host_beta_anneals_to_the_clamp():
    buf = _buffer(8)
    buf.insert_episode_batch(_episodes(6))
    buf.beta, buf.beta_increment_per_sampling = 0.9, 0.04
    seen = []
    for _ in range(5):
        seen.append(buf.sample(2).is_weight)
        assert buf.beta <= 1.0
    assert buf.beta == 1.0 and buf.draws == 5
    assert all(torch.equal(w, torch.ones(2)) for w in seen)  # flat priorities: every weight is the maximum


def test_host_heavy_slot_is_drawn_repeatedly():
    buf = _buffer(16, seed=2)
    buf.insert_episode_batch(_episodes(16))
    buf.priorities[:] = 1.0
    buf.priorities[5] = 135.0  # 90 % of the mass
    s = buf.sample(10)
    rows, w, margin = PR.sample(buf.priorities.numpy(), 16, 10, 2, 0, buf.beta)
    assert margin > PC.NEAR_TIE and np.array_equal(s.rows.numpy(), rows)
    assert int((s.rows == 5).sum()) >= 8 and float(s.is_weight[s.rows == 5][0]) < 1.0
    np.testing.assert_allclose(s.is_weight.numpy(), w, rtol=1e-6)


def test_errors_must_match_the_batch():
    buf = _buffer(8)
    with pytest.raises(ValueError, match="errors has 2 entries for 3 episodes"):
        buf.insert_episode_batch(_episodes(3), errors=np.zeros(2, np.float32))


# ---- dispatch and ABI --------------------------------------------------------------------------------------------------
def test_describe_gains_per_only_with_per(monkeypatch):
    from maleague import _native
    lib = _native.load()
    sites = set()
    for pc in PC.LEARNER_CASES:
        for k, v in pc.env.items():
            monkeypatch.setenv(k, v)
        off, on = PC.learner_cfg(pc, 0), PC.learner_cfg(pc, 1)
        assert _native.qlearner_describe(off) == pc.case.arm
        assert _native.qlearner_describe(on) == pc.case.arm + " + per"
        w0, w1 = (lib.mlg_qlearner_workspace_floats(_native.byref(c)) for c in (off, on))
        rm = off.B * (off.T - 1)
        assert w0 > 0 and w1 == w0 + (rm + 3) // 4 * 4
        for k in pc.env:
            monkeypatch.delenv(k)
        sites.add(PC.TD_SITE[pc.id])
    assert sites == {"mix_td_kernel", "mix_td1_kernel", "mix_td2_kernel", "iql_td_kernel"}


def test_default_cfg_is_unchanged():
    """A cfg built the old way (no per field given) describes and sizes as before; per = 2 is refused by name."""
    from maleague import _native
    lib = _native.load()
    for cid in ("split-h64-3v3", "generic-h128-9v9", "iql-h128-2v2"):
        c = LA.case(cid)
        cfg = LA.learner_cfg(LA.case_args(c, "cpu"), LA.dims(c)[3])
        assert cfg.per == 0 and _native.qlearner_describe(cfg) == c.arm
    cfg.per = 2
    assert lib.mlg_qlearner_workspace_floats(_native.byref(cfg)) == -1
    assert b"per=2 unsupported" in lib.mlg_last_error()


def test_struct_layout_of_the_new_fields():
    from maleague import _native
    C, Bf = _native.MlgLearnerCfg, _native.MlgLearnerBufs
    assert C._fields_[-1][0] == "per" and C.per.offset == C.distinct.offset + 4 == 84 and ctypes.sizeof(C) == 88
    assert [n for n, _ in Bf._fields_[-3:]] == ["host_rows", "is_weight", "td_abs"]
    assert Bf.is_weight.offset == Bf.host_rows.offset + 8 and Bf.td_abs.offset == Bf.is_weight.offset + 8
    assert ctypes.sizeof(Bf) == ctypes.sizeof(_native.MlgBatch) + 11 * 8
    # positional construction as the existing callers do it: the new fields are zero / NULL
    b = Bf(_native.MlgBatch(), 1, 2, 3, 4, 5, 6, None, None, None)
    assert b.is_weight is None and b.td_abs is None and b.stats == 6
    for name, n in (("mlg_per_sample", 11), ("mlg_per_insert", 9), ("mlg_per_update", 9)):
        assert len(_native.SIGNATURES[name][1]) == n and hasattr(_native.load(), name)
    assert _native.load().mlg_per_max_slots() >= 65536 > _native.load().mlg_per_lds_slots() >= 5000


def test_host_checks_name_what_they_refuse():
    """Launch nothing: every refusal is a host check (pointers are never dereferenced on the host)."""
    from maleague import _native
    lib = _native.load()
    big = lib.mlg_per_max_slots() + 1
    assert lib.mlg_per_sample(8, big, 4, 0, 0, 0.4, 8, 8, None, 0, None) != 0
    assert f"episodes_in_buffer={big} unsupported".encode() in lib.mlg_last_error()
    assert lib.mlg_per_sample(8, 100, 4097, 0, 0, 0.4, 8, 8, None, 0, None) != 0
    assert b"batch_size=4097 unsupported" in lib.mlg_last_error()
    n = lib.mlg_per_lds_slots() + 1
    assert lib.mlg_per_sample(8, n, 4, 0, 0, 0.4, 8, 8, None, 0, None) != 0
    assert b"needs scan_workspace" in lib.mlg_last_error()
    assert lib.mlg_per_sample(8, n, 4, 0, 0, 0.4, 8, 8, 16, n - 1, None) != 0
    assert b"needs scan_workspace" in lib.mlg_last_error()
    assert lib.mlg_per_sample(8, 10, 4, 0, 0, 1.5, 8, 8, None, 0, None) != 0 and b"beta" in lib.mlg_last_error()
    assert lib.mlg_per_insert(8, 10, 10, 1, None, 0.01, 0.6, 8, None) != 0 and b"slot0=10" in lib.mlg_last_error()
    assert lib.mlg_per_insert(8, 10, 0, 11, None, 0.01, 0.6, 8, None) != 0 and b"count=11" in lib.mlg_last_error()
    assert lib.mlg_per_update(8, 4, None, 8, 5, 0.01, 0.6, 8, None) != 0 and b"identity rows" in lib.mlg_last_error()
    assert lib.mlg_per_update(None, 4, None, 8, 4, 0.01, 0.6, 8, None) != 0 and b"null pointer" in lib.mlg_last_error()


def test_refil_and_coma_learners_refuse_by_name():
    from maleague.learners import COMALearner, REFILLearner
    for cls, args in ((REFILLearner, refil_args(prioritized_replay=True)),
                      (COMALearner, qmix_args(prioritized_replay=True))):
        with pytest.raises(ValueError, match=f"{cls.__name__}: prioritized_replay=True is not supported"):
            cls(None, None, None, args)


def test_experiment_builds_the_prioritized_buffer():
    """MultiAgentExperiment._build_learners reads prioritized_replay and the per_* keys with their defaults."""
    import inspect
    from maleague.runs import ma_experiment
    src = inspect.getsource(ma_experiment.MultiAgentExperiment._build_learners)
    for key in ("prioritized_replay", "per_alpha", "per_eps", "per_beta", "per_beta_increment"):
        assert f'getattr(a, "{key}"' in src
