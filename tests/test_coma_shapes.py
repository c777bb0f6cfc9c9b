"""The COMA shape cases on the CPU (no GPU call): the dispatch of mlg_rollout_policy pinned through the host-only query
(mlg_rollout_policy_describe), the coverage the case tables claim, the properties each critic case is named for, the
fp32 noise floors that set the GPU tolerances (tests/coma_shapes.py), and -- on the restatement side -- that the
comparisons of tests/test_gpu_coma_shapes.py would notice the defects they target: a restatement with the defect lies
outside the case's tolerance of the float64 one."""
import numpy as np
import pytest

import coma_ref as CR
import coma_shapes as CS
from helpers import DELTA, NEAR_TIE_CAP, drqn_dims, shape_plan

LDS_LIMIT = 160 * 1024


# ---- mlg_rollout_policy_describe ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CS.POLICY_CASES + [CS.LEARNER_CASE], ids=CS.POLICY_IDS + [CS.LEARNER_CASE.id])
def test_policy_case_arm(c):
    name, lds = CS.policy_describe(c)
    assert name == c.arm
    assert 0 < lds <= LDS_LIMIT
    assert (lds > 32 * 1024) == name.startswith("policy-lds")  # the weights' image is what fills LDS


def _describe(plan, hidden):
    return CS.policy_describe(CS.PolicyCase("x", hidden, plan, "", 0, 1.0, ()))


def test_policy_cases_cover_every_reachable_instantiation():
    """Every (H, TPW, WLDS) the default environment reaches with a K-vs-K plan (K = 1..32), `large` or an asymmetric
    plan has a case; between them the cases run every TPW with both weight placements, one to five action tiles and
    all three H. Not reached: policy-lds at H = 128 and policy-lds/tpw2..4 at H = 64 (the weights' image does not fit
    next to the env state), policy-global at H = 32 (it always fits)."""
    have = {(c.H, c.arm) for c in CS.POLICY_CASES}
    reached = set()
    for hidden in (32, 64, 128):
        for plan in [f"{k}v{k}" for k in range(1, 33)] + ["large", "5v7", "3v5", "medium_1h_4t", "small"]:
            reached.add((hidden, _describe(plan, hidden)[0]))
    assert reached == have
    arms = {c.arm for c in CS.POLICY_CASES}
    assert arms == {f"policy-{w}/tpw{k}" for w in ("lds", "global") for k in (1, 2, 3, 4)}
    assert {c.H for c in CS.POLICY_CASES} == {32, 64, 128}
    tiles = {c.id: CS.n_action_tiles(CS.policy_spec(c).n_actions) for c in CS.POLICY_CASES}
    assert set(tiles.values()) == {1, 2, 3, 4, 5}
    # the masked greedy run goes on every case, the unmasked one on at least one case per action-tile count
    assert all(True in c.greedy for c in CS.POLICY_CASES)
    assert {tiles[c.id] for c in CS.POLICY_CASES if False in c.greedy} == {1, 2, 3, 4, 5}
    # the ring-mode equality: one case per agent-tiles-per-wave count
    assert sorted(CS.policy_case(cid).arm[-1] for cid in CS.RING_CASES) == ["1", "2", "3", "4"]
    assert CS.ORACLE_NEAR_TIE_CAP == 0.01 and NEAR_TIE_CAP == 0.02 and CS.DELTA == DELTA == 2e-4


def test_fifth_action_tile_is_admitted_and_a_sixth_refused():
    from maleague import _native
    from maleague.envs.teams_env import TeamsEnvSpec
    c = CS.policy_case("lds4-h32-30v30")
    spec = CS.policy_spec(c)
    assert spec.n_actions == 65 and CS.policy_describe(c)[0] == "policy-lds/tpw4"
    assert _describe("32v32", 64)[0] == "policy-global/tpw4"  # the largest plan: A = 69, the last column of tile 4
    dims = drqn_dims(spec, 32)
    dims.n_actions, dims.d_in = 81, dims.d_in + 16  # a sixth tile: no env has it (A = 5 + U <= 69), the dims check refuses
    with pytest.raises(_native.NativeError, match="agent dims do not match"):
        _native.rollout_policy_describe(spec.to_c(), dims)
    small = TeamsEnvSpec.from_env_args({"match_build_plan": shape_plan("small")})
    for hidden in (16, 48, 256):
        with pytest.raises(_native.NativeError, match="rnn_hidden_dim"):
            _native.rollout_policy_describe(small.to_c(), drqn_dims(small, hidden))
    lib = _native.load()
    import ctypes
    name, lds = ctypes.create_string_buffer(4), ctypes.c_int64(0)
    d = drqn_dims(small, 64)
    assert lib.mlg_rollout_policy_describe(_native.byref(small.to_c()), _native.byref(d), name, len(name),
                                           ctypes.byref(lds)) != 0
    assert b"name buffer" in lib.mlg_last_error()
    assert lib.mlg_rollout_policy_describe(_native.byref(small.to_c()), _native.byref(d), None, 0, None) != 0


# ---- the critic cases: what each is named for -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def critic_runs():
    """The float64 and fp32 restatements of every critic case, two calls each: computed once."""
    return {c.id: (CS.run_critic_ref(c, np.float64), CS.run_critic_ref(c, np.float32)) for c in CS.CRITIC_CASES}


def test_critic_cases_have_the_properties_they_claim(critic_runs):
    from maleague import _native
    lib = _native.load()
    by = {c.id: c for c in CS.CRITIC_CASES}
    for c in CS.CRITIC_CASES:
        cfg = _native.MlgComaCfg(B=c.B, T=c.T, N=c.N, A=c.A, d_obs=c.d_obs, S=c.S, hidden=128)
        n = lib.mlg_coma_param_count(_native.byref(cfg))
        assert n > 0 and (n + 255) // 256 == CS.critic_blocks(c)
        pc, store, slots, batch = CS.critic_data(c)
        assert batch["obs"].shape[:3] == (c.B, c.T, c.N) and sum(v.size for v in pc.values()) == n
        assert all(r["taken"] > 0 for r in critic_runs[c.id][0])
    assert by["A96"].A == 96 and CS.critic_blocks(by["A96"]) == 314 > 256          # six fc3 tiles, two norm passes
    assert all(CS.critic_blocks(c) <= 256 for c in CS.CRITIC_CASES if c.id != "A96")
    assert (by["A16"].A, by["A17"].A, by["A33"].A) == (16, 17, 33)
    r = by["R272"]
    assert r.B * r.N == 272 > 256 and r.B * (r.T - 1) == 272 > 256
    _, _, _, rb = CS.critic_data(r)
    filled = rb["filled"][:, :, 0].sum(axis=1)
    assert filled[0] == 0 and not any(v[0].any() for v in rb.values())           # never filled
    assert filled[1] == 2 and rb["terminated"][1, 0, 0] == 1                     # one transition
    assert len(set(filled.tolist())) >= 8 and filled.max() == r.T                # mixed, one to the limit
    assert critic_runs["R272"][0][0]["taken"] == 8
    assert (by["N32"].N, by["N32"].B, by["N1"].N) == (32, 1, 1)
    t = by["Tm258"]
    assert t.T - 1 == 258 > 256 and critic_runs["Tm258"][0][0]["taken"] == 258 and list(t.lengths) == [258, 3]
    for call in critic_runs["clip"][0]:                                          # coef < 1 at every step
        assert len(call["norms"]) == call["taken"] == 3 and min(call["norms"]) > 10.0 + 1e-3
    for cid in CS.CRITIC_IDS:                                                    # ... and at no step elsewhere,
        if cid not in ("clip", "Tm258"):                                         # Tm258's early steps aside
            assert max(n for call in critic_runs[cid][0] for n in call["norms"]) < 10.0, cid
    s = by["stride"]
    n_store, T1, slots = s.store
    assert T1 == 9 > s.T == 6 and n_store > s.B == len(slots) and slots != sorted(slots)
    _, store, _, sb = CS.critic_data(s)
    assert store["obs"].shape[:2] == (5, 9) and int(sb["filled"].sum(axis=1).max()) == s.T  # cut to the longest
    assert CS.ZERO_WORKSPACE_CASE in CS.CRITIC_IDS


def test_fp32_restatement_stays_within_the_recorded_floors(critic_runs):
    for c in CS.CRITIC_CASES:
        r64, r32 = critic_runs[c.id]
        d = CS.distance(r32, r64, CS.CRITIC_KEYS)
        print(c.id, {k: f"{v:.3g}" for k, v in d.items()})
        for k, floor in zip(CS.CRITIC_KEYS, c.floors):
            assert 0 < floor and d[k] <= 1.05 * floor, (c.id, k, d[k], floor)
            # the floor is rounding noise: far below the quantity itself
            assert floor <= 1e-6 * max(1.0, max(float(np.abs(r[k]).max()) for r in r64)), (c.id, k)


@pytest.fixture(scope="module")
def learner_runs():
    spec, batch, ep_len = CS.learner_oracle_batch()
    return spec, batch, ep_len, CS.run_learner_ref(batch, spec, np.float64), CS.run_learner_ref(batch, spec, np.float32)


def test_learner_case_is_cut_below_its_storage_and_within_its_floors(learner_runs):
    spec, batch, ep_len, r64, r32 = learner_runs
    assert batch["obs"].shape[1] == ep_len.max() + 1 < CS.LEARNER_LIMIT + 1   # max_seq_length below the storage length
    assert len(set(ep_len.tolist())) > 1
    d = CS.distance(r32, r64, CS.LEARNER_KEYS)
    print({k: f"{v:.3g}" for k, v in d.items()})
    for k, floor in zip(CS.LEARNER_KEYS, CS.LEARNER_FLOORS):
        assert 0 < floor and d[k] <= 1.05 * floor, (k, d[k], floor)


# ---- the comparisons notice the defects they target -----------------------------------------------------------------
@pytest.mark.parametrize("cid,defect,key", [("R272", "stats_rows_256", "critic_stats"),
                                            ("R272", "target_rows_256", "targets"),
                                            ("R272", "masks_256", "targets"),
                                            ("A96", "norm_blocks_256", "critic_stats"),
                                            ("Tm258", "masksum_256", "q_vals")])
def test_a_forgotten_second_pass_leaves_the_tolerance(critic_runs, cid, defect, key):
    c = CS.critic_case(cid)
    bad = CS.run_critic_ref(c, np.float64, defect=defect)
    d = CS.distance(bad, critic_runs[cid][0], CS.CRITIC_KEYS)
    assert d[key] > 100 * CS.critic_tol(c)[key], (cid, defect, d)
    small = CS.critic_case("A17")  # below every 256 boundary the same defect changes nothing
    if defect != "masksum_256":
        same = CS.distance(CS.run_critic_ref(small, np.float64, defect=defect), critic_runs["A17"][0], CS.CRITIC_KEYS)
        assert max(same.values()) < 1e-12  # the norm is summed in another order, nothing else differs


def test_wrong_action_tile_or_unclipped_step_leaves_the_tolerance(critic_runs):
    """fc3 rows of the sixth action tile dropped (A96), the A = 17 column dropped, the clip left out."""
    for cid, lo in (("A96", 80), ("A17", 16), ("A33", 32)):
        c = CS.critic_case(cid)
        pc, _, _, batch = CS.critic_data(c)
        pc = {k: v.copy() for k, v in pc.items()}
        pc["fc3.weight"][lo:] = 0
        pc["fc3.bias"][lo:] = 0
        q = CR.CriticRef(pc).train(batch)[0]
        assert np.abs(q - critic_runs[cid][0][0]["q_vals"]).max() > 100 * CS.critic_tol(c)["q_vals"]
    c = CS.critic_case("clip")
    pc, _, _, batch = CS.critic_data(c)
    ref = CR.CriticRef(pc, clip=1e30)
    ref.train(batch)
    flat = np.concatenate([ref.p[k].reshape(-1) for k in CR.CRITIC_KEYS])
    # RMSprop normalises the first step, so the unclipped parameters differ only through the later steps: still far out
    assert np.abs(flat - critic_runs["clip"][0][0]["critic_params"]).max() > 100 * CS.critic_tol(c)["critic_params"]
    s = CS.critic_case("stride")  # the store read with stride cfg.T instead of T1: other bytes
    pc, store, slots, batch = CS.critic_data(s)
    wrong = {k: v.reshape((-1,) + v.shape[2:])[:len(slots) * s.T].reshape((len(slots), s.T) + v.shape[2:])
             for k, v in store.items()}
    assert not np.array_equal(wrong["obs"], batch["obs"])


def _draw(m, on, u, reset_at_tiles=False):
    """The multinomial rule over a row of masked probabilities (float64); reset_at_tiles: the running sum restarts at
    every 16-wide action tile (a kernel that lost the cross-tile carry)."""
    total = m.sum()
    run = 0.0
    for k in np.nonzero(on)[0]:
        if reset_at_tiles and k % 16 == 0:
            run = 0.0
        run += m[k]
        if run > u * total:
            return int(k)
    return int(np.nonzero(on)[0][-1])


@pytest.mark.parametrize("A", [23, 39, 55, 65])
def test_the_cdf_rule_notices_a_lost_tile_carry_and_a_first_tile_argmax(A):
    """The checker's rule (helpers._check_policy_run: lo - DELTA <= u * total < cdf[a] + DELTA) holds for every draw of
    the rule itself and fails for draws whose running sum restarts at a tile edge; the greedy rule fails for an argmax
    over the first tile only."""
    rng = np.random.RandomState(A)
    bad_draws = bad_greedy = 0
    for _ in range(200):
        on = rng.rand(A) < 0.6
        on[rng.randint(A)] = True
        m = np.where(on, rng.dirichlet(np.ones(A)), 0.0)
        u = float(rng.rand())
        cdf = np.cumsum(m)
        ok = lambda a: (cdf[a - 1] if a > 0 else 0.0) - DELTA <= u * cdf[-1] < cdf[a] + DELTA  # noqa: E731
        assert ok(_draw(m, on, u))
        bad_draws += not ok(_draw(m, on, u, reset_at_tiles=True))
        srt = np.sort(m)
        if srt[-1] - srt[-2] >= DELTA:
            bad_greedy += int(np.argmax(m[:16])) != int(np.argmax(m))
    assert bad_draws > 20 and bad_greedy > 20


def test_actor_cases():
    rows = {cid: B * Tm * N for cid, B, Tm, N, A in CS.ACTOR_CASES}
    assert rows["R360"] == 360 > 256 and rows["R1"] == 1 and rows["R1pad"] == 2
    assert {A for *_, A in CS.ACTOR_CASES} >= {1, 96}
    for cid, B, Tm, N, A in CS.ACTOR_CASES:
        pi, avail, actions, q, mask = CS.actor_inputs(B, Tm, N, A)
        pad = ~avail.any(axis=-1)
        assert mask.sum() > 0
        if cid != "R1":
            assert pad.any() and not mask[pad.any(axis=-1)].any()
    # a loss kernel that stopped after one pass of its 256-thread stride loop: rows 256.. of R360 dropped from the sums
    import torch
    pi, avail, actions, q, mask = CS.actor_inputs(9, 8, 5, 11)
    t = lambda *a: [torch.tensor(x) for x in a]  # noqa: E731
    full = CR.actor_loss_torch(*t(pi, avail, actions, q, mask))
    cut = mask.copy()
    cut.reshape(-1)[256 // 5 + 1:] = 0  # mask entries of the (b, t) rows past flat agent row 256
    part = CR.actor_loss_torch(*t(pi, avail, actions, q, cut))
    num = lambda r: np.array([float(r[0] * r[3]), float(r[1] * r[3]), float(r[2] * r[3])])  # noqa: E731
    assert (np.abs(num(full) - num(part)) > 1e-2 * np.abs(num(full))).all()  # the sums, against rtol 2e-5
