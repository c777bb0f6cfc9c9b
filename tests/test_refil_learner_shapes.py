"""The conditions on the REFIL learner's case table (tests/refil_learner_shapes.py), checked on the CPU with the float64
oracle alone, and the oracle's entity_last_action = False branch pinned to the reference's own call
(tests/golden/refil_learner_nola.npz, made by tests/golden/make_refil_golden.py nola). No kernel runs here."""
import numpy as np
import pytest
import torch

import refil_learner_shapes as RS
import refil_ref as RR
from helpers import Q_TOL


def test_table_is_complete():
    assert len(set(RS.IDS)) == len(RS.IDS) == 23
    assert set(RS.ORACLE_F64) == set(RS.GRAD_D32) == set(RS.REACHES) == set(RS.IDS)
    assert RS.Q_TOL == Q_TOL == 1e-4
    for c in RS.CASES:
        assert 1 <= c.NA <= 8 and c.NA <= c.NE <= 16 and 1 <= c.A <= 32  # check_cfg of csrc/refil_learner.hip
        assert c.ED + (c.A if c.last_action else 0) <= RS.KMAX
        assert len(c.lens) == c.B and max(c.lens) + 1 < c.T  # max_t_filled < T: a stored step past every episode
        assert len(RS.GRAD_D32[c.id]) == (13 if c.mixer == "vdn" else 41)
        assert (c.id in RS.CLIPPED) == c.id.endswith("-clip") == (c.reward_scale > 1)
        assert c.id.startswith("attn-") == (c.agent == RS.PLAIN)


@pytest.mark.parametrize("cid", RS.IDS)
def test_case_reaches_what_its_comment_claims(cid):
    """D0, K1, Ap, the parity of B * T, Ron against the four- and 16-row tiles, the set of mix_len values and the mask
    path, recomputed from the table; and the batch itself: lengths, the never-filled and one-transition episodes,
    half the episodes terminated, an available action everywhere it is read."""
    c = RS.case(cid)
    arrs = RS.case_arrays(c)
    got = RS.derived(c, arrs)
    for k, v in RS.REACHES[cid].items():
        assert got[k] == v, f"{cid}: {k} is {got[k]}, the table claims {v}"
    filled = arrs["filled"][:, :, 0]
    assert filled.sum(axis=1).tolist() == [n + 1 for n in c.lens]
    assert got["Te"] == max(c.lens) + 1 < c.T
    if cid not in ("t130", "twords"):  # the two cases whose lengths are the point
        assert -1 in c.lens and 1 in c.lens
    n_term = int(arrs["terminated"].sum())
    assert n_term == sum(1 for b, n in enumerate(c.lens) if b % 2 == 0 and n >= 1) and abs(2 * n_term - c.B) <= 2
    live = RS.live_mask(arrs)
    assert RS.mask_sum(arrs) == live.sum() > 0
    n_avail = arrs["avail_actions"].sum(-1)
    for b, n in enumerate(c.lens):  # a never-filled episode is all zero; the step after a live transition has actions
        if n < 0:
            assert all(not v[b].any() for v in arrs.values())
        for t in np.flatnonzero(live[b]):
            assert (n_avail[b, t] >= 1).all() and (n_avail[b, t + 1] >= 1).all()
    assert np.array_equal(np.take_along_axis(arrs["avail_actions"], arrs["actions"], -1)[filled != 0],
                          np.ones_like(arrs["actions"])[filled != 0])
    if c.reward_scale != 1:
        assert abs(arrs["reward"]).max() > 50
    # the last action is taken somewhere it counts: the last input column (D0 - 1, column 47 of the K1 = 48 cases)
    # carries a one and the last action's Q is a chosen Q. A wrong last column passed unnoticed on a batch without.
    assert RS.last_action_picks(c, arrs) >= 1


@pytest.mark.parametrize("cid", RS.IDS)
def test_case_gap_and_grad_norm(cid):
    """The float64 oracle: the smallest top-two gap of the masked online Q is at least Q_TOL (a flipped double-Q pick
    would move a target by a jump), the first-call grad_norm is above 20 for the -clip cases and below 5 elsewhere,
    and both are the figures written in the table."""
    c = RS.case(cid)
    stats, ref, grads, gap = RS.run_oracle(c, torch.float64)
    gn = stats[0]["grad_norm"]
    print(f"  {cid}: gap {gap:.2e}, grad_norm {gn:.4g}")
    assert gap >= RS.Q_TOL
    assert gn > 20 if cid in RS.CLIPPED else gn < 5
    assert RS.clips(cid) == (cid in RS.CLIPPED)
    np.testing.assert_allclose([gap, gn], RS.ORACLE_F64[cid][2:], rtol=6e-3)  # written with three digits
    assert ref.last_target_update_episode == 200 and len(grads) == len(ref.params) == len(RS.GRAD_D32[cid])
    assert ("im_loss" in stats[0]) == (c.agent == RS.IMAGINE)
    for k in ref.agent:  # the third call ended with the sync
        assert torch.equal(ref.agent[k].detach(), ref.t_agent[k])


def test_oracle_dtype_is_explicit():
    """Every float tensor of the float64 oracle is float64 (parameters, RMSprop state, gradients), whatever the
    batch's dtype; last_grads is the gradient before the clip."""
    c = RS.case("k48-a32-clip")
    stats, ref, grads, _ = RS.run_oracle(c, torch.float64, calls=RS.CALLS[:1])
    assert all(p.dtype == torch.float64 for p in ref.params) and all(g.dtype == torch.float64 for g in grads)
    assert all(st["square_avg"].dtype == torch.float64 for st in ref.opt.state.values())
    norm = float(torch.sqrt(sum((g ** 2).sum() for g in grads)))
    np.testing.assert_allclose(norm, stats[0]["grad_norm"], rtol=1e-12)
    assert norm > RS.CLIP  # clipped: .grad was scaled after last_grads was taken
    kept = float(torch.sqrt(sum((p.grad ** 2).sum() for p in ref.params)))
    np.testing.assert_allclose(kept, RS.CLIP, rtol=1e-6)
    s32, r32, g32, _ = RS.run_oracle(c, torch.float32, calls=RS.CALLS[:1])
    assert all(p.dtype == torch.float32 for p in r32.params) and all(g.dtype == torch.float32 for g in g32)


def test_oracle_without_last_action_matches_reference(golden):
    """REFILLearnerRef with entity_last_action False against one REFILLearner.train call of the reference at NA 5,
    NE 9, ED 8, A 16 (the nola-a16 shape); the figures of test_refil_oracle.py::test_refil_learner_two_calls."""
    d, after = golden("refil_learner_nola.npz"), golden("refil_learner_nola_after.npz")
    na, ne, ed, A = (int(x) for x in d["dims"])
    assert (na, ne, ed, A) == RS.case("nola-a16")[3:7]
    from helpers import refil_args
    a = refil_args(device="cpu", n_agents=na, n_entities=ne, n_actions=A, entity_shape=ed, entity_last_action=False)
    pre = lambda z, p: {k[len(p):]: torch.from_numpy(np.array(z[k])) for k in z.files if k.startswith(p)}  # noqa: E731
    batch = pre(d, "b.")
    agent_p = pre(d, "p0.agent.")
    assert agent_p["fc1.weight"].shape == (64, ed)  # no one-hot columns
    L = RR.REFILLearnerRef(agent_p, pre(d, "p0.mixer."), a)
    st = L.train(batch, torch.from_numpy(d["c0.groupA"]), episode_num=0)
    for k, v in st.items():
        np.testing.assert_allclose(v, float(d[f"c0.stat.{k}"]), rtol=1e-4, atol=1e-6, err_msg=k)
    for k, v in L.agent.items():
        np.testing.assert_allclose(v.detach().numpy(), after[f"c0.agent.{k}"], atol=2e-5, rtol=0, err_msg=k)
    for k, v in L.mixer.items():
        np.testing.assert_allclose(v.detach().numpy(), after[f"c0.mixer.{k}"], atol=2e-5, rtol=0, err_msg=k)
    assert len(L.mixer) == 28
