"""The DRQN / QMixer op shape cases on the CPU (no GPU call): the conditions tests/drqn_op_shapes.py lists, asserted on
the oracle's values alone, the properties each case is named for, and the host-side size queries
(mlg_qmix_backward_workspace_floats, mlg_agent_backward_workspace_floats, mlg_packed_agent_size).

Condition 3 is what makes the GPU bound meaningful: the fp32 CPU oracle, which sums in its own order, must itself lie
within a quarter of 1e-4 max(1, max|y64|) of the float64 oracle, per tensor (`pytest -s` prints the shares)."""
import numpy as np
import pytest
import torch

import drqn_op_shapes as DS
import learner_ref as LR
from test_gpu_autograd import agent_reference, mixer_reference

f64, f32 = torch.float64, torch.float32


def _oracle_share(name, ref32, ref64):
    """Condition 3 for one tensor; returns the fp32 oracle's share of the bound."""
    err = float((ref32.detach().to(f64) - ref64.detach()).abs().max()) if ref64.numel() else 0.0
    bound = DS.bound_of(ref64)
    assert err <= DS.ORACLE_SHARE * bound, f"{name}: fp32 oracle {err:.3e} from float64, bound {bound:.3e}"
    return err / bound


# ---- A ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", DS.FWD_A)
@pytest.mark.parametrize("H", DS.FWD_H)
def test_agent_forward_cases(H, A):
    assert DS.fwd_d_in(A) % 16 != 0
    p = DS.fwd_params(H, A)
    cases = DS.fwd_inputs(H, A)
    assert [R for R, _, _ in cases] == list(DS.FWD_R) + [DS.FWD_R_NULL]
    assert [h is None for _, _, h in cases] == [False] * len(DS.FWD_R) + [True]
    worst = 0.0
    for R, x, h in cases:
        q64, h64 = DS.fwd_reference(p, x, h, f64)
        q32, h32 = DS.fwd_reference(p, x, h, f32)
        assert tuple(q64.shape) == (R, A) and tuple(h64.shape) == (R, H)
        worst = max(worst, _oracle_share(f"q R={R}", q32, q64), _oracle_share(f"h' R={R}", h32, h64))
    print(f"agent forward H={H} A={A}: fp32 oracle at most {worst:.2%} of the bound")


def test_agent_forward_table_reaches_the_edges_it_names():
    tiles = [(A + 15) // 16 for A in DS.FWD_A]
    assert tiles == [1, 1, 2, 5] and 16 in DS.FWD_A and 17 in DS.FWD_A
    assert set(DS.FWD_H) == {32, 64, 128}
    assert {1, 15, 16, 17} <= set(DS.FWD_R) and max(DS.FWD_R) > 64  # past one 4-tile workgroup


# ---- B ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", DS.MAC_IDS)
def test_mac_forward_cases(cid):
    c = DS.mac_case(cid)
    assert c.B * c.N == DS.MAC_ROWS[cid]
    p = DS.mac_params(c)
    assert p["fc1.weight"].shape == (c.H, DS.mac_d_in(c))
    tb, h0 = DS.mac_inputs(c)
    assert tb["obs"].shape == (c.B, DS.MAC_T1, c.N, DS.MAC_D_OBS) and h0.shape == (c.B * c.N, c.H)
    q64, h64 = DS.mac_reference(c, p, tb, h0, f64)
    q32, h32 = DS.mac_reference(c, p, tb, h0, f32)
    assert tuple(q64.shape) == (c.B, DS.MAC_T1, c.N, c.A)
    share = max(_oracle_share("q", q32, q64), _oracle_share("h", h32, h64))
    print(f"mac forward {cid}: fp32 oracle at most {share:.2%} of the bound")
    if c.last_action:  # the last action matters: the unroll without it differs by far more than the bound
        off = LR.mac_unroll({k: v.double() for k, v in p.items()},
                            {"obs": tb["obs"].double(), "actions_onehot": torch.zeros_like(tb["actions_onehot"]).double()},
                            c.N, h0=h0.double(), last_action=True, agent_id=c.agent_id)[0]
        assert float((off - q64)[:, 1:].abs().max()) > 100 * DS.bound_of(q64)
        assert torch.equal(off[:, 0], q64[:, 0])  # t = 0 reads no last action


def test_mac_table_reaches_the_edges_it_names():
    flags = {(c.last_action, c.agent_id) for c in DS.MAC_CASES}
    assert flags == {(True, True), (False, True), (True, False), (False, False)}
    obs_only = DS.mac_case("h64-obs-only")
    assert DS.mac_d_in(obs_only) == DS.MAC_D_OBS
    rows = sorted(DS.MAC_ROWS.values())
    assert rows == [15, 16, 18, 33, 35, 63] and sum(r % 16 != 0 for r in rows) == 5
    assert {c.H for c in DS.MAC_CASES} == {32, 64, 128}
    assert max(DS.SAMPLED_ROWS) == DS.SAMPLED_SLOTS - 1 and len(set(DS.SAMPLED_ROWS)) < len(DS.SAMPLED_ROWS)
    assert DS.SAMPLED_ROWS != sorted(DS.SAMPLED_ROWS)
    assert not DS.mac_case(DS.MODULE_PATH_CASE).last_action


# ---- C ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixer_refs():
    """float64 (conditions 1 and 2 asserted inside) and fp32 gradients and values of every (case, R): computed once."""
    out = {}
    for c in DS.MIXER_CASES:
        for R in DS.MIXER_R:
            mp, qs, st, g_out = DS.mixer_inputs(c, R)
            g64 = mixer_reference(mp, qs, st, g_out, c.layers, c.N, f64, check=True, S_DIM=c.S, E_DIM=c.E)
            g32 = mixer_reference(mp, qs, st, g_out, c.layers, c.N, f32, S_DIM=c.S, E_DIM=c.E)
            out[c.id, R] = (g64, g32, DS.mixer_forward_reference(c, mp, qs, st, f64),
                            DS.mixer_forward_reference(c, mp, qs, st, f32))
    return out


@pytest.mark.parametrize("R", DS.MIXER_R)
@pytest.mark.parametrize("cid", DS.MIXER_IDS)
def test_mixer_cases(mixer_refs, cid, R):
    c = DS.mixer_case_of(cid)
    g64, g32, y64, y32 = mixer_refs[cid, R]
    mp, qs, st, g_out = DS.mixer_inputs(c, R)
    assert sum(v.numel() for v in mp.values()) == DS.mixer_param_count(c)
    assert set(g64) == set(mp) | {"d_agent_qs"} and tuple(y64.shape) == (R,)
    share = _oracle_share("q_tot", y32, y64)
    for k in g64:
        assert g64[k].abs().max() > 0, k
        share = max(share, _oracle_share(k, g32[k], g64[k]))
    print(f"mixer {cid} R={R} seed {DS.mixer_seed(cid, R)}: fp32 oracle at most {share:.2%} of the bound")


def test_mixer_table_reaches_the_edges_it_names():
    by = {c.id: c for c in DS.MIXER_CASES}
    e5 = by["e5"]  # every leading dimension of a weight-gradient job: no multiple of 4
    assert all(v % 4 for v in (e5.S, e5.E, e5.HE, e5.N * e5.E))
    assert all((R * v) % 4 for R in (1, 65, 257) for v in (e5.E, e5.HE, e5.N * e5.E))  # take() pads every section
    assert by["n1"].N == 1 and by["n1"].S % 4 != 0
    big = by["e64-he256"]
    assert (big.E, big.HE) == (64, 256) and (big.N * big.E + 63) // 64 == 9 and (big.HE + 63) // 64 == 4
    assert by["n32"].N * by["n32"].E == 1024
    assert by["l1-n17-e16"].layers == 1 and by["l1-n17-e16"].N * by["l1-n17-e16"].E == 272 and by["l1-n17-e16"].S % 2
    assert by["l1-e64"].layers == 1 and by["l1-e64"].S < 16
    assert DS.MIXER_R == (1, 65, 257)


def _qmix_params(c, **kw):
    from maleague import _native
    d = dict(n_agents=c.N, state_dim=c.S, embed_dim=c.E, hypernet_embed=c.HE, hypernet_layers=c.layers)
    d.update(kw)
    return _native.MlgQMixParams(**d)


def test_qmix_backward_workspace_query():
    from maleague import _native
    lib = _native.load()
    for c in DS.MIXER_CASES:
        sizes = [lib.mlg_qmix_backward_workspace_floats(_native.byref(_qmix_params(c)), R)
                 for R in (0, 1, 2, 64, 65, 256, 257, 258)]
        assert all(n > 0 and n % 4 == 0 for n in sizes), (c.id, sizes)
        assert sizes == sorted(sizes), (c.id, sizes)
        # the row sections alone (each rounded up to 4 floats) fit in front of the partial sums
        R = 65
        rows = [R * c.E] * 4 + [R * c.N * c.E] + ([R * c.HE] * 4 if c.layers == 2 else [])
        assert sizes[4] > sum((n + 3) // 4 * 4 for n in rows), c.id
    c = DS.mixer_case_of("e64-he256")
    assert lib.mlg_qmix_backward_workspace_floats(_native.byref(_qmix_params(c, embed_dim=65)), 8) == -1
    assert b"embed dims too large" in lib.mlg_last_error()
    assert lib.mlg_qmix_backward_workspace_floats(_native.byref(_qmix_params(c, hypernet_embed=257)), 8) == -1
    assert lib.mlg_qmix_backward_workspace_floats(_native.byref(_qmix_params(c)), -1) == -1
    assert lib.mlg_qmix_backward_workspace_floats(_native.byref(_qmix_params(c)), 8) > 0


# ---- D ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", DS.AGENT_GRAD_IDS)
def test_agent_gradient_cases(cid):
    c = DS.agent_grad_case_of(cid)
    p, x, h, gq, gh = DS.agent_grad_inputs(c)
    assert p["fc1.weight"].shape == (c.H, DS.agent_grad_d_in(c)) and x.shape == (c.R, DS.agent_grad_d_in(c))
    g64 = agent_reference(p, x, h, gq, gh, f64, check=True)  # conditions 1 and 2
    g32 = agent_reference(p, x, h, gq, gh, f32)
    share = 0.0
    for k in g64:
        assert g64[k].abs().max() > 0, k
        share = max(share, _oracle_share(k, g32[k], g64[k]))
    q64, h64 = DS.fwd_reference(p, x, h, f64)
    q32, h32 = DS.fwd_reference(p, x, h, f32)
    share = max(share, _oracle_share("q", q32, q64), _oracle_share("h'", h32, h64))
    print(f"agent gradients {cid}: fp32 oracle at most {share:.2%} of the bound")


def test_agent_gradient_table_reaches_the_edges_it_names():
    by = {c.id: c for c in DS.AGENT_GRAD_CASES}
    assert [by[k].R for k in ("r64", "r65", "r257")] == [64, 65, 257]
    assert (by["h32-r65"].H, by["h128-r65"].H) == (32, 128)
    assert [by[k].A for k in ("a5", "a16", "a65")] == [5, 16, 65]
    assert {(c.last_action, c.agent_id) for c in DS.AGENT_GRAD_CASES} == {(a, b) for a in (0, 1) for b in (0, 1)}
    assert DS.agent_grad_d_in(by["obs-only"]) == DS.GRAD_D_OBS
    assert by[DS.POISON_AGENT].R == DS.POISON_R and DS.POISON_MIXER in DS.MIXER_IDS


def _agent_dims(d_obs, A, N, H, la, ai):
    from maleague import _native
    return _native.MlgAgentDims(d_obs=d_obs, n_actions=A, n_agents=N, hidden=H, d_in=d_obs + A * la + N * ai,
                                obs_last_action=la, obs_agent_id=ai)


def test_packed_agent_size_and_backward_workspace_queries():
    """The packed block of an agent without a flag lacks exactly that flag's gathered block (w1a [A][H] / w1n [N][H]);
    its dense fc1 image [H][d_in rounded up to 16] narrows with d_in. Every term is a multiple of 16 floats."""
    from maleague import _native
    lib = _native.load()
    pad = lambda v: (v + 15) // 16 * 16  # noqa: E731
    shapes = [(DS.GRAD_D_OBS, c.A, DS.GRAD_N, c.H) for c in DS.AGENT_GRAD_CASES]
    shapes += [(DS.MAC_D_OBS, c.A, c.N, c.H) for c in DS.MAC_CASES]
    shapes += [(DS.FWD_D_OBS, A, DS.FWD_N, H) for H in DS.FWD_H for A in DS.FWD_A]
    for d_obs, A, N, H in sorted(set(shapes)):
        size = {(la, ai): lib.mlg_packed_agent_size(_native.byref(_agent_dims(d_obs, A, N, H, la, ai)))
                for la in (0, 1) for ai in (0, 1)}
        assert all(v > 0 and v % 4 == 0 for v in size.values()), (d_obs, A, N, H, size)
        for la, ai in size:
            dense = H * (pad(d_obs + A + N) - pad(d_obs + A * la + N * ai))
            assert size[1, 1] - size[la, ai] == dense + (1 - la) * A * H + (1 - ai) * N * H, (d_obs, A, N, H, la, ai)
    for c in DS.AGENT_GRAD_CASES:
        d = _agent_dims(DS.GRAD_D_OBS, c.A, DS.GRAD_N, c.H, int(c.last_action), int(c.agent_id))
        sizes = [lib.mlg_agent_backward_workspace_floats(_native.byref(d), R) for R in (0, 1, 64, 65, 256, 257)]
        assert all(n > 0 and n % 4 == 0 for n in sizes) and sizes == sorted(sizes), (c.id, sizes)
        assert sizes[3] > 65 * (11 * c.H) + (65 * c.A + 3) // 4 * 4  # the row sections: x, hc, hp, dx, dgi, dgh, gq
    bad = _agent_dims(80, 15, 5, 64, 1, 1)
    bad.d_in -= 1
    assert lib.mlg_packed_agent_size(_native.byref(bad)) == -1
    assert lib.mlg_agent_backward_workspace_floats(_native.byref(bad), 8) == -1


# ---- F ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,A", DS.GREEDY_SHAPES)
def test_selection_cases(B, N, A):
    q, av, rows = DS.select_case(B, N, A)
    R = B * N
    qf, af = q.reshape(R, A), av.reshape(R, A)
    g = LR.greedy_select(torch.from_numpy(q), torch.from_numpy(av)).numpy().reshape(R)
    masked = np.where(af != 0, qf, -np.inf)
    if (B, N, A) == (1, 1, 1):
        assert rows == {"tie": [], "max_unavailable": [], "masked": []} and g.tolist() == [0]
        return
    assert len(rows["tie"]) >= 2 and len(rows["max_unavailable"]) >= 2 and len(rows["masked"]) == 1
    assert len(set(rows["tie"]) | set(rows["max_unavailable"]) | set(rows["masked"])) == \
        len(rows["tie"]) + len(rows["max_unavailable"]) + 1
    for r in rows["tie"]:  # condition 4: two available slots hold the same bits, and that value is the row's maximum
        top = np.nonzero(masked[r] == masked[r].max())[0]
        assert len(top) == 2 and qf[r, top[0]].tobytes() == qf[r, top[1]].tobytes(), r
        assert g[r] == top[0]  # the oracle takes the lower index
    for r in rows["max_unavailable"]:
        k = int(np.argmax(qf[r]))
        assert af[r, k] == 0 and g[r] != k and af[r, g[r]] == 1
    r = rows["masked"][0]
    assert not af[r].any() and g[r] == 0
    live = np.ones(R, bool)
    live[rows["masked"]] = False
    assert af[live].any(axis=1).all() and 0.3 < af.mean() < 0.55
    if R > 256:  # both blocks hold special rows or plain ones: the second block is not empty
        assert (np.arange(R) >= 256).sum() > 0


@pytest.mark.parametrize("B,N,A", DS.EPS_SHAPES)
def test_epsilon_cases_mix_greedy_and_random_picks(B, N, A):
    q, av, rows = DS.select_case(B, N, A, masked_row=False)
    assert rows["masked"] == [] and av.reshape(B * N, A).any(axis=1).all()
    keys, episodes = DS.select_keys(B)
    assert all(int(k) >> 63 for k in keys) and len(set(episodes.tolist())) > 1
    for t in DS.EPS_T:
        for eps, eps_list in ((0.6, episodes.tolist()), (1.0, episodes.tolist()), (0.6, [0] * B)):
            a, g = LR.eps_select(torch.from_numpy(q), torch.from_numpy(av), eps, [int(k) for k in keys], eps_list, t)
            assert np.take_along_axis(av, a[..., None], 2).all()  # every pick is available
            if eps == 1.0:
                assert not g.any()
            else:
                assert 0 < g.sum() < g.size
    a0, _ = LR.eps_select(torch.from_numpy(q), torch.from_numpy(av), 0.6, [int(k) for k in keys], episodes.tolist(), 0)
    a1, _ = LR.eps_select(torch.from_numpy(q), torch.from_numpy(av), 0.6, [int(k) for k in keys], [0] * B, 0)
    assert not np.array_equal(a0, a1)  # the episode counter enters the stream: NULL episodes is another case
