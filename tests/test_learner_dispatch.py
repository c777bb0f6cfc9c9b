"""The fused learner's dispatch, pinned through the host-only query (mlg_qlearner_describe; no GPU needed): which
kernels mlg_qlearner_train launches for a cfg under the MLG_MIX_GENERIC environment. run_train reads the struct the
query prints (one host function, make_dispatch, decides for both), so the GPU parity cases of
tests/test_gpu_learner_arms.py are named after arms this file pins.

A name is "<agent part> + <mixer part>". Agent part: h32 | h64 | h128 (run_train<H>: agent_in / agent_rec4 or
rec4_mixpre / agent_q / agent_bwd4 / agent_dx), bwd-fused (H = 64: bwd4_wgrad_kernel) or bwd-split, q1..q6 (16-action
tiles: agent_q_kernel runs 64 threads per tile). Mixer part: iql (iql_td_kernel), vdn-fast / vdn
(mix_td_kernel<64, 32, true> / <64, 32> with mixer 1), qmix-split (rec4_mixpre_kernel<H> + mix_td2_kernel<64, 32>),
qmix-generic (mix_td_kernel<64, 32>), qmix1-e{E} (mix_td1_kernel<E>), qmix-he{HE}-e{E} (mix_td_kernel<HE, E>).

An arm that no cfg reaches: the QMIX branch inside mix_td_kernel<64, 32, true>. The prefetching one-kernel form is
taken by a QMIX cfg only when the split form is not, and the split form needs the agent workgroup (H / 16 waves, 128 /
256 / 512 threads) to be a multiple of 128 threads, which holds for all three H. make_dispatch would name it
"qmix-fast1"; test_qmix_fast_one_kernel_form_is_unreachable sweeps for it.
"""
import ctypes
import re

import pytest

import learner_arm_shapes as LA
from helpers import qmix_args

PLANS = [f"{k}v{k}" for k in range(1, 33)] + ["large", "5v7", "3v5"]
MIXERS = {"qmix": {}, "vdn": {"mixer": "vdn"}, "iql": {"mixer": None}}
NAME = re.compile(r"^h(32|64|128)/bwd-(fused|split)/q([1-6]) \+ "
                  r"(iql|vdn-fast|vdn|qmix-split|qmix-generic|qmix1-e(16|32|64)|qmix-he(32|64|128)-e(16|32|64))$")


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    for k in ("MLG_MIX_GENERIC", "MLG_LEARNER_FULL"):
        monkeypatch.delenv(k, raising=False)


def _describe(dims, hidden, **kw):
    from maleague import _native
    N, A, S, d_obs = dims
    args = qmix_args(n_agents=N, n_actions=A, state_shape=S, rnn_hidden_dim=hidden, device="cpu", **kw)
    return _native.qlearner_describe(LA.learner_cfg(args, d_obs))


@pytest.mark.parametrize("cid", LA.IDS)
def test_case_arm(cid):
    c = LA.case(cid)
    name = LA.describe(c)
    assert name == c.arm
    assert NAME.match(name), name
    N, A, _, _ = LA.dims(c)
    assert name.startswith(f"h{c.H}/bwd-{'fused' if c.H == 64 else 'split'}/q{(A + 15) // 16} + ")


def test_case_table_is_complete():
    """The cases the table must hold, what their names promise, and a float64 figure for each."""
    assert len(set(LA.IDS)) == len(LA.IDS) and set(LA.ORACLE_F64) == set(LA.IDS)
    assert LA.dims(LA.case("split-h64-1v1"))[0] == 1
    assert LA.dims(LA.case("split-at-bounds"))[:3] == (8, 16, 64)
    assert LA.dims(LA.case("generic-h64-32v32"))[0] == 32          # MAXN
    assert LA.dims(LA.case("maxa-h128"))[1] == 96                  # MLG_BWD_MAXA
    assert max(LA.dims(c)[3] + LA.dims(c)[1] + LA.dims(c)[0] for c in LA.CASES) == 613   # d_in of 32v32
    assert {int(c.arm.split("/q")[1][0]) for c in LA.CASES} == {1, 2, 3, 4, 5, 6}
    for h in (32, 64, 128):
        assert any(c.H == h and LA.mixer_part(c.arm) == "qmix-split" for c in LA.CASES)
        assert any(c.H == h and LA.mixer_part(c.arm) == "qmix-generic" for c in LA.CASES)
    assert any(LA.clips(i) for i in LA.IDS) and not all(LA.clips(i) for i in LA.IDS)
    for i in LA.IDS:  # ten times the oracle's own error loosens no bound
        assert LA.bounds(i) == (LA.STAT_RTOL, LA.PARAM_ATOL, LA.GRAD_RTOL)


def test_plan_dims_follow_the_env():
    for k in (1, 2, 5, 9, 32):
        assert LA.plan_dims(f"{k}v{k}") == (k, 2 * k + 5, 12 * k, 16 * k)
    assert LA.plan_dims("large") == (25, 55, 300, 400)
    assert LA.plan_dims("small") == (3, 11, 36, 48)


def test_default_arms_all_have_a_gpu_case():
    """Every (H, mixer part) the default environment reaches with a plan (K-vs-K for K = 1..32, `large`, 5v7, 3v5) and
    the default qmix, vdn or iql config appears in a GPU parity case of the table, or in ARMS_COVERED_ELSEWHERE for
    the arms the earlier learner suites run."""
    have = {(c.H, LA.mixer_part(c.arm)) for c in LA.CASES}
    met = set()
    for hidden in (32, 64, 128):
        for plan in PLANS:
            dims = LA.plan_dims(plan)
            for kw in MIXERS.values():
                name = _describe(dims, hidden, **kw)
                assert NAME.match(name), name
                met.add((hidden, LA.mixer_part(name)))
    assert met == {(h, m) for h in (32, 64, 128) for m in ("qmix-split", "qmix-generic", "vdn-fast", "vdn", "iql")}
    missing = met - have - LA.ARMS_COVERED_ELSEWHERE
    assert not missing, missing


def test_bounds_of_the_fast_side():
    """N <= 8, A <= 16 and the padded state width <= 64, each crossed alone; MLG_MIX_GENERIC (read per call)."""
    for hidden in (32, 64, 128):
        part = lambda *d, **kw: LA.mixer_part(_describe(d, hidden, **kw))  # noqa: E731
        assert part(8, 16, 64, 23) == "qmix-split" and part(8, 16, 49, 23) == "qmix-split"
        assert part(9, 16, 64, 23) == part(8, 17, 64, 23) == part(8, 16, 65, 23) == "qmix-generic"
        assert part(8, 16, 64, 23, mixer="vdn") == "vdn-fast"
        assert part(9, 16, 64, 23, mixer="vdn") == part(8, 17, 64, 23, mixer="vdn") == "vdn"
        assert part(8, 16, 65, 23, mixer="vdn") == "vdn"
        assert part(9, 17, 65, 23, mixer=None) == part(2, 3, 4, 5, mixer=None) == "iql"


def test_forcing_variable_and_widths(monkeypatch):
    d = (5, 15, 60, 80)
    assert _describe(d, 64) == "h64/bwd-fused/q1 + qmix-split"
    assert _describe(d, 64, hypernet_layers=1, mixing_embed_dim=16) == "h64/bwd-fused/q1 + qmix1-e16"
    assert _describe(d, 32, mixing_embed_dim=64, hypernet_embed=128) == "h32/bwd-split/q1 + qmix-he128-e64"
    assert _describe(d, 64, mixing_embed_dim=32, hypernet_embed=64, hypernet_layers=2) == "h64/bwd-fused/q1 + qmix-split"
    monkeypatch.setenv("MLG_MIX_GENERIC", "1")
    assert _describe(d, 64) == "h64/bwd-fused/q1 + qmix-generic"
    assert _describe(d, 64, mixer="vdn") == "h64/bwd-fused/q1 + vdn"
    assert _describe(d, 64, mixer=None) == "h64/bwd-fused/q1 + iql"
    monkeypatch.delenv("MLG_MIX_GENERIC")
    monkeypatch.setenv("MLG_LEARNER_FULL", "1")  # changes what is skipped, not what is launched
    assert _describe(d, 64) == "h64/bwd-fused/q1 + qmix-split"


def test_qmix_fast_one_kernel_form_is_unreachable():
    for hidden in (32, 64, 128):
        for n in (1, 8):
            for a in (1, 16):
                for s in (1, 64):
                    assert LA.mixer_part(_describe((n, a, s, 7), hidden)) == "qmix-split"


@pytest.mark.parametrize("kw,key", [(dict(N=33), "N=33"), (dict(A=97), "n_actions=97"), (dict(H=48), "rnn_hidden_dim=48"),
                                    (dict(T=1), "T=1"), (dict(E=24), "mixing_embed_dim=24"),
                                    (dict(HE=48), "hypernet_embed=48")],
                         ids=["N=33", "A=97", "H=48", "T=1", "E=24", "HE=48"])
def test_refusals_name_their_key(kw, key):
    """Where mlg_qlearner_train would refuse, the query and the two size calls refuse with the same message."""
    from maleague import _native
    lib = _native.load()
    cfg = LA.learner_cfg(qmix_args(device="cpu"), 80)
    assert _native.qlearner_describe(cfg) == "h64/bwd-fused/q1 + qmix-split"
    for k, v in kw.items():
        setattr(cfg, k, v)
    with pytest.raises(_native.NativeError, match=key):
        _native.qlearner_describe(cfg)
    assert lib.mlg_qlearner_workspace_floats(_native.byref(cfg)) == -1
    assert key.encode() in lib.mlg_last_error()
    assert lib.mlg_qlearner_param_counts(_native.byref(cfg), None, None) == -1
    assert key.encode() in lib.mlg_last_error()


def test_describe_checks_its_output_buffer():
    from maleague import _native
    lib = _native.load()
    cfg = LA.learner_cfg(qmix_args(device="cpu"), 80)
    small = ctypes.create_string_buffer(8)
    assert lib.mlg_qlearner_describe(_native.byref(cfg), small, len(small)) != 0
    assert b"too small" in lib.mlg_last_error() and small.value == b""
    assert lib.mlg_qlearner_describe(_native.byref(cfg), None, 0) != 0


@pytest.mark.parametrize("cid", LA.IDS)
def test_param_counts_and_workspace(cid):
    """mlg_qlearner_param_counts against the torch modules, at every case's dims."""
    from maleague import _native
    from maleague.modules.agents.drqn_agent import DRQNAgentNetwork
    from maleague.modules.mixers import QMixer
    c = LA.case(cid)
    lib = _native.load()
    args = LA.case_args(c, "cpu")
    N, A, S, d_obs = LA.dims(c)
    cfg = LA.learner_cfg(args, d_obs)
    assert lib.mlg_qlearner_workspace_floats(_native.byref(cfg)) > 0, lib.mlg_last_error()
    na, nm = ctypes.c_int64(-1), ctypes.c_int64(-1)
    total = lib.mlg_qlearner_param_counts(_native.byref(cfg), ctypes.byref(na), ctypes.byref(nm))
    want_a = sum(p.numel() for p in DRQNAgentNetwork(d_obs + A + N, args).parameters())
    want_m = sum(p.numel() for p in QMixer(args).parameters()) if args.mixer == "qmix" else 0
    assert (na.value, nm.value, total) == (want_a, want_m, want_a + want_m)
