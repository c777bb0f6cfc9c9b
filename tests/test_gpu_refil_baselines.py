"""GPU parity of REFILLearner.train on the two attention baselines (mlg_refil_train with imagine = 0: the plain
entity agent with FlexQMixer, attention-QMIX, and with VDNMixer, attention-VDN) against the reference's golden
vectors (tests/golden/refil_attn_qmix.npz, refil_attn_vdn.npz: two consecutive REFILLearner.train calls) and
against the CPU restatement (tests/refil_baseline_ref.py) on other batches.

Tolerances are those the imagine path is held to on the same batches (tests/test_gpu_refil_learner.py): stats rtol
2e-4 (fp32, different summation orders), parameters after RMSprop atol 2e-5.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import refil_baseline_ref as BR
from helpers import batch_mask_sum, refil_args
from refil_learner_shapes import synthetic_entity_batch as _synthetic_entity_batch
from test_gpu_refil_learner import _Log, _batch_from, _learner, _pre

pytestmark = pytest.mark.gpu

KEYS = {"loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean"}  # refil_learner.py:185-196, no im_loss
PLAIN = "entity_attend_rnn"


def _mixer_p(mixer, a_cpu):
    from maleague.modules.mixers import FlexQMixer
    if mixer == "vdn":
        return None
    return {k: v.detach().cpu().numpy() for k, v in FlexQMixer(a_cpu).state_dict().items()}


def _check(L, ref, got, want, tag, stat_atol=1e-5):
    assert set(got) == set(want) == KEYS, tag
    for k in want:
        np.testing.assert_allclose(got[k], want[k], rtol=2e-4, atol=stat_atol, err_msg=f"{tag} {k}")
    for k, v in L.mac.agent.named_parameters():
        np.testing.assert_allclose(v.detach().cpu().numpy(), ref.agent[k].detach().numpy(), atol=2e-5, rtol=0,
                                   err_msg=f"{tag} agent {k}")
    assert [k for k, _ in L.mixer.named_parameters()] == list(ref.mixer)
    for k, v in L.mixer.named_parameters():
        np.testing.assert_allclose(v.detach().cpu().numpy(), ref.mixer[k].detach().numpy(), atol=2e-5, rtol=0,
                                   err_msg=f"{tag} mixer {k}")


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", ["static", "generic"])
@pytest.mark.parametrize("mixer,fixture", [("flex_qmix", "refil_attn_qmix.npz"), ("vdn", "refil_attn_vdn.npz")])
def test_baselines_two_calls_match_golden(device, golden, mixer, fixture, inst, monkeypatch):
    """Two reference train calls on the B = 4, T = 7 fixture batch, static (refil_8) and generic instantiations;
    initial parameters: refil_learner.npz's."""
    if inst == "generic":
        monkeypatch.setenv("MLG_REFIL_GENERIC", "1")
    d, d0 = golden(fixture), golden("refil_learner.npz")
    a = refil_args(device="cuda", agent=PLAIN, mixer=mixer)
    arrs = _pre(d, "b.")
    eb = _batch_from(arrs, device)
    L, log = _learner(eb, _pre(d0, "p0.agent."), _pre(d0, "p0.mixer.") if mixer == "flex_qmix" else None, a)
    assert len(L.parameters()) == (13 if mixer == "vdn" else 41)
    msum = 0
    for call in range(2):
        L.train(eb, 0, episode_num=call)
        st = L.last_stats
        assert set(st) == KEYS
        for k, v in st.items():
            np.testing.assert_allclose(v, float(d[f"c{call}.stat.{k}"]), rtol=2e-4, atol=1e-6, err_msg=f"call {call} {k}")
        for k, v in L.mac.agent.named_parameters():
            np.testing.assert_allclose(v.detach().cpu().numpy(), d[f"c{call}.agent.{k}"], atol=2e-5, rtol=0,
                                       err_msg=f"call {call} agent {k}")
        for k, v in L.mixer.named_parameters():
            np.testing.assert_allclose(v.detach().cpu().numpy(), d[f"c{call}.mixer.{k}"], atol=2e-5, rtol=0,
                                       err_msg=f"call {call} mixer {k}")
        assert float(L._stats[1].item()) == 0.0  # stats[1] (im_loss of the imagine path) is written as 0
        msum += int(batch_mask_sum(arrs["filled"], arrs["terminated"]))
    assert set(log.stats) == KEYS
    assert L.mac.agent.trained_steps == msum == 2 * int(round(float(L._stats[6].item())))


# ---- 2. the restatement on HIP rollouts --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip_rollout(device):
    from test_gpu_refil import _rollout
    spec, ag, a0, nb, summ, _ = _rollout(device, B=8, T=30, seed=11, eps=0.3, test_mode=False)
    T = int(summ["len"].max()) + 1
    arrs = {k: np.ascontiguousarray(v[:, :T]) for k, v in nb.items()}
    return arrs, {k: v.detach().cpu().numpy() for k, v in ag.state_dict().items()}


@pytest.mark.parametrize("mixer,softmax,double_q", [("flex_qmix", False, True), ("flex_qmix", True, False),
                                                    ("vdn", False, True)])
def test_baselines_match_restatement_on_hip_rollouts(device, hip_rollout, mixer, softmax, double_q):
    """Episodes from the HIP REFIL rollout (variable 3..8 agents, eps 0.3), 2 train calls."""
    arrs, agent_p = hip_rollout
    kw = dict(agent=PLAIN, mixer=mixer, softmax_mixing_weights=softmax, double_q=double_q)
    a, a_cpu = refil_args(device="cuda", **kw), refil_args(device="cpu", **kw)
    eb = _batch_from(arrs, device)
    torch.manual_seed(4)
    mixer_p = _mixer_p(mixer, a_cpu)
    L, _ = _learner(eb, agent_p, mixer_p, a)
    ref = BR.REFILBaselineRef(agent_p, mixer_p, a_cpu)
    batch = {k: torch.from_numpy(v) for k, v in arrs.items()}
    for call in range(2):
        want = ref.train(batch, episode_num=call)
        L.train(eb, 0, episode_num=call)
        _check(L, ref, L.last_stats, want, f"call {call}")


# ---- 3. the baseline is the imagine path at lmbda = 0 ------------------------------------------------------------
def test_attn_qmix_equals_imagine_path_with_lmbda_0(device, golden):
    """The fixture batch, the imagine fixture's group draws, the same initial parameters, two calls: every common
    stat and all parameters within the tolerances of test 1 (the reference's own two paths differ by 2e-8 on the
    CPU). The bitwise comparison is printed, not asserted."""
    d = golden("refil_learner.npz")
    arrs = _pre(d, "b.")
    La, _ = _learner(_batch_from(arrs, device), _pre(d, "p0.agent."), _pre(d, "p0.mixer."),
                     refil_args(device="cuda", agent=PLAIN))
    Li, _ = _learner(_batch_from(arrs, device), _pre(d, "p0.agent."), _pre(d, "p0.mixer."),
                     refil_args(device="cuda", lmbda=0.0))
    for call in range(2):
        La.train(_batch_from(arrs, device), 0, episode_num=call)
        Li.train(_batch_from(arrs, device), 0, episode_num=call, groupA=torch.from_numpy(d[f"c{call}.groupA"]))
        sa, si = La.last_stats, Li.last_stats
        assert set(si) - set(sa) == {"im_loss"}
        for k in sa:
            np.testing.assert_allclose(sa[k], si[k], rtol=2e-4, atol=1e-6, err_msg=f"call {call} {k}")
        pa, pi = La._flat.flat.cpu().numpy(), Li._flat.flat.cpu().numpy()
        print(f"call {call}: bitwise equal parameters {np.array_equal(pa, pi)}, max abs diff {np.abs(pa - pi).max():.3e}, "
              f"stats equal {all(sa[k] == si[k] for k in sa)}")
        np.testing.assert_allclose(pa, pi, atol=2e-5, rtol=0, err_msg=f"call {call}")


# ---- 4. NA not a multiple of 8 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mixer", ["flex_qmix", "vdn"])
@pytest.mark.parametrize("NA,NE", [(5, 12), (3, 7)])
def test_baselines_na_not_multiple_of_8(device, NA, NE, mixer):
    """The NA % 8 != 0 branch (generic instantiations, no t-major skipping, conditional zeroing of d2 / dfc2 / dout)."""
    A = 5 + NE
    B, T1 = 8, 25
    lens = np.random.RandomState(NA).randint(4, T1 - 1, size=B)
    arrs = _synthetic_entity_batch(B, T1, NA, NE, 8, A, lens, seed=NA * 10 + NE)
    T = int(lens.max()) + 1
    arrs = {k: np.ascontiguousarray(v[:, :T]) for k, v in arrs.items()}
    kw = dict(n_agents=NA, n_entities=NE, n_actions=A, agent=PLAIN, mixer=mixer)
    a_dev, a_cpu = refil_args(device="cuda", **kw), refil_args(device="cpu", **kw)
    eb = _batch_from(arrs, device, NE=NE, NA=NA, A=A)
    torch.manual_seed(NA)
    from maleague.modules.agents import REGISTRY as agent_REGISTRY
    mixer_p = _mixer_p(mixer, a_cpu)
    agent_p = {k: v.detach().cpu().numpy() for k, v in agent_REGISTRY[PLAIN](8 + A, a_cpu).state_dict().items()}
    L, _ = _learner(eb, agent_p, mixer_p, a_dev)
    ref = BR.REFILBaselineRef(agent_p, mixer_p, a_cpu)
    batch = {k: torch.from_numpy(v) for k, v in arrs.items()}
    for call in range(2):
        want = ref.train(batch, episode_num=call)
        L.train(eb, 0, episode_num=call)
        _check(L, ref, L.last_stats, want, f"NA={NA} call {call}")


# ---- 5. the second mask-scan path --------------------------------------------------------------------------------
@pytest.mark.parametrize("mixer", ["flex_qmix", "vdn"])
def test_baselines_mask_scan_path(device, mixer):
    """33 episodes (> 32): the general mask scan of batch_mask_device.h. B = 33, T = 9, one call vs the restatement
    and the exact mask sum."""
    NA, NE, A, B, T1 = 8, 16, 21, 33, 9
    lens = np.random.RandomState(5).randint(2, T1 - 1, size=B)
    lens[0] = T1 - 2
    arrs = _synthetic_entity_batch(B, T1, NA, NE, 8, A, lens, seed=33)
    arrs = {k: np.ascontiguousarray(v[:, :T1]) for k, v in arrs.items()}
    kw = dict(agent=PLAIN, mixer=mixer)
    a_dev, a_cpu = refil_args(device="cuda", **kw), refil_args(device="cpu", **kw)
    eb = _batch_from(arrs, device)
    assert eb.max_seq_length == 9
    torch.manual_seed(6)
    from maleague.modules.agents import REGISTRY as agent_REGISTRY
    mixer_p = _mixer_p(mixer, a_cpu)
    agent_p = {k: v.detach().cpu().numpy() for k, v in agent_REGISTRY[PLAIN](8 + A, a_cpu).state_dict().items()}
    L, _ = _learner(eb, agent_p, mixer_p, a_dev)
    ref = BR.REFILBaselineRef(agent_p, mixer_p, a_cpu)
    T = int(lens.max()) + 1  # the reference trains on the batch truncated at max_t_filled (8 of the 9 steps)
    want = ref.train({k: torch.from_numpy(np.ascontiguousarray(v[:, :T])) for k, v in arrs.items()}, episode_num=0)
    L.train(eb, 0, episode_num=0)
    _check(L, ref, L.last_stats, want, "B=33")
    assert np.float32(L._stats[6].item()) == batch_mask_sum(arrs["filled"], arrs["terminated"])


# ---- 6. sampled views --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixer", ["flex_qmix", "vdn"])
def test_baselines_sampled_view_matches_copy(device, hip_rollout, mixer, monkeypatch):
    """Six episodes sampled as an in-place view of a device replay ring, through both slot-map paths -- the
    kernel-argument map (host_rows) and the device map (rows; taken when the batch exceeds the inline-row capacity,
    set to 0 here) -- train bitwise like the gathered copy of the same episodes, as
    test_refil_learner_sampled_view_matches_copy holds the imagine path to. The ring is five steps longer than any
    episode. Steps past max_t_filled are inert: a ring whose unfilled tail holds junk (NaN entities and rewards, set
    masks, random availability) trains bitwise like the clean one.

    Against the copy truncated in time at max_t_filled the results agree to rounding only, not bitwise: the per-item
    partials (stats) and the weight-gradient chunks are laid out by i = b * T + t, so another T sums the same terms
    in another order. Measured on the MI355X: loss 0.0082281502 vs 0.0082281511, td_error_abs 0.03726523 vs
    0.03726522 (1e-7 relative). That holds for the imagine path as well (test_refil_learner_padded_steps_are_inert
    bounds it by rtol 1e-5 / atol 1e-7 on the stats and atol 1e-6 on the parameters); the same bounds are held here."""
    from maleague import _native
    from maleague.components.replay_buffer import ReplayBuffer
    from helpers import entity_scheme_for
    arrs, agent_p = hip_rollout
    B, T = arrs["entities"].shape[:2]
    T1 = T + 5
    pad = {k: np.concatenate([v, np.zeros((B, T1 - T) + v.shape[2:], v.dtype)], axis=1) for k, v in arrs.items()}
    junk = {k: v.copy() for k, v in pad.items()}
    rng = np.random.RandomState(0)
    junk["entities"][:, T:] = np.nan
    junk["reward"][:, T:] = np.nan
    junk["obs_mask"][:, T:] = 1
    junk["entity_mask"][:, T:] = rng.randint(0, 2, size=junk["entity_mask"][:, T:].shape)
    junk["avail_actions"][:, T:] = rng.randint(0, 2, size=junk["avail_actions"][:, T:].shape)
    junk["actions"][:, T:] = rng.randint(0, 21, size=junk["actions"][:, T:].shape)
    junk["actions_onehot"][:, T:] = 7.0
    info = {"n_agents": 8, "n_actions": 21, "n_entities": 16, "entity_shape": 8, "episode_limit": T1 - 1}
    scheme, groups, pre = entity_scheme_for(info, torch)
    bufs = []
    for src in (pad, junk):
        buf = ReplayBuffer(scheme, groups, 12, T1, preprocess=pre, device=device)
        buf.insert_episode_batch(_batch_from(src, device))
        for k, v in src.items():  # the insert recomputes actions_onehot: restore the junk tail
            buf.data.transition_data[k][:B].copy_(torch.as_tensor(v))
        bufs.append(buf)
    np.random.seed(1)
    view = bufs[0].sample(6, view=True)
    assert view.host_rows is not None and view.max_seq_length == T1
    ids = view.ep_ids
    Tf = int(arrs["filled"][ids].sum(axis=1).max())
    assert Tf < T1
    copy_ = bufs[0][ids]
    assert copy_.max_seq_length == T1
    trunc = _batch_from({k: np.ascontiguousarray(v[ids, :Tf]) for k, v in arrs.items()}, device)
    a = refil_args(device="cuda", agent=PLAIN, mixer=mixer)
    torch.manual_seed(8)
    mixer_p = _mixer_p(mixer, refil_args(device="cpu"))
    Lh, Lr, Lj, Lc, Lt = [_learner(trunc, agent_p, mixer_p, a)[0] for _ in range(5)]
    lib = _native.load(require_gpu=True)
    for call in range(2):
        Lh.train(view, 0, episode_num=call)
        assert view._rows is None  # the slot map travelled as a kernel argument
        Lc.train(copy_, 0, episode_num=call)
        Lj.train(type(view)(bufs[1], ids), 0, episode_num=call)
        Lt.train(trunc, 0, episode_num=call)
        with monkeypatch.context() as m:
            m.setattr(lib, "mlg_qlearner_inline_rows", lambda: 0)
            view_r = type(view)(bufs[0], ids)
            Lr.train(view_r, 0, episode_num=call)
            assert view_r._rows is not None and view_r._data is None
        sc = Lc.last_stats
        for tag, L in (("host_rows", Lh), ("rows", Lr), ("junk tail", Lj)):
            assert L.last_stats == sc, (call, tag, L.last_stats, sc)
            assert torch.equal(L._flat.flat, Lc._flat.flat) and torch.equal(L._grads, Lc._grads), (call, tag)
        st = Lt.last_stats
        print(f"call {call} view vs time-truncated copy:", {k: (sc[k], st[k]) for k in sc},
              "max abs parameter diff", float((Lt._flat.flat - Lc._flat.flat).abs().max()))
        for k in sc:
            np.testing.assert_allclose(sc[k], st[k], rtol=1e-5, atol=1e-7, err_msg=f"call {call} {k}")
        np.testing.assert_allclose(Lc._flat.flat.cpu().numpy(), Lt._flat.flat.cpu().numpy(), atol=1e-6, rtol=0)


# ---- 7. workspace (host only) ------------------------------------------------------------------------------------
def _cfg(**kw):
    from maleague import _native
    d = dict(B=32, T=101, n_agents=8, n_entities=16, entity_shape=8, n_actions=21, entity_last_action=1,
             attn_embed_dim=64, attn_n_heads=4, rnn_hidden_dim=64, hypernet_embed=64, mixing_embed_dim=32, double_q=1,
             softmax_mixing_weights=0, imagine=1, mixer=0, gamma=0.99, lmbda=0.5, lr=5e-4, optim_alpha=0.99,
             optim_eps=1e-5, grad_norm_clip=10.0)
    d.update(kw)
    return _native.MlgRefilLearnerCfg(**d)


def test_baseline_workspace_and_param_counts():
    """At the refil_8 shape with B = 32, T = 101: imagine = 0 needs strictly less workspace than imagine = 1, vdn
    no more than flex_qmix; vdn's flat parameters are the agent alone."""
    from maleague import _native
    lib = _native.load()
    ws = {k: lib.mlg_refil_workspace_floats(_native.byref(_cfg(imagine=k[0], mixer=k[1])))
          for k in ((1, 0), (0, 0), (0, 1))}
    print("workspace floats", ws)
    assert 0 < ws[(0, 1)] <= ws[(0, 0)] < ws[(1, 0)]
    for (im, mx), (na, nm) in {(1, 0): (48853, 81792), (0, 0): (48853, 81792), (0, 1): (48853, 0)}.items():
        a, m = ctypes.c_int64(), ctypes.c_int64()
        n = lib.mlg_refil_param_counts(_native.byref(_cfg(imagine=im, mixer=mx)), ctypes.byref(a), ctypes.byref(m))
        assert (n, a.value, m.value) == (na + nm, na, nm)


# ---- 8. refusals -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,msg", [(dict(imagine=1, mixer=1), "imagine=1 with mixer=1 (vdn)"),
                                    (dict(imagine=2), "imagine=2"), (dict(imagine=-1), "imagine=-1"),
                                    (dict(imagine=0, mixer=2), "mixer=2"), (dict(mixer=-1), "mixer=-1")])
def test_c_level_refusals(kw, msg):
    """check_cfg refuses by name (mlg_last_error) in all three entry points; mlg_refil_train returns before it reads
    its buffers (a zeroed MlgRefilLearnerBufs: nothing could be launched from it)."""
    from maleague import _native
    lib = _native.load()
    c = _cfg(**kw)
    assert lib.mlg_refil_workspace_floats(_native.byref(c)) == -1
    assert msg in lib.mlg_last_error().decode()
    assert lib.mlg_refil_param_counts(_native.byref(c), None, None) == -1
    bufs = _native.MlgRefilLearnerBufs()
    assert lib.mlg_refil_train(_native.byref(c), _native.byref(bufs), None) != 0
    assert msg in lib.mlg_last_error().decode()


def test_unsupported_train_launches_nothing(device, golden):
    """A learner whose combination became unsupported after construction (the cfg is built per call): train raises
    the C refusal and parameters, RMSprop state, stats and the trained-step counter stay untouched."""
    from maleague import _native
    d = golden("refil_learner.npz")
    eb = _batch_from(_pre(d, "b."), device)
    L, _ = _learner(eb, _pre(d, "p0.agent."), None, refil_args(device="cuda", agent=PLAIN, mixer="vdn"))
    L.imagine = True  # imagine = 1 with vdn
    before = L._flat.flat.clone()
    with pytest.raises(_native.NativeError, match="imagine=1 with mixer=1"):
        L.train(eb, 0, episode_num=0)
    torch.cuda.synchronize()
    assert torch.equal(L._flat.flat, before) and float(L._sq.abs().sum()) == 0.0
    assert float(L._stats.abs().sum()) == 0.0 and L.train_calls == 0 and L.mac.agent.trained_steps == 0
    with pytest.raises(ValueError, match="groupA"):
        L.imagine = False
        L.train(eb, 0, episode_num=0, groupA=torch.zeros(4, 16, dtype=torch.uint8))
    assert L.train_calls == 0


# ---- 9. end to end -----------------------------------------------------------------------------------------------
def test_attn_vdn_end_to_end(device, tmp_path):
    from maleague.controllers import EntityMAC
    from maleague.custom_logging import MainLogger
    from maleague.learners import REFILLearner
    from maleague.modules.mixers import VDNMixer
    from maleague.runs import MultiAgentExperiment
    from maleague.utils.config import build_config, to_args
    cfg = build_config("attn_vdn", "ma_entity",
                       overrides=["runner=parallel", "batch_size_run=8", "batch_size=8", "buffer_cpu_only=False",
                                  "buffer_size=16", "env_args.episode_limit=10", "seed=0", "show_exp_parameters=False",
                                  "t_max=1000000", "test_interval=100000000", "learner_log_interval=0",
                                  f"local_results_path={tmp_path}"])
    np.random.seed(0)
    torch.manual_seed(0)
    exp = MultiAgentExperiment(to_args(cfg), MainLogger(log_interval=10 ** 12))
    L = exp.home_learner
    assert type(L) is REFILLearner and type(L.mixer) is VDNMixer and not L.imagine
    log = _Log()
    L.logger = log
    exp._init_stepper()
    for i in range(3):
        exp._train_episode(i * 8)
    assert L.train_calls == 3 and L._groups is None  # no group draw was launched
    assert set(log.stats) == KEYS and set(L.last_stats) == KEYS
    assert all(np.isfinite(v) for v in L.last_stats.values()) and L.mac.agent.trained_steps > 0
    path = str(tmp_path / "ckpt")
    os.makedirs(path)
    L.save_models(path, L.name)
    assert sorted(os.listdir(path)) == [f"{L.name}{f}" for f in ("agent.th", "mixer.th", "opt.th")]
    assert torch.load(f"{path}/{L.name}mixer.th", weights_only=True) == {}
    opt = torch.load(f"{path}/{L.name}opt.th", weights_only=True)
    assert len(opt["state"]) == 13  # the agent's RMSprop state alone
    mac2 = EntityMAC(exp.home_buffer.scheme, exp.groups, exp.args)
    fresh = REFILLearner(mac2, exp.home_buffer.scheme, _Log(), exp.args, name="home")
    fresh.build_optimizer()
    assert not torch.equal(fresh._flat.flat, L._flat.flat)
    fresh.load_models(path)
    assert torch.equal(fresh._flat.flat, L._flat.flat) and fresh._flat.flat.numel() == 48853
    assert torch.equal(fresh._tflat.flat, L._flat.flat)
    assert torch.equal(fresh._sq, L._sq) and float(fresh._sq.abs().sum()) > 0
    assert float(fresh._step) == float(L._step) == 3.0
    exp.stepper.close_env()


# ---- 10. workspace reuse across calls ----------------------------------------------------------------------------
@pytest.mark.parametrize("mixer", ["flex_qmix", "vdn"])
@pytest.mark.parametrize("NA,NE", [(8, 16), (5, 12)])
def test_baselines_no_stale_rows_across_calls(device, NA, NE, mixer):
    """Rows the backward kernels skip (items past an episode's live steps) must not carry data from an earlier call,
    as test_refil_learner_no_stale_rows_across_calls checks for the imagine path: a learner trained on LONG episodes
    and then on SHORT ones (same workspace layout) ends bit-identical to a fresh learner, holding its parameters,
    RMSprop state and targets, trained on the short batch alone."""
    A = 5 + NE
    B, T1 = 8, 41
    long_b = _synthetic_entity_batch(B, T1, NA, NE, 8, A, np.full(B, T1 - 2), seed=1)
    short_b = _synthetic_entity_batch(B, T1, NA, NE, 8, A, np.random.RandomState(2).randint(3, 9, size=B), seed=2)
    kw = dict(n_agents=NA, n_entities=NE, n_actions=A, agent=PLAIN, mixer=mixer)
    a_dev, a_cpu = refil_args(device="cuda", **kw), refil_args(device="cpu", **kw)
    torch.manual_seed(3)
    from maleague.modules.agents import REGISTRY as agent_REGISTRY
    mixer_p = _mixer_p(mixer, a_cpu)
    agent_p = {k: v.detach().cpu().numpy() for k, v in agent_REGISTRY[PLAIN](8 + A, a_cpu).state_dict().items()}
    e_long = _batch_from(long_b, device, NE=NE, NA=NA, A=A)
    e_short = _batch_from(short_b, device, NE=NE, NA=NA, A=A)
    L1, _ = _learner(e_long, agent_p, mixer_p, a_dev)
    L1.train(e_long, 0, episode_num=0)
    torch.cuda.synchronize()
    L2, _ = _learner(e_short, agent_p, mixer_p, a_dev)
    with torch.no_grad():
        L2._flat.flat.copy_(L1._flat.flat)
        L2._sq.copy_(L1._sq)
        L2._tflat.flat.copy_(L1._tflat.flat)
    L1.train(e_short, 0, episode_num=1)
    L2.train(e_short, 0, episode_num=1)
    torch.cuda.synchronize()
    assert torch.equal(L1._flat.flat, L2._flat.flat) and torch.equal(L1._grads, L2._grads)
    assert L1.last_stats == L2.last_stats
