"""The QMIX learner's skipped work (learner.hip Skip): steps past the episodes of a 16-row tile, mixer rows past an
episode's last live transition, and the target pass while the target parameters are a bit copy of the online ones.
Everything skipped is exactly redundant, so the default path must equal MLG_LEARNER_FULL=1 (every row to
max_t_filled, both nets) under ==, also with the workspace filled with NaN before each call (no kernel may read a
workspace element that the call did not write), and stats[7] must report the planned forward blocks.

Batch: the 5v5 dims of the golden fixtures (H = 64), B = 7 episodes of episode_limit 12 (T = 13), R = 35 agent rows:
three 16-row tiles (the last with 3 rows), nine 4-row tiles (the last with 3 rows). Filled counts
[13, 2, 9, 5, 7, 6, 4]: the limit (cut by it, never terminated), the minimum, the others terminated at their last
transition; with 5 agents per episode every episode boundary falls inside a 4-row tile. Steps past an episode's end
are zeros, as a rollout leaves them. Tile lengths (max count over a tile's episodes): [13, 7, 4].
"""
import copy

import numpy as np
import pytest
import torch

import learner_ref as LR
from helpers import qmix_args, scheme_for

pytestmark = pytest.mark.gpu

FILLED = [13, 2, 9, 5, 7, 6, 4]
LIMIT = 12
STAT_KEYS = ["loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean"]


class _Log:
    def log_stat(self, k, v, t):
        pass

    def info(self, *a):
        pass


def _dims(d):
    b = LR.batch_from_npz(d)
    return {"state_shape": b["state"].shape[-1], "obs_shape": b["obs"].shape[-1],
            "n_actions": b["avail_actions"].shape[-1], "n_agents": b["obs"].shape[2]}


def _batch_dict(info):
    """The synthetic batch as CPU tensors with the scheme's dtypes."""
    rs = np.random.RandomState(7)
    B, T, N, A = len(FILLED), LIMIT + 1, info["n_agents"], info["n_actions"]
    filled = np.zeros((B, T, 1), np.int64)
    term = np.zeros((B, T, 1), np.uint8)
    for b, f in enumerate(FILLED):
        filled[b, :f] = 1
        if f < T:
            term[b, f - 2] = 1  # the episode's last transition ends it
    live = filled.astype(np.float32)
    avail = (rs.rand(B, T, N, A) < 0.6).astype(np.int32)
    avail[..., 0] = 1
    actions = np.zeros((B, T, N, 1), np.int64)
    for idx in np.ndindex(B, T, N):
        actions[idx][0] = rs.choice(np.flatnonzero(avail[idx]))
    onehot = np.zeros((B, T, N, A), np.float32)
    np.put_along_axis(onehot, actions, 1.0, axis=-1)
    lv4 = live[:, :, None, :]
    out = {
        "state": rs.randn(B, T, info["state_shape"]).astype(np.float32) * live,
        "obs": rs.randn(B, T, N, info["obs_shape"]).astype(np.float32) * lv4,
        "actions": actions * filled[:, :, None, :],
        "avail_actions": avail * filled[:, :, None, :].astype(np.int32),
        "reward": rs.randn(B, T, 1).astype(np.float32) * live,
        "terminated": term,
        "actions_onehot": onehot * lv4,
        "filled": filled,
    }
    return {k: torch.from_numpy(v) for k, v in out.items()}


def _planned_blocks(n_agents, nets):
    """stats[7] in numpy: per 16-row tile the longest filled count of its episodes, clamped to [2, max_t_filled]."""
    f = np.asarray(FILLED)
    te = int(np.clip(f.max(), 2, LIMIT + 1))
    R = len(f) * n_agents
    total = 0
    for r0 in range(0, R, 16):
        eps = np.arange(r0, min(R, r0 + 16)) // n_agents
        total += int(np.clip(f[eps].max(), 2, te))
    return float(total * nets), float(((R + 15) // 16) * te * 2)


@pytest.fixture(scope="module")
def case(golden):
    d = golden("qlearner_qmix_dq.npz")
    info = _dims(d)
    agent0 = {k[len("p0.agent."):]: np.array(d[k]) for k in d.files if k.startswith("p0.agent.")}
    mixer0 = {k[len("p0.mixer."):]: np.array(d[k]) for k in d.files if k.startswith("p0.mixer.")}
    return info, agent0, mixer0, _batch_dict(info)


def _learner(case, device, args):
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    from maleague.learners import QLearner
    info, agent0, mixer0, tb = case
    scheme, groups, preprocess = scheme_for(info, torch)
    eb = EpisodeBatch(scheme, groups, len(FILLED), LIMIT + 1, preprocess=preprocess, device=device)
    for k, v in tb.items():
        eb.data.transition_data[k].copy_(v)
    assert eb.data.transition_data["filled"].sum(dim=(1, 2)).tolist() == FILLED
    mac = BasicMAC(eb.scheme, eb.groups, args)
    mac.load_state_dict({k: torch.from_numpy(v) for k, v in agent0.items()})
    learner = QLearner(mac, eb.scheme, _Log(), args, name="home")
    if args.mixer == "qmix":
        msd = {k: torch.from_numpy(v) for k, v in mixer0.items()}
        learner.mixer.load_state_dict(msd)
        learner.target_mixer.load_state_dict(msd)
    learner.build_optimizer()
    return learner, eb


def _ulp(t, idx):
    """t with element idx moved by one ulp (a copy)."""
    a = t.detach().cpu().numpy().copy()
    a[idx] = np.nextafter(a[idx], np.float32(np.inf), dtype=np.float32)
    return torch.from_numpy(a)


def _perturb_target(learner, qmix=True):
    """One target fc2 weight and one target mixer weight moved by one ulp, through load_state_dict."""
    sd = {k: v.detach().clone() for k, v in learner.target_mac.agent.state_dict().items()}
    sd["fc2.weight"] = _ulp(sd["fc2.weight"], (3, 5)).to(sd["fc2.weight"].device)
    learner.target_mac.agent.load_state_dict(sd)
    if qmix:
        sd = {k: v.detach().clone() for k, v in learner.target_mixer.state_dict().items()}
        sd["hyper_w_1.2.weight"] = _ulp(sd["hyper_w_1.2.weight"], (7, 11)).to(sd["hyper_w_1.2.weight"].device)
        learner.target_mixer.load_state_dict(sd)


def _snapshot(learner):
    torch.cuda.synchronize()
    return {"stats": learner._stats.cpu().numpy().copy(), "grads": learner._grads.cpu().numpy().copy(),
            "params": learner._flat.flat.cpu().numpy().copy(), "sq": learner._sq.cpu().numpy().copy()}


def _nan_workspace(learner, eb):
    from maleague import _native
    lib = _native.load(require_gpu=True)
    cfg = learner._cfg(eb.batch_size, eb.max_seq_length)
    need = int(lib.mlg_qlearner_workspace_floats(_native.byref(cfg)))
    if learner._ws is None:
        learner._ws = torch.empty(int(need * 1.25) + 1024, dtype=torch.float32, device=learner.device)
    assert learner._ws.numel() >= need
    learner._ws.fill_(float("nan"))


def _run(case, device, monkeypatch, full, episodes, args=None, before=None, nan_fill=False):
    """train() once per entry of `episodes` (the episode_num of the call); before[i](learner) runs ahead of call i."""
    if full:
        monkeypatch.setenv("MLG_LEARNER_FULL", "1")
    else:
        monkeypatch.delenv("MLG_LEARNER_FULL", raising=False)
    learner, eb = _learner(case, device, args or qmix_args())
    out = []
    for i, ep in enumerate(episodes):
        if before and before.get(i):
            before[i](learner)
        if nan_fill:
            _nan_workspace(learner, eb)
        learner.train(eb, i, ep)
        out.append(_snapshot(learner))
    monkeypatch.delenv("MLG_LEARNER_FULL", raising=False)
    return out


def _assert_same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.all(np.isfinite(g["stats"])), f"{what} call {i}: stats {g['stats']}"
        assert np.array_equal(g["stats"][:7], w["stats"][:7]), f"{what} call {i}: {g['stats']} vs {w['stats']}"
        for k in ("grads", "params", "sq"):
            assert np.array_equal(g[k], w[k]), f"{what} call {i}: {k} differ at {np.flatnonzero(g[k] != w[k])[:8]}"


def test_skip_path_equals_full_path(case, device, monkeypatch):
    """Three consecutive calls; the second is due a target update (episode 200), so the target is a copy in calls 1
    and 3 and stale in call 2. The default path runs on a workspace refilled with NaN before every call."""
    n = case[0]["n_agents"]
    eps = [0, 200, 200]
    got = _run(case, device, monkeypatch, False, eps, nan_fill=True)
    want = _run(case, device, monkeypatch, True, eps)
    _assert_same(got, want, "skip vs full")
    for i, nets in enumerate([1, 2, 1]):
        blocks, full_blocks = _planned_blocks(n, nets)
        assert got[i]["stats"][7] == blocks, f"call {i}"
        assert want[i]["stats"][7] == full_blocks, f"call {i} (full)"
    assert _planned_blocks(n, 1)[0] == 13 + 7 + 4


def test_target_copy_runs_no_target_blocks(case, device, monkeypatch):
    """(a) the target is a bit copy: no target block planned, results equal to the full path."""
    got = _run(case, device, monkeypatch, False, [0])
    want = _run(case, device, monkeypatch, True, [0])
    _assert_same(got, want, "copy")
    assert got[0]["stats"][7] == _planned_blocks(case[0]["n_agents"], 1)[0]


def test_target_one_ulp_off_runs_both_nets(case, device, monkeypatch):
    """(b) one target mixer weight and one target fc2 weight one ulp off: both nets planned, equal to the full path."""
    before = {0: _perturb_target}
    got = _run(case, device, monkeypatch, False, [0], before=before)
    want = _run(case, device, monkeypatch, True, [0], before=before)
    _assert_same(got, want, "one ulp")
    assert got[0]["stats"][7] == _planned_blocks(case[0]["n_agents"], 2)[0]


def test_target_loaded_between_calls_runs_target_pass(case, device, monkeypatch):
    """(c) a target update after call 0 makes the target a copy; it is then changed through load_state_dict with no
    sync: call 1 must see it (no host-side flag could) and run the target pass."""
    def load(learner):
        sd = {k: v.detach().clone() for k, v in learner.target_mac.agent.state_dict().items()}
        sd["fc2.bias"] = sd["fc2.bias"] + 0.25
        learner.target_mac.agent.load_state_dict(sd)

    eps = [200, 200]
    n = case[0]["n_agents"]
    got = _run(case, device, monkeypatch, False, eps, before={1: load})
    want = _run(case, device, monkeypatch, True, eps, before={1: load})
    _assert_same(got, want, "loaded target")
    assert got[0]["stats"][7] == _planned_blocks(n, 1)[0]
    assert got[1]["stats"][7] == _planned_blocks(n, 2)[0]
    unchanged = _run(case, device, monkeypatch, False, eps)
    assert unchanged[1]["stats"][7] == _planned_blocks(n, 1)[0]
    assert not np.array_equal(unchanged[1]["grads"], got[1]["grads"]), "the loaded target changed nothing"


@pytest.mark.parametrize("ulp", [False, True], ids=["copy", "one_ulp"])
@pytest.mark.parametrize("kw", [{}, {"mixer": "vdn"}, {"double_q": False}], ids=["qmix", "vdn", "no_double_q"])
def test_skip_path_vs_oracle(case, device, monkeypatch, kw, ulp):
    """One call against the CPU oracle with the tolerances of test_gpu_learner.py, target a copy / one ulp off."""
    monkeypatch.delenv("MLG_LEARNER_FULL", raising=False)
    info, agent0, mixer0, tb = case
    args = qmix_args(**kw)
    qmix = args.mixer == "qmix"
    learner, eb = _learner(case, device, args)
    ref = LR.QLearnerRef(agent0, mixer0 if qmix else None, copy.copy(args))
    if ulp:
        _perturb_target(learner, qmix)
        ref.tp["fc2.weight"] = _ulp(ref.tp["fc2.weight"], (3, 5))
        if qmix:
            ref.tmp["hyper_w_1.2.weight"] = _ulp(ref.tmp["hyper_w_1.2.weight"], (7, 11))
    want = ref.train({k: v.clone() for k, v in tb.items()}, 0, 0)
    learner.train(eb, 0, 0)
    for k in STAT_KEYS:
        np.testing.assert_allclose(learner.last_stats[k], want[k], rtol=2e-4, atol=1e-6, err_msg=k)
    assert learner._stats[7].item() == _planned_blocks(info["n_agents"], 2 if ulp else 1)[0]
    for k, v in learner.mac.agent.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), ref.agent_state()[k].numpy(), atol=5e-5, rtol=0, err_msg=k)
    if qmix:
        for k, v in learner.mixer.state_dict().items():
            np.testing.assert_allclose(v.cpu().numpy(), ref.mixer_state()[k].numpy(), atol=5e-5, rtol=0, err_msg=k)
