"""COMA in self-play on the GPU: mlg_rollout_selfplay_policy per arm (two weight placements, one to four agent tiles per
wave, one to three action tiles, H 32 / 64 / 128) against the float64 oracle, and mlg_crossplay_rollout_policy against
per-pair launches of it. The cases, their inputs and the two-sided check are in tests/coma_selfplay_shapes.py;
tests/test_coma_selfplay.py pins, without a GPU, the arm each case is named for.

Every case first asserts through the host query (stepper.describe_rollout) that it launches the arm it is named for. Its
runs go through coma_selfplay_shapes.check_policy_sides: both batches, the returns of both sides and the episode lengths
bit-exact against stepper_ref.run_self_play under teacher forcing, every draw within DELTA = 2e-4 of the float64 cdf of
its side's own epsilon floor (0.3 home, 0.1 away) on stream index s * nh + n, every greedy pick the float64 argmax but
for near ties (at most 2 % of a side's rows), and at least 2 envs of the greedy run ending before the limit."""
import contextlib
import os

import numpy as np
import pytest
import torch

import coma_selfplay_shapes as SP
import maleague  # noqa: F401  (registers torch.ops.maleague.*)

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _fresh_envs(stepper, device):
    from maleague.envs.teams_env import VecEnvState
    stepper.envs = VecEnvState(stepper.spec, stepper.batch_size, device)


def _bytes(batch):
    return {k: batch[k].clone() for k in batch.data.transition_data}


def _assert_same(a, b, what):
    for k, v in a.items():
        assert torch.equal(v, b[k]), (what, k)


# ---- mlg_rollout_selfplay_policy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("cid", SP.IDS)
def test_rollout_selfplay_policy_case(device, cid, mask):
    """Episode 0 in train mode (epsilon floor 0.3 home / 0.1 away), episode 1 in test mode without test_greedy, episode 2
    greedy where the case lists the mask. The away batch is the stepper's reused one (rewritten in full-write mode by
    every run). At the cases on the LDS arm the train-mode episode again with MLG_ROLLOUT_GLOBAL_WEIGHTS set: every
    tensor of both batches byte-equal. At the ring cases: the home batch written into a ring that held other bytes and
    wraps equals the plain bytes, and a reused away batch equals a fresh one on the second run."""
    from maleague.components.replay_buffer import ReplayBuffer
    c = SP.case(cid)
    stepper, macs, args, (scheme, groups, preprocess) = SP.build_policy_selfplay(device, c.plan, c.H, mask)
    name, lds = stepper.describe_rollout()
    assert name == c.arm and 0 < lds <= 160 * 1024
    runs = [("train", SP.EP_TRAIN, False, True), ("draw", SP.EP_DRAW, True, False)]
    if mask in c.greedy:
        runs.append(("greedy", SP.EP_GREEDY, True, True))
    plain = None
    for tag, episode, test_mode, test_greedy in runs:
        stepper.args.test_greedy = test_greedy
        home, away, infos = stepper.run(test_mode=test_mode)
        st = {}
        SP.check_policy_sides(stepper, macs, args, (home, away), infos, episode, test_mode, mask, test_greedy, stats=st)
        L, sides = stepper.last_run["ep_len"], st["sides"]
        shares = ", ".join("%.3f %%" % (100.0 * x["near_ties"] / x["rows"]) for x in sides)
        excess = ", ".join("%.3g" % max(x["cdf_excess"], 0.0) for x in sides)
        print(f"{cid} mask={int(mask)} {tag}: rows {[x['rows'] for x in sides]}, episode lengths "
              f"{int(L.min())}..{int(L.max())}, {st['early']} of {SP.B} envs end early, "
              + (f"near ties home / away {[x['near_ties'] for x in sides]} ({shares})" if tag == "greedy"
                 else f"largest distance of a draw outside its cdf interval home / away {excess}"))
        if tag == "train":
            assert stepper.epsilons == SP.EPS
            plain = (_bytes(home), _bytes(away))
        if tag == "greedy":
            assert st["early"] >= SP.MIN_EARLY, f"{st['early']} envs end before the limit"
    stepper.args.test_greedy = True
    if c.arm.startswith("sp-policy-lds"):
        with _env(MLG_ROLLOUT_GLOBAL_WEIGHTS="1"):
            assert stepper.describe_rollout()[0] == c.arm.replace("-lds", "-global")
            _fresh_envs(stepper, device)
            home, away, _ = stepper.run(test_mode=False)
            _assert_same(plain[0], home, "global arm, home")
            _assert_same(plain[1], away, "global arm, away")
        assert stepper.describe_rollout()[0] == c.arm
    if cid not in SP.RING_CASES:
        return
    # fresh away batches, the home batch into ring slots that held other bytes (slots 30..39, 0..6)
    ring = ReplayBuffer(scheme, groups, 40, stepper.episode_limit + 1, preprocess=preprocess, device=device)
    for v in ring.data.transition_data.values():
        v.fill_(7)
    ring.buffer_index = 30
    _fresh_envs(stepper, device)
    stepper.args.reuse_away_batch = False
    assert stepper.attach_replay(ring)
    home, away, _ = stepper.run(test_mode=False)
    _assert_same(plain[0], home, "ring, home")
    _assert_same(plain[1], away, "fresh away, first run")
    _, away, _ = stepper.run(test_mode=False)  # the ring's slots are outstanding: a fresh home batch
    fresh2 = _bytes(away)
    stepper._ring = None
    _fresh_envs(stepper, device)
    stepper.args.reuse_away_batch = True  # the buffer last written by an earlier run of this test
    stepper.run(test_mode=False)
    _, away, _ = stepper.run(test_mode=False)
    _assert_same(fresh2, away, "reused away, second run")


def test_rollout_selfplay_policy_refuses_without_launching(device):
    """17 agents per side (five agent tiles per wave): the run is refused through mlg_last_error with every pointer
    valid, and the host query says the same."""
    from maleague._native import NativeError
    stepper, _, _, _ = SP.build_policy_selfplay(device, SP.REJECTED_PLAN, 32, True, n_envs=4)
    with pytest.raises(NativeError, match="agent tiles per wave"):
        stepper.run(test_mode=False)
    with pytest.raises(NativeError, match="agent tiles per wave"):
        stepper.describe_rollout()


# ---- mlg_crossplay_rollout_policy -----------------------------------------------------------------------------------
def _flat(mac):
    return torch.cat([p.detach().reshape(-1) for p in mac.agent.parameters()])


@pytest.mark.parametrize("test_greedy", [True, False], ids=["greedy", "draw"])
@pytest.mark.parametrize("plan,H", SP.CROSSPLAY_CASES, ids=[f"{p}-h{h}" for p, h in SP.CROSSPLAY_CASES])
def test_crossplay_policy_equals_per_pair_launches(device, plan, H, test_greedy):
    """Two policies, the four ordered pairs, E = 17: ep_len, ret, ret_away, won and draw bit-identical to four test-mode
    mlg_rollout_selfplay_policy launches on the global arm; the summary is the reduction of those; the games of at
    least one pair differ from another pair's (the pair index is read)."""
    from maleague.league.evaluation import PolicyCrossPlayEvaluator, build_pairs
    from maleague.runs.sp_ma_experiment import load_agent_vector
    E, ep0 = SP.B, SP.CROSSPLAY_EPISODE0
    stepper, macs, args, _ = SP.build_policy_selfplay(device, plan, H, True, n_envs=E)
    stepper.args.reuse_away_batch = False
    stepper.args.test_greedy = test_greedy
    pool = torch.stack([_flat(m) for m in macs]).clone()
    table = build_pairs(range(2), range(2))
    ref = {k: [] for k in ("ep_len", "won", "draw", "ret", "ret_away")}
    with _env(MLG_ROLLOUT_GLOBAL_WEIGHTS="1"):
        assert stepper.describe_rollout()[0].startswith("sp-policy-global")
        for h, a, _ in table.pairs.tolist():
            load_agent_vector(macs[0], pool[h])
            load_agent_vector(macs[1], pool[a])
            _fresh_envs(stepper, device)
            stepper.envs.episode.fill_(ep0)
            stepper.run(test_mode=True)
            stepper.flush()
            torch.cuda.synchronize()
            info = stepper.last_run_info().cpu().numpy().copy()
            ref["ep_len"].append(info[0:E])
            ref["won"].append(info[E:3 * E].reshape(E, 2))
            ref["draw"].append(info[3 * E:4 * E])
            ref["ret"].append(info[4 * E:5 * E])
            ref["ret_away"].append(info[5 * E:6 * E])
    ref = {k: np.stack(v) for k, v in ref.items()}
    ev_args = SP.coma_sp_args(plan, H, True, n_envs=E, test_greedy=test_greedy)
    ev = PolicyCrossPlayEvaluator(ev_args, device, episodes_per_launch=E)
    assert ev.spec_of(None).to_c().team[:] == stepper.spec.to_c().team[:]
    res = ev.evaluate(pool, table, E, episode0=ep0)
    got = {k: ev.last[k].cpu().numpy() for k in ref}
    for k in ("ep_len", "won", "draw"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    for k in ("ret", "ret_away"):
        np.testing.assert_array_equal(got[k].view(np.int32), ref[k], err_msg=k)
    assert any(not np.array_equal(got["ep_len"][0], got["ep_len"][k]) or
               not np.array_equal(got["ret"][0], got["ret"][k]) for k in range(1, 4)), "every pair played the same games"
    # the summary: the reduction of the per-env results in the documented fixed order
    w0, w1 = ref["won"][..., 0] != 0, ref["won"][..., 1] != 0
    dr = (ref["draw"] != 0) | (w0 == w1)
    want = np.zeros((4, 8), np.float32)
    want[:, 0] = E
    want[:, 1], want[:, 2], want[:, 3] = (~dr & w0).sum(1), (~dr & ~w0).sum(1), dr.sum(1)
    want[:, 6] = ref["ep_len"].sum(1)
    for col, key in ((4, "ret"), (5, "ret_away")):
        tot = np.zeros(4, np.float32)
        for e in range(E):  # E <= 64: one env per lane, lanes added in ascending order from 0
            tot = (tot + ref[key][:, e].view(np.float32)).astype(np.float32)
        want[:, col] = tot
    np.testing.assert_array_equal(ev.last["summary"].cpu().numpy(), want)
    assert res.games.tolist() == [[float(E)] * 2] * 2
    assert torch.equal(res.wins + res.losses + res.draws, res.games)
    print(f"{plan} H={H} greedy={int(test_greedy)}: episode lengths per pair "
          f"{[(int(x.min()), int(x.max())) for x in got['ep_len']]}, decided {int((~dr).sum())} of {4 * E}")
