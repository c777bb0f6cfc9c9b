"""The two-policy COMA rollout cases shared by tests/test_coma_selfplay.py (CPU: the describe table, the rejections, the
registries, the near-tie conditions of the two smallest cases), tests/test_gpu_coma_selfplay.py (GPU: oracle parity of
mlg_rollout_selfplay_policy per arm, cross-play bit-identity) and scripts/coma_selfplay_near_ties.py (CPU: the near-tie
shares and the early-ending envs of the float64 oracle alone).

Inputs follow tests/mix_shapes.py: random self-play policies never end an episode before the limit on the 20-cell grid,
so the cases play grid_size 8, episode_limit 40, env seed 11, B = 17 (the second workgroup holds one env), the plan
helpers.shape_plan(name, self_play=True). Weights: rollout_shapes.agent_params(d_in, H, A, 11) for home, seed 12 for
away, then fc2.weight *= 4, fc2.bias[5:] += 2.0 (prefer the attack actions), fc2.bias[3] += 0.7 for home and
fc2.bias[4] += 0.7 for away (advance towards each other). Train-mode epsilon floor 0.3 for home and 0.1 for away: unequal,
so that a launch that read one side's floor for both would miss the other side's cdf by far more than DELTA. Every
(case, mask) runs episode 0 in train mode, episode 1 in test mode without test_greedy and -- where listed -- episode 2
greedy.

A case is (id, plan, H, arm, greedy masks): ``arm`` what mlg_rollout_selfplay_policy_describe reports (two H = 32 images
fit next to the env state up to 14 agents per side -- 158144 B of the 160 KiB; 15v15 and 16v16 read global memory),
``greedy masks`` the values of mask_before_softmax whose greedy run is checked. The rule is coma_shapes': a (case, mask)
runs the greedy check only where the float64 oracle alone sees at most 1 % near ties (top two masked probabilities
within DELTA = 2e-4) on each side; the GPU check then accepts at most 2 % of a side's rows. Each greedy GPU run also
asserts at least MIN_EARLY envs ending before the limit. scripts/coma_selfplay_near_ties.py counts both with the oracle
alone; its figures stand beside the cases (masked home / away, unmasked home / away, early-ending envs of 17 masked).
The last two cases add the LDS arm at two and at four tiles per wave (14v14: the largest plan on it), which the first
seven do not reach."""
from collections import namedtuple

import numpy as np

import coma_shapes as CS
import rollout_shapes as RS

GRID, EPISODE_LIMIT, SEED, B = 8, 40, 11, 17
EPS = (0.3, 0.1)  # train-mode epsilon floor: home, away
FC2_SCALE, ATTACK_SHIFT, ADVANCE_SHIFT = 4.0, 2.0, 0.7
DELTA, ORACLE_NEAR_TIE_CAP, NEAR_TIE_CAP = CS.DELTA, CS.ORACLE_NEAR_TIE_CAP, 0.02
MIN_EARLY = 2
EP_TRAIN, EP_DRAW, EP_GREEDY = 0, 1, 2

Case = namedtuple("Case", "id plan H arm greedy")
_M, _U = (True,), (True, False)
CASES = [Case(*c) for c in [
    ("3v3-h32", "3v3", 32, "sp-policy-lds/tpw1", _U),         # 0.056 % / 0.000 %, 0.845 % / 0.225 %; 7
    ("3v3-h128", "3v3", 128, "sp-policy-global/tpw1", _M),    # 0.000 % / 0.000 %, 0.285 % / 2.740 %; 6
    ("5v5-h64", "5v5", 64, "sp-policy-global/tpw2", _U),      # 0.183 % / 0.000 %, 0.916 % / 0.672 %; 5
    ("9v9-h32", "9v9", 32, "sp-policy-lds/tpw3", _M),         # 0.018 % / 0.018 %, 0.352 % / 1.726 %; 8
    ("9v9-h64", "9v9", 64, "sp-policy-global/tpw3", _M),      # 0.053 % / 0.071 %, 1.068 % / 0.623 %; 7
    ("16v16-h32", "16v16", 32, "sp-policy-global/tpw4", _M),  # 0.082 % / 0.128 %, 1.113 % / 2.245 %; 4
    ("16v16-h64", "16v16", 64, "sp-policy-global/tpw4", _M),  # 0.075 % / 0.093 %, 1.392 % / 1.654 %; 4
    ("5v5-h32", "5v5", 32, "sp-policy-lds/tpw2", _M),         # 0.000 % / 0.064 %, 0.900 % / 1.254 %; 5
    ("14v14-h32", "14v14", 32, "sp-policy-lds/tpw4", _M),     # 0.103 % / 0.069 %, 2.286 % / 2.514 %; 9
]]
IDS = [c.id for c in CASES]
RING_CASES = ["3v3-h32", "9v9-h64"]
# cross-play: two policies (the case's home and away weights), the four ordered pairs, E = 17
CROSSPLAY_CASES = [("3v3", 32), ("5v5", 64), ("9v9", 128)]
CROSSPLAY_EPISODE0 = 3
REJECTED_PLAN = "17v17"  # five agent tiles per wave


def case(cid):
    return next(c for c in CASES if c.id == cid)


def env_args(plan):
    from helpers import shape_plan
    return {"match_build_plan": shape_plan(plan, self_play=True), "grid_size": GRID, "stochastic_spawns": True,
            "episode_limit": EPISODE_LIMIT, "seed": SEED}


def spec_of(plan):
    from maleague.envs.teams_env import TeamsEnvSpec
    return TeamsEnvSpec.from_env_args(env_args(plan))


def describe(plan, H):
    from helpers import drqn_dims
    from maleague import _native
    spec = spec_of(plan)
    return _native.rollout_selfplay_policy_describe(spec.to_c(), drqn_dims(spec, H, self_play=True))


def side_params(side, d_in, hidden, n_actions):
    """state_dict arrays (float32) of side 0 (home) / 1 (away) with the scale and the bias shifts described above."""
    p = RS.agent_params(d_in, hidden, n_actions, SEED + side)
    p["fc2.weight"] = (p["fc2.weight"] * np.float32(FC2_SCALE)).astype(np.float32)
    b = p["fc2.bias"].astype(np.float32).copy()
    b[5:] += np.float32(ATTACK_SHIFT)
    b[3 + side] += np.float32(ADVANCE_SHIFT)
    p["fc2.bias"] = b
    return p


def pick_from(m, on, u):
    """The multinomial rule on the masked probabilities m: the first available k whose running sum exceeds u * total,
    else the last available k (0 without one)."""
    cdf = np.cumsum(m)
    thr = u * cdf[-1]
    hit = [k for k in on if cdf[k] > thr]
    return int(hit[0]) if hit else (int(on[-1]) if len(on) else 0)


def oracle_run(plan, hidden, mask, mode, episode, n_envs=B):
    """One run of the float64 oracle alone (oracle env, learner_ref.drqn_forward, coma_ref.softmax_policy) as
    mlg_rollout_selfplay_policy makes it: side s picks with its own weights and its own floor EPS[s] on the stream index
    s * nh + n. mode: "train", "draw" (test mode without test_greedy) or "greedy". -> (episode lengths, picks per side,
    near ties per side: the picks whose top two masked probabilities lie within DELTA)."""
    import torch
    import coma_ref as CR
    import envref
    import learner_ref as LR
    from helpers import ref_envs_for
    spec = spec_of(plan)
    N2, A = spec.n_agents, spec.n_actions
    nh = N2 // 2
    d_in = 8 * spec.U + A + nh
    P = [{k: torch.from_numpy(v).double() for k, v in side_params(s, d_in, hidden, A).items()} for s in range(2)]
    refs = ref_envs_for(spec, n_envs, seed=SEED)
    for r in refs:
        r.episode = episode
        r.reset()
    eye = torch.eye(nh, dtype=torch.float64).repeat(n_envs, 1)
    h = [torch.zeros(n_envs * nh, hidden, dtype=torch.float64) for _ in range(2)]
    last = np.zeros((n_envs, N2, A))
    status = [0] * n_envs  # 0 running, 1 terminated (one more pick is recorded), 2 finished
    ep_len = np.zeros(n_envs, np.int64)
    picks, near, t = [0, 0], [0, 0], 0
    while any(s < 2 for s in status):
        obs = np.stack([r.obs() for r in refs])
        avail = np.stack([r.avail() for r in refs])
        acts = np.zeros((n_envs, N2), np.int64)
        for s in range(2):
            sl = slice(s * nh, (s + 1) * nh)
            x = torch.cat([torch.from_numpy(obs[:, sl].astype(np.float64).reshape(n_envs * nh, -1)),
                           torch.from_numpy(last[:, sl].reshape(n_envs * nh, A)), eye], dim=1)
            with torch.no_grad():
                logits, h[s] = LR.drqn_forward(P[s], x, h[s])
            p = CR.softmax_policy(logits.numpy().reshape(n_envs, nh, A), avail[:, sl], EPS[s], mask, mode != "train")
            m = np.where(avail[:, sl] != 0, p, 0.0)
            for e in range(n_envs):
                if status[e] == 2:
                    continue
                key = envref.env_key(SEED, e)
                for n in range(nh):
                    on = np.nonzero(avail[e, s * nh + n])[0]
                    srt = np.sort(m[e, n])
                    picks[s] += 1
                    near[s] += int(srt[-1] - srt[-2] < DELTA)
                    if mode == "greedy":
                        acts[e, s * nh + n] = int(on[np.argmax(m[e, n, on])]) if len(on) else 0
                    else:
                        acts[e, s * nh + n] = pick_from(m[e, n], on, float(CR.policy_u(key, episode, t, s * nh + n)))
        last[:] = 0
        np.put_along_axis(last, acts[:, :, None], 1.0, axis=2)
        for e, r in enumerate(refs):
            if status[e] == 2:
                last[e] = 0
            elif status[e] == 0:
                _, done, _ = r.step(acts[e])
                ep_len[e] += 1
                status[e] = 1 if done else 0
            else:
                status[e] = 2
        t += 1
    return ep_len, picks, near


# ---- GPU side: the stepper of a case and the two-sided check ---------------------------------------------------------
def coma_sp_args(plan, H, mask, n_envs=B, **kw):
    from helpers import coma_args
    a = dict(batch_size_run=n_envs, seed=SEED, rnn_hidden_dim=H, mask_before_softmax=mask, epsilon_start=EPS[0],
             epsilon_finish=EPS[0], test_greedy=True, env_args=env_args(plan))
    a.update(kw)
    return coma_args(**a)


def build_policy_selfplay(device, plan, H, mask, n_envs=B, stepper_cls=None):
    """A SelfPlayPolicyParallelStepper over ``plan`` with two pi_logits BasicMACs holding side_params; the home
    selector's schedule is flat at EPS[0], the away selector's at EPS[1]. -> (stepper, (home, away), args, (scheme,
    groups, preprocess))."""
    import copy
    import torch
    from helpers import scheme_for
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import SelfPlayPolicyParallelStepper
    args = coma_sp_args(plan, H, mask, n_envs)
    stepper = (stepper_cls or SelfPlayPolicyParallelStepper)(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(dict(info, n_agents=args.n_agents), torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    away_args = copy.copy(args)
    away_args.epsilon_start = away_args.epsilon_finish = EPS[1]
    macs = (BasicMAC(proto.scheme, groups, args), BasicMAC(proto.scheme, groups, away_args))
    for s, mac in enumerate(macs):
        d = mac.agent.dims()
        mac.agent.load_state_dict({k: torch.from_numpy(v) for k, v in side_params(s, d.d_in, H, d.n_actions).items()})
        mac.agent.mark_dirty()
    stepper.initialize(scheme, groups, preprocess, *macs)
    return stepper, macs, args, (scheme, groups, preprocess)


def check_policy_sides(stepper, macs, args, batches, infos, episode, test_mode, mask, test_greedy=True, stats=None):
    """The two-sided form of helpers.check_sides / helpers._check_policy_run. Env tensors, filled, one-hots, rewards,
    returns, away returns and episode lengths bit-exact against stepper_ref.run_self_play, teacher-forced with the
    recorded actions of both sides; then every pick of side s against the float64 policy of that side's weights along
    its recorded batch: a draw within DELTA of the cdf built with that side's own epsilon floor on stream index
    s * nh + n, a greedy pick the argmax but for near ties (at most NEAR_TIE_CAP of the side's rows). ``stats``
    receives per side rows, near_ties and cdf_excess (the largest distance of a draw outside its cdf interval), and
    early: the envs ending before the limit."""
    import torch
    import coma_ref as CR
    import envref
    import learner_ref as LR
    import stepper_ref
    from helpers import np_batch, ref_envs_for
    spec = stepper.spec
    n_envs, nh, A, T1 = stepper.batch_size, spec.n_agents // 2, spec.n_actions, stepper.episode_limit + 1
    nbs = [np_batch(b) for b in batches]
    ep_len = stepper.last_run["ep_len"].numpy()
    assert (ep_len >= 1).all() and (ep_len <= stepper.episode_limit).all()
    refs = ref_envs_for(spec, n_envs, seed=args.seed)
    for r in refs:
        r.episode = episode
    pol = [lambda t, run, b, s=s: nbs[s]["actions"][run, t, :, 0] for s in range(2)]
    out = stepper_ref.run_self_play(stepper_ref.RefVecEnv(refs), pol[0], pol[1], n_envs, T1, nh, A, 8 * spec.U,
                                    6 * spec.U, test_mode=test_mode)
    for s, key in enumerate(("home", "away")):
        for k, v in out[key].items():
            np.testing.assert_array_equal(nbs[s][k], v, err_msg=f"{key}[{k}]")
    np.testing.assert_array_equal(stepper.last_run["returns"].numpy(), np.float32(out["returns"][0]))
    np.testing.assert_array_equal(stepper.last_run["away_returns"].numpy(), np.float32(out["returns"][1]))
    np.testing.assert_array_equal(ep_len, out["home"]["filled"][:, :, 0].sum(axis=1) - 1)
    assert stepper.t == out["t"] and [infos[i] for i in range(n_envs)] == out["env_infos"]
    if not test_mode:
        assert int(ep_len.sum()) == out["env_steps"]
    greedy = bool(test_mode and test_greedy)
    Tm = int(ep_len.max()) + 1
    per_side = []
    for s, (mac, nb) in enumerate(zip(macs, nbs)):
        params = {k: v.detach().cpu().double() for k, v in mac.agent.state_dict().items()}
        tb = {k: torch.from_numpy(nb[k]).double() for k in ("obs", "actions_onehot")}
        with torch.no_grad():
            logits, _ = LR.mac_unroll(params, tb, nh, T=Tm,
                                      h0=torch.zeros(n_envs * nh, args.rnn_hidden_dim, dtype=torch.float64))
        avail = nb["avail_actions"][:, :Tm]
        m = np.where(avail != 0, CR.softmax_policy(logits.numpy(), avail, EPS[s], mask, test_mode), 0.0)
        rows = near = 0
        worst = 0.0
        for b in range(n_envs):
            key = envref.env_key(args.seed, b)
            for t in range(int(ep_len[b]) + 1):
                for n in range(nh):
                    a = int(nb["actions"][b, t, n, 0])
                    assert avail[b, t, n, a] != 0, (s, b, t, n, a)
                    rows += 1
                    if greedy:
                        srt = np.sort(m[b, t, n])
                        if srt[-1] - srt[-2] < DELTA:
                            near += 1
                            assert m[b, t, n, a] >= srt[-1] - DELTA, (s, b, t, n, a)
                        else:
                            assert a == int(np.argmax(m[b, t, n])), (s, b, t, n, a)
                        continue
                    cdf = np.cumsum(m[b, t, n])
                    thr = float(CR.policy_u(key, episode, t, s * nh + n)) * cdf[-1]
                    lo = cdf[a - 1] if a > 0 else 0.0
                    worst = max(worst, lo - thr, thr - cdf[a])
                    assert lo - DELTA <= thr < cdf[a] + DELTA, (s, b, t, n, a, lo, thr, cdf[a])
        assert rows == int((ep_len + 1).sum()) * nh
        per_side.append({"rows": rows, "near_ties": near, "cdf_excess": worst})
        if greedy:
            assert near <= NEAR_TIE_CAP * rows, f"side {s}: {near} near-tie rows of {rows}"
    if stats is not None:
        stats.update(sides=per_side, early=int((ep_len < stepper.episode_limit).sum()))
    return per_side
