"""The COMA shape cases shared by tests/test_coma_shapes.py (CPU: the policy dispatch table, the coverage sets, the
properties each case claims and the fp32 floors are pinned), tests/test_gpu_coma_shapes.py (GPU: oracle parity per
instantiation of mlg_rollout_policy and at the loop edges of the critic pipeline), scripts/coma_near_ties.py (CPU: the
near-tie share of the float64 oracle alone) and scripts/coma_oracle_f64_distance.py (CPU: the fp32 noise floors).

Policy rollout cases. A case is (id, H, plan, arm, seed, fc2 scale, greedy masks): ``plan`` a name helpers.shape_plan
resolves, ``arm`` what mlg_rollout_policy_describe reports, ``seed`` the stepper seed (env keys, draw stream) and the
seed of the agent weights (rollout_shapes.agent_params: numpy, so the CPU scripts play the same policy), ``fc2 scale``
the factor on fc2.weight (a sharper policy than the near-uniform initialisation), ``greedy masks`` the values of
mask_before_softmax whose greedy test-mode run is checked. B = 17 (two workgroups, the second holding one env),
episode_limit 12. Every (case, mask) runs, on fresh envs, episode 0 in train mode (epsilon 0.3), episode 1 in test
mode without test_greedy (a draw from the floor-less probabilities) and -- for the greedy masks -- episode 2 in test
mode with test_greedy.

The greedy check accepts a pick other than the oracle's argmax only at a near tie (top two masked probabilities within
DELTA = 2e-4) and caps the accepted share at NEAR_TIE_CAP = 2 %. That cap is a condition on the case: a (case, mask)
runs the greedy check only if the float64 oracle alone, rolled out over the oracle env at episode 2, sees at most 1 %
of its picks at such a gap. scripts/coma_near_ties.py counts this; its shares stand beside the cases. Without the mask
the softmax mass sits partly on unavailable actions, and sharper weights move more of it there (every available
probability falls under DELTA), so the unmasked greedy run stays off at most of the large shapes: at least one case per
action-tile count keeps it.

RO_MAXAT = 5 (the fifth 16-wide action tile, A = 5 + U > 64) is reachable: 30v30 at H = 32 is admitted
(policy-lds/tpw4, A = 65).

Critic cases run mlg_coma_critic_train twice against coma_ref.CriticRef in float64. A case's tolerances are 4x its own
fp32-vs-float64 floor: the largest |fp32 restatement - float64 restatement| per quantity over the calls, measured by
scripts/coma_oracle_f64_distance.py on the CPU (numpy's summation order differs from the kernels' ascending-row sums,
hence the factor; it is measured against the restatement, never against a kernel). The floors stand beside the cases
and in profiles/coma/oracle_f64_distance_shapes.txt; tests/test_coma_shapes.py holds the fp32 restatement to 1.05x
of them. Three comparisons missed the bound at first (A96 q_vals 9.73e-8 / 7.2e-8, stride critic_params 1.05e-6 /
8.48e-7, the learner's pi_max 7.59e-8 / 6.52e-8); traced to the one sequential chain of the critic's dense layers,
which now sum in blocks of 32 inputs (coma.hip, dense16): 3.03e-8, 5.67e-7 and 1.63e-8 since."""
from collections import namedtuple

import numpy as np

import rollout_shapes as RS

B, EPISODE_LIMIT, EPS = 17, 12, 0.3
DELTA = 2e-4
ORACLE_NEAR_TIE_CAP = 0.01
EP_TRAIN, EP_DRAW, EP_GREEDY = 0, 1, 2

PolicyCase = namedtuple("PolicyCase", "id H plan arm seed scale greedy")
_M, _U = (True,), (True, False)
# oracle near-tie share of the greedy run (episode 2), masked / unmasked; picks
POLICY_CASES = [PolicyCase(*c) for c in [
    ("lds1-h32-3v3", 32, "small", "policy-lds/tpw1", 11, 16.0, _U),               # 0.000 % / 0.000 %; 663
    ("lds1-h64-2v2", 64, "2v2", "policy-lds/tpw1", 11, 16.0, _U),                 # 0.000 % / 0.000 %; 442
    ("lds1-h64-5v7", 64, "5v7", "policy-lds/tpw1", 11, 16.0, _U),                 # 0.181 % / 0.452 %; 1105
    ("lds1-h64-3v5", 64, "3v5", "policy-lds/tpw1", 11, 16.0, _U),                 # 0.000 % / 0.603 %; 663
    ("lds1-h64-7v7", 64, "7v7", "policy-lds/tpw1", 11, 16.0, _U),                 # 0.065 % / 0.517 %; 1547
    ("global1-h64-8v8", 64, "8v8", "policy-global/tpw1", 11, 16.0, _U),           # 0.057 % / 0.509 %; 1768
    ("global1-h128-3v3", 128, "small", "policy-global/tpw1", 11, 16.0, _U),       # 0.000 % / 0.000 %; 663
    ("lds2-h32-9v9", 32, "9v9", "policy-lds/tpw2", 11, 16.0, _U),                 # 0.000 % / 0.905 %; 1989
    ("global2-h64-9v9", 64, "9v9", "policy-global/tpw2", 11, 16.0, _M),           # 0.101 % / 1.156 %; 1989
    ("global2-h128-9v9", 128, "9v9", "policy-global/tpw2", 11, 16.0, _U),         # 0.101 % / 0.654 %; 1989
    ("lds3-h32-17v17", 32, "17v17", "policy-lds/tpw3", 11, 16.0, _U),             # 0.133 % / 0.293 %; 3757
    ("global3-h64-17v17", 64, "17v17", "policy-global/tpw3", 11, 16.0, _M),       # 0.000 % / 2.901 %; 3757
    ("global3-h128-17v17", 128, "17v17", "policy-global/tpw3", 11, 16.0, _U),     # 0.027 % / 0.293 %; 3757
    ("lds4-h32-large", 32, "large", "policy-lds/tpw4", 11, 16.0, _U),             # 0.000 % / 0.253 %; 5525
    ("global4-h64-large", 64, "large", "policy-global/tpw4", 11, 16.0, _M),       # 0.217 % / 5.955 %; 5525
    ("global4-h128-large", 128, "large", "policy-global/tpw4", 11, 16.0, _M),     # 0.127 % / 5.810 %; 5525
    ("lds4-h32-30v30", 32, "30v30", "policy-lds/tpw4", 12, 8.0, _U),              # 0.106 % / 0.965 %; 6630
]]
POLICY_IDS = [c.id for c in POLICY_CASES]
# the ring-mode = plain-mode byte equality runs at one case per agent-tiles-per-wave count
RING_CASES = ["lds1-h32-3v3", "global2-h64-9v9", "lds3-h32-17v17", "global4-h64-large"]


def policy_case(cid):
    return next(c for c in POLICY_CASES if c.id == cid)


def n_action_tiles(n_actions):
    return (n_actions + 15) // 16


def policy_agent_params(c):
    """(d_in, H, n_actions) -> state_dict arrays of the case's agent before the fc2 scale."""
    return lambda d_in, hidden, n_actions: RS.agent_params(d_in, hidden, n_actions, c.seed)


def policy_spec(c, grid_size=20, episode_limit=EPISODE_LIMIT):
    from helpers import shape_plan
    from maleague.envs.teams_env import TeamsEnvSpec
    return TeamsEnvSpec.from_env_args({"match_build_plan": shape_plan(c.plan), "grid_size": grid_size,
                                       "stochastic_spawns": True, "episode_limit": episode_limit, "seed": c.seed})


def policy_describe(c):
    from helpers import drqn_dims
    from maleague import _native
    spec = policy_spec(c)
    return _native.rollout_policy_describe(spec.to_c(), drqn_dims(spec, c.H))


def oracle_policy_run(spec, hidden, seed, scale, mask, episode, mode, n_envs=B, eps=EPS, weights_seed=None,
                      agent_params=None, infos=None):
    """One run of the float64 oracle alone (oracle env, oracle DRQN, coma_ref.softmax_policy) as mlg_rollout_policy
    makes it. mode: "train" (a draw from the probabilities with the epsilon floor), "draw" (test mode without
    test_greedy: a draw from the floor-less probabilities) or "greedy" (the first-index argmax of the masked
    probabilities). -> (batch as host arrays [n_envs, episode_limit + 1, ...], episode lengths, picks, near ties: the
    picks whose top two masked probabilities lie within DELTA). ``agent_params``: a callable (d_in, H, n_actions) ->
    state_dict arrays before the fc2 scale, in place of the seeded draw; ``infos``: a dict that receives env index ->
    the env's final info."""
    import torch
    import coma_ref as CR
    import envref
    import learner_ref as LR
    from helpers import ref_envs_for
    N, A, T1 = spec.n_agents, spec.n_actions, spec.episode_limit + 1
    d_in = 8 * spec.U + A + N
    drawn = agent_params(d_in, hidden, A) if agent_params is not None else \
        RS.agent_params(d_in, hidden, A, seed if weights_seed is None else weights_seed)
    params = {k: torch.from_numpy(v).double() for k, v in drawn.items()}
    params["fc2.weight"] = params["fc2.weight"] * scale
    refs = ref_envs_for(spec, n_envs, seed=seed)
    for r in refs:
        r.episode = episode
        r.reset()
    b = {"state": np.zeros((n_envs, T1, 6 * spec.U), np.float32), "obs": np.zeros((n_envs, T1, N, 8 * spec.U), np.float32),
         "actions": np.zeros((n_envs, T1, N, 1), np.int64), "avail_actions": np.zeros((n_envs, T1, N, A), np.int32),
         "reward": np.zeros((n_envs, T1, 1), np.float32), "terminated": np.zeros((n_envs, T1, 1), np.uint8),
         "actions_onehot": np.zeros((n_envs, T1, N, A), np.float32), "filled": np.zeros((n_envs, T1, 1), np.int64)}
    eye = torch.eye(N, dtype=torch.float64).repeat(n_envs, 1)
    h = torch.zeros(n_envs * N, hidden, dtype=torch.float64)
    last = np.zeros((n_envs, N, A))
    status = [0] * n_envs  # 0 running, 1 terminated (one more pick is recorded), 2 finished
    ep_len = np.zeros(n_envs, np.int64)
    picks = near = t = 0
    while any(s < 2 for s in status):
        obs = np.stack([r.obs() for r in refs])
        avail = np.stack([r.avail() for r in refs])
        x = torch.cat([torch.from_numpy(obs.astype(np.float64).reshape(n_envs * N, -1)),
                       torch.from_numpy(last.reshape(n_envs * N, A)), eye], dim=1)
        with torch.no_grad():
            logits, h = LR.drqn_forward(params, x, h)
        p = CR.softmax_policy(logits.numpy().reshape(n_envs, N, A), avail, eps, mask, mode != "train")
        m = np.where(avail != 0, p, 0.0)
        acts = np.zeros((n_envs, N), np.int64)
        for e in range(n_envs):
            if status[e] == 2:
                continue
            key = envref.env_key(seed, e)
            for n in range(N):
                srt = np.sort(m[e, n])
                picks += 1
                near += int(srt[-1] - srt[-2] < DELTA)
                on = np.nonzero(avail[e, n])[0]
                if mode == "greedy":
                    acts[e, n] = int(on[np.argmax(m[e, n, on])]) if len(on) else 0
                    continue
                cdf = np.cumsum(m[e, n])
                thr = float(CR.policy_u(key, episode, t, n)) * cdf[-1]
                hit = [k for k in on if cdf[k] > thr]
                acts[e, n] = hit[0] if hit else (on[-1] if len(on) else 0)
        last[:] = 0
        np.put_along_axis(last, acts[:, :, None], 1.0, axis=2)
        for e, r in enumerate(refs):
            if status[e] == 2:
                last[e] = 0
                continue
            b["state"][e, t], b["obs"][e, t], b["avail_actions"][e, t] = r.state(), obs[e], avail[e]
            b["actions"][e, t, :, 0], b["actions_onehot"][e, t], b["filled"][e, t] = acts[e], last[e], 1
            if status[e] == 0:
                rew, done, info = r.step(acts[e])
                if done and infos is not None:
                    infos[e] = info
                b["reward"][e, t, 0], b["terminated"][e, t, 0] = rew[0], int(done)
                ep_len[e] = t + 1
                status[e] = 1 if done else 0
            else:
                status[e] = 2
        t += 1
    return b, ep_len, picks, near


# ---- mlg_coma_critic_train ------------------------------------------------------------------------------------------
# reward_scale multiplies the rewards; store = (episodes, T1, slot map): the batch is read out of a larger store whose
# time stride T1 exceeds cfg.T, as the learner passes a truncated sample.
CriticCase = namedtuple("CriticCase", "id B T N A d_obs S lengths reward_scale store floors")
_R272_LENGTHS = [-1, 1] + [1 + (5 * i) % 9 for i in range(32)]  # never filled, one transition, mixed 1..9
# floors: q_vals, targets, critic_stats, critic_params (scripts/coma_oracle_f64_distance.py)
CRITIC_CASES = [CriticCase(*c) for c in [
    ("A96", 2, 4, 2, 96, 8, 6, [3, 2], 1.0, None,
     (1.80e-08, 3.14e-08, 6.95e-08, 4.39e-08)),
    ("A16", 3, 4, 3, 16, 8, 6, [3, 1, 2], 1.0, None,
     (4.39e-08, 7.13e-08, 9.47e-08, 1.16e-07)),
    ("A17", 3, 4, 3, 17, 8, 6, [3, 1, 2], 1.0, None,
     (4.39e-08, 8.28e-08, 2.30e-07, 3.23e-07)),
    ("A33", 3, 4, 3, 33, 8, 6, [3, 1, 2], 1.0, None,
     (3.99e-08, 1.60e-07, 6.47e-08, 1.28e-07)),
    ("R272", 34, 9, 8, 7, 8, 6, _R272_LENGTHS, 1.0, None,
     (7.64e-08, 2.95e-07, 5.01e-08, 5.60e-08)),
    ("N32", 1, 4, 32, 5, 8, 6, [3], 1.0, None,
     (2.87e-07, 1.48e-07, 3.16e-07, 7.28e-08)),
    ("N1", 5, 4, 1, 6, 8, 6, [3, 1, 2, 3, 2], 1.0, None,
     (7.60e-08, 1.86e-07, 1.63e-07, 8.08e-08)),
    ("Tm258", 2, 259, 1, 5, 8, 6, [258, 3], 1.0, None,
     (3.33e-07, 6.62e-07, 1.96e-06, 2.20e-07)),
    ("clip", 3, 4, 3, 11, 8, 6, [3, 2, 3], 200.0, None,
     (9.12e-08, 2.13e-05, 1.88e-03, 4.39e-07)),
    ("stride", 3, 6, 2, 7, 8, 6, [1, 8, 4, 5, 2], 1.0, (5, 9, [3, 0, 4]),
     (9.52e-08, 1.22e-07, 3.47e-07, 2.12e-07)),
]]
CRITIC_IDS = [c.id for c in CRITIC_CASES]
CRITIC_KEYS = ("q_vals", "targets", "critic_stats", "critic_params")
ZERO_WORKSPACE_CASE = "A17"
PARAM_SEED, BATCH_SEED = 31, 41
TARGET_INTERVAL = 200  # the target critic follows after 200 steps: between the two calls of Tm258 only


def critic_case(cid):
    return next(c for c in CRITIC_CASES if c.id == cid)


def critic_tol(c):
    return {k: 4.0 * v for k, v in zip(CRITIC_KEYS, c.floors)}


def critic_blocks(c):
    """The gradient blocks (256 parameters each) of the case: the length of the norm's partial-sum array."""
    D = c.S + c.d_obs + 2 * c.N * c.A + c.N
    return (128 * D + 128 + 128 * 128 + 128 + c.A * 128 + c.A + 255) // 256


def critic_data(c):
    """-> (critic parameters, the store as host arrays, the slot map or None, the batch the call sees: the store's
    slots, cut to cfg.T)."""
    from helpers import _random_batch, _random_critic
    D = c.S + c.d_obs + 2 * c.N * c.A + c.N
    pc = _random_critic(D, c.A, PARAM_SEED)
    n_store, T1, slots = c.store if c.store else (c.B, c.T, None)
    lengths = list(c.lengths)
    store = _random_batch(n_store, T1, c.N, c.A, c.d_obs, c.S, [max(L, 1) for L in lengths], BATCH_SEED)
    for e, L in enumerate(lengths):
        if L < 0:  # an episode slot that was never filled: every key zero
            for v in store.values():
                v[e] = 0
    store["reward"] *= np.float32(c.reward_scale)
    batch = store if slots is None else {k: v[slots] for k, v in store.items()}
    batch = {k: v[:, :c.T] for k, v in batch.items()}
    return pc, store, slots, batch


def run_critic_ref(c, dtype=np.float64, calls=2, defect=None, ascending=False):
    """The restatement's outputs per call: dicts of q_vals, targets, critic_stats (the five means), critic_params
    (flat), taken, steps, norms. ``defect``: one of CriticRef.DEFECTS (the checks that a comparison would notice)."""
    import coma_ref as CR
    pc, _, _, batch = critic_data(c)
    ref = CR.CriticRef(pc, dtype=dtype, defect=defect, ascending=ascending)
    out = []
    for _ in range(calls):
        q, tg, sums, taken = ref.train(batch)
        ref.maybe_update_target(TARGET_INTERVAL)
        assert q.dtype == dtype and tg.dtype == dtype and all(v.dtype == dtype for v in ref.p.values())
        out.append(dict(q_vals=q, targets=tg, critic_stats=sums / max(taken, 1), taken=taken, steps=ref.steps,
                        critic_params=np.concatenate([ref.p[k].reshape(-1) for k in CR.CRITIC_KEYS]),
                        norms=list(ref.norms)))
    return out


def distance(a, b, keys):
    """The largest |a - b| per key over the calls."""
    return {k: max(float(np.abs(np.asarray(x[k], np.float64) - np.asarray(y[k], np.float64)).max())
                   for x, y in zip(a, b)) for k in keys}


# ---- the actor loss ----------------------------------------------------------------------------------------------------
# (id, B, Tm, N, A): rows x N = 360 takes two passes of the 256-thread stride loop. Every case has padding rows but
# R1, whose one row must be live (R1pad is that row next to a padding row).
ACTOR_CASES = [("R360", 9, 8, 5, 11), ("R1", 1, 1, 1, 7), ("R1pad", 2, 1, 1, 7), ("A1", 3, 5, 4, 1),
               ("A96", 3, 5, 4, 96)]


def actor_inputs(B, Tm, N, A, seed=9):
    """pi, avail, actions, q, mask as float64 / integer arrays; the last row of every episode but the first is padding
    (avail all zero, mask zero). With one row only, that row is live and the padding is an agent row without actions."""
    rng = np.random.RandomState(seed)
    pi = rng.dirichlet(np.ones(A), size=(B, Tm, N))
    avail = (rng.rand(B, Tm, N, A) < 0.6).astype(np.int32)
    actions = np.zeros((B, Tm, N, 1), np.int64)
    for idx in np.ndindex(B, Tm, N):
        if not avail[idx].any():
            avail[idx][rng.randint(A)] = 1
        actions[idx][0] = rng.choice(np.nonzero(avail[idx])[0])
    mask = (rng.rand(B, Tm, 1) < 0.7).astype(np.float64)
    mask[0, 0] = 1
    for e in range(1, B):
        avail[e, Tm - 1] = 0
        actions[e, Tm - 1] = 0
        mask[e, Tm - 1] = 0
    q = rng.randn(B, Tm, N, A)
    return pi, avail, actions, q, mask


# ---- the learner off the fixture shape ----------------------------------------------------------------------------
# COMALearner on the policy rollout's own batch: 9v9 at H = 64, 8 envs, episode limit LEARNER_LIMIT; the sample is cut
# to the longest episode, so max_seq_length is below the storage length. Floors (three calls, the batch the float64
# oracle alone rolls out at the same shape): q_vals, targets, critic_stats, actor_stats, critic_params, agent_params.
LEARNER_CASE = PolicyCase("learner-h64-9v9", 64, "9v9", "policy-global/tpw2", 11, 8.0, ())
LEARNER_B, LEARNER_LIMIT, LEARNER_MASK = 8, 64, True
LEARNER_KEYS = ("q_vals", "targets", "critic_stats", "actor_stats", "critic_params", "agent_params")
LEARNER_FLOORS = (8.43e-07, 2.26e-07, 1.07e-07, 1.63e-08, 4.98e-07, 1.06e-07)
CRITIC_STATS = ["critic_loss", "critic_grad_norm", "td_error_abs", "q_taken_mean", "target_mean"]
ACTOR_STATS = ["advantage_mean", "coma_loss", "agent_grad_norm", "pi_max"]


def learner_tol():
    return {k: 4.0 * v for k, v in zip(LEARNER_KEYS, LEARNER_FLOORS)}


def learner_spec():
    from helpers import shape_plan
    from maleague.envs.teams_env import TeamsEnvSpec
    c = LEARNER_CASE
    return TeamsEnvSpec.from_env_args({"match_build_plan": shape_plan(c.plan), "grid_size": 20,
                                       "stochastic_spawns": True, "episode_limit": LEARNER_LIMIT, "seed": c.seed})


def learner_params(spec):
    """(agent parameters with the fc2 scale applied, critic parameters) of the learner case, as float32 arrays."""
    from helpers import _random_critic
    c = LEARNER_CASE
    N, A = spec.n_agents, spec.n_actions
    pa = RS.agent_params(8 * spec.U + A + N, c.H, A, c.seed)
    pa["fc2.weight"] = (pa["fc2.weight"] * np.float32(c.scale)).astype(np.float32)
    return pa, _random_critic(6 * spec.U + 8 * spec.U + 2 * N * A + N, A, PARAM_SEED)


def run_learner_ref(batch, spec, dtype=np.float64, calls=3):
    """LearnerRef over ``batch`` (host arrays, cut to the longest episode): per call the dict of LEARNER_KEYS."""
    import coma_ref as CR
    import learner_ref as LR
    pa, pc = learner_params(spec)
    ref = CR.LearnerRef(pa, pc, spec.n_agents, EPS, LEARNER_MASK, dtype=dtype)
    out = []
    for _ in range(calls):
        stats, q, tg = ref.train(batch)
        out.append(dict(q_vals=q, targets=tg, critic_stats=np.array([stats[k] for k in CRITIC_STATS], np.float64),
                        actor_stats=np.array([stats[k] for k in ACTOR_STATS], np.float64), stats=stats,
                        critic_params=np.concatenate([ref.critic.p[k].reshape(-1) for k in CR.CRITIC_KEYS]),
                        agent_params=np.concatenate([ref.agent[k].detach().numpy().reshape(-1)
                                                     for k in LR.AGENT_KEYS])))
    return out


def learner_oracle_batch():
    """The train-mode batch the float64 oracle alone rolls out for the learner case, cut to its longest episode."""
    spec = learner_spec()
    c = LEARNER_CASE
    b, ep_len, _, _ = oracle_policy_run(spec, c.H, c.seed, c.scale, LEARNER_MASK, 0, "train", n_envs=LEARNER_B)
    T = int(ep_len.max()) + 1
    return spec, {k: v[:, :T] for k, v in b.items()}, ep_len
