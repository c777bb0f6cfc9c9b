"""The feed-forward self-play rollout cases shared by tests/test_dqn_selfplay.py (CPU: the dispatch table of
mlg_rollout_selfplay_ff is pinned through mlg_rollout_selfplay_ff_describe), tests/test_gpu_dqn_selfplay.py (GPU: oracle
parity per dispatch arm and edge) and scripts/dqn_selfplay_near_ties.py (CPU: the near-tie share of the float64 oracle
alone). It follows tests/distinct_selfplay_shapes.py.

A case is (id, rnn_hidden_dim, plan, obs_last_action, obs_agent_id, arm, seed, fc2_scale): ``plan`` is a name
helpers.shape_plan(name, self_play=True) resolves (nh agents per side: nh 16-row tiles per side, 2 nh tiles), ``arm``
what mlg_rollout_selfplay_ff_describe reports for it, ``seed`` the stepper seed (env keys, epsilon streams) and the seed
of the home weights (dqn_ref.agent_params: numpy, so the CPU script plays the same weights); the away weights are seeded
apart, at ``seed + AWAY_SEED``. ``fc2_scale`` a factor on fc2.

B = 37: three 16-env workgroups, the last with 5 live envs. Episode limit 30. A test-mode run of episode 0, then a
train-mode run of episode 1 at epsilon 0.525 (home) and 0.3 (away).

Seeds follow the rule of tests/distinct_shapes.py: the GPU checker accepts a greedy pick that differs from the oracle's
argmax only at a near tie (top-two masked Q within Q_TOL = 1e-4) and caps the accepted share at 1 % of a case's greedy
picks; a (seed, fc2_scale) is kept only if the float64 oracle alone, rolled out on the CPU over the oracle env at the
same B and episode limit with both sides' weights, sees at most 0.5 % of its greedy picks at such a gap.
scripts/dqn_selfplay_near_ties.py counts it; the share is written beside each case.

Arms: 2 nh tiles on min(2 nh, 8) waves, wave w owns tiles w, w + W, ...: nh 1..4 is tpw1, 5..8 tpw2, 9..12 tpw3,
13..16 tpw4; 17 agents per side are refused. Both sides' weight images sit in LDS beside the env state (ffsp-lds) while
they fit in 160 KiB: every H = 32 shape, H = 64 up to 12 agents per side, H = 128 up to 5; past that the weights are
read from global memory (ffsp-global). ffsp-global/tpw1 is reached by no admitted shape of its own accord (two images of
at most 4 agents per side always fit) and ffsp-global/tpw2 only by 6 to 8 agents per side at H = 128: both are run
through MLG_ROLLOUT_GLOBAL_WEIGHTS at 3v3 and 5v5 (LDS_VS_GLOBAL), where they must store the bytes of the lds arm that
the parity cases check. The flag-off cases move the w1a / w1n offsets and so the base of the away image in LDS.
"""
B, EPISODE_LIMIT = 37, 30
T_ENV = 25000
EPS = max(0.05, 1.0 - 0.95 / 50000 * T_ENV)  # 0.525, the home schedule's value at T_ENV
EPS_AWAY = 0.3                               # the away selector's own epsilon
AWAY_SEED = 50                               # away weights: dqn_ref.agent_params(..., seed + AWAY_SEED)

# (id, H, plan, obs_last_action, obs_agent_id, arm, seed, fc2_scale)                     oracle near-tie share (picks)
CASES = [
    ("ffsp-n1-h64", 64, "1v1", True, True, "ffsp-lds/tpw1", 11, 1.0),                    # 0.000 % (0 / 3659)
    ("ffsp-n2-h64", 64, "2v2", True, True, "ffsp-lds/tpw1", 11, 1.0),                    # 0.000 % (0 / 7334)
    ("ffsp-n3-h32", 32, "small", True, True, "ffsp-lds/tpw1", 11, 1.0),                  # 0.009 % (1 / 10966)
    ("ffsp-n3-h64", 64, "small", True, True, "ffsp-lds/tpw1", 11, 1.0),                  # 0.082 % (9 / 10966)
    ("ffsp-n3-h128", 128, "small", True, True, "ffsp-lds/tpw1", 11, 1.0),                # 0.082 % (9 / 10966)
    ("ffsp-n3-h32-noid", 32, "small", True, False, "ffsp-lds/tpw1", 11, 1.0),            # 0.073 % (8 / 10966)
    ("ffsp-n5-h64", 64, "medium_1h_4t", True, True, "ffsp-lds/tpw2", 11, 1.0),           # 0.077 % (14 / 18188)
    ("ffsp-n5-h64-nola", 64, "medium_1h_4t", False, True, "ffsp-lds/tpw2", 11, 1.0),     # 0.099 % (18 / 18188)
    ("ffsp-n5-h64-bare", 64, "medium_1h_4t", False, False, "ffsp-lds/tpw2", 11, 1.0),    # 0.022 % (4 / 18188)
    ("ffsp-n7-h64", 64, "7v7", True, True, "ffsp-lds/tpw2", 11, 1.0),                    # 0.083 % (21 / 25451)
    ("ffsp-n9-h64", 64, "9v9", True, True, "ffsp-lds/tpw3", 11, 1.0),                    # 0.101 % (33 / 32741)
    ("ffsp-n9-h128", 128, "9v9", True, True, "ffsp-global/tpw3", 11, 1.0),               # 0.113 % (37 / 32741)
    ("ffsp-n13-h128", 128, "13v13", True, True, "ffsp-global/tpw4", 11, 1.0),            # 0.112 % (53 / 47262)
    ("ffsp-n16-h32", 32, "16v16", True, True, "ffsp-lds/tpw4", 11, 1.0),                 # 0.084 % (49 / 58173)
    ("ffsp-n16-h64", 64, "16v16", True, True, "ffsp-global/tpw4", 11, 1.0),              # 0.084 % (49 / 58173); the last admitted shape
]
IDS = [c[0] for c in CASES]

# ring mode: 3 and 9 agents per side (tpw1 and tpw3)
RING_CASES = ["ffsp-n3-h64", "ffsp-n9-h64"]
# the lds arm against the forced global arm: (case, the arm MLG_ROLLOUT_GLOBAL_WEIGHTS gives)
LDS_VS_GLOBAL = [("ffsp-n3-h64", "ffsp-global/tpw1"), ("ffsp-n5-h64", "ffsp-global/tpw2")]
# the CPU test rolls the float64 oracle itself for these (about 2 s each)
ORACLE_CASES = ["ffsp-n1-h64", "ffsp-n3-h64"]

# the describe table of tests/test_dqn_selfplay.py: agents per side -> arm at H = 32 / 64 / 128, None = refused
DESCRIBE = [(4, ("ffsp-lds/tpw1", "ffsp-lds/tpw1", "ffsp-lds/tpw1")),
            (5, ("ffsp-lds/tpw2", "ffsp-lds/tpw2", "ffsp-lds/tpw2")),
            (8, ("ffsp-lds/tpw2", "ffsp-lds/tpw2", "ffsp-global/tpw2")),
            (9, ("ffsp-lds/tpw3", "ffsp-lds/tpw3", "ffsp-global/tpw3")),
            (12, ("ffsp-lds/tpw3", "ffsp-lds/tpw3", "ffsp-global/tpw3")),
            (13, ("ffsp-lds/tpw4", "ffsp-global/tpw4", "ffsp-global/tpw4")),
            (16, ("ffsp-lds/tpw4", "ffsp-global/tpw4", "ffsp-global/tpw4")),
            (17, None)]

# cross-play: (plan, H, second roster in the spec table)
CROSSPLAY_CASES = [("small", 64, True), ("medium_1h_4t", 32, False)]
CROSSPLAY_E, CROSSPLAY_POOL, CROSSPLAY_EPISODE0 = 20, 3, 3


def case(cid):
    return next(c for c in CASES if c[0] == cid)


def spec_of(plan, seed=0, grid_size=20, episode_limit=EPISODE_LIMIT):
    """The self-play env spec of a plan name (both teams policy-controlled) or of a list of two team dicts."""
    from helpers import shape_plan
    from maleague.envs.teams_env import TeamsEnvSpec
    return TeamsEnvSpec.from_env_args({"match_build_plan": shape_plan(plan, self_play=True) if isinstance(plan, str)
                                       else plan, "grid_size": grid_size, "stochastic_spawns": True,
                                       "episode_limit": episode_limit, "seed": seed})


def dims_of(spec, hidden, last_action=True, agent_id=True):
    """One side's MlgAgentDims over the self-play ``spec`` (n_agents = nh)."""
    from maleague import _native
    nh, A = spec.n_agents // 2, spec.n_actions
    return _native.MlgAgentDims(d_obs=8 * spec.U, n_actions=A, n_agents=nh, hidden=hidden,
                                d_in=8 * spec.U + (A if last_action else 0) + (nh if agent_id else 0),
                                obs_last_action=int(last_action), obs_agent_id=int(agent_id))


def side_params(d_in, hidden, n_actions, seed, fc2_scale=1.0):
    """(home, away): each side's parameter dict (numpy), the away side seeded apart."""
    import dqn_ref as DQ
    return (DQ.agent_params(d_in, hidden, n_actions, seed, fc2_scale),
            DQ.agent_params(d_in, hidden, n_actions, seed + AWAY_SEED, fc2_scale))


def oracle_q(mac, tb, N, T, dtype=None):
    """dqn_ref.oracle_q with the input flags of ``mac.args`` (dqn_ref.oracle_q builds inputs with both flags on; with
    both on this is that function): Q [B, T, N, A] along a recorded batch with ``mac``'s parameters."""
    import torch
    import dqn_ref as DQ
    params = {k: v.detach().cpu() for k, v in mac.agent.state_dict().items()}
    tb = {k: tb[k] for k in ("obs", "actions_onehot")}
    if dtype is not None:
        params = {k: v.to(dtype) for k, v in params.items()}
        tb = {k: v.to(dtype) for k, v in tb.items()}
    with torch.no_grad():
        return DQ.mac_unroll(params, tb, N, T=T, last_action=bool(mac.args.obs_last_action),
                             agent_id=bool(mac.args.obs_agent_id)).numpy()


def near_ties(plan, hidden, last_action, agent_id, seed, fc2_scale):
    """(greedy picks, near ties among them, epsilon draws) of the float64 oracle alone over both runs of a case, both
    sides: the oracle env (both teams policy-controlled), dqn_ref.dqn_forward with each side's weights, epsilon draws
    from the counter RNG as the kernel makes them (one epsilon per side, the global agent index s * nh + ln as the
    stream index, the side-local index ln as the agent id input)."""
    import numpy as np
    import torch
    import envref
    import dqn_ref as DQ
    from helpers import Q_TOL, ref_envs_for
    spec = spec_of(plan, seed)
    N, A = spec.n_agents, spec.n_actions
    nh = N // 2
    d_in = 8 * spec.U + (A if last_action else 0) + (nh if agent_id else 0)
    ps = [{k: torch.from_numpy(v).double() for k, v in p.items()}
          for p in side_params(d_in, hidden, A, seed, fc2_scale)]
    ids = torch.eye(nh, dtype=torch.float64).repeat(2, 1).unsqueeze(0).expand(B, N, nh)
    picks = ties = draws = 0
    for episode, eps in ((0, (0.0, 0.0)), (1, (EPS, EPS_AWAY))):
        refs = ref_envs_for(spec, B, seed=seed)
        for r in refs:
            r.episode = episode
            r.reset()
        last = np.zeros((B, N, A))
        status = [0] * B  # 0 running, 1 terminated (one more pick is recorded), 2 finished
        t = 0
        while any(s < 2 for s in status):
            obs = torch.from_numpy(np.stack([r.obs() for r in refs]).astype(np.float64))
            avail = np.stack([r.avail() for r in refs])
            acts = np.zeros((B, N), np.int64)
            x = torch.cat([obs] + ([torch.from_numpy(last)] if last_action else []) + ([ids] if agent_id else []), dim=2)
            with torch.no_grad():
                q = torch.cat([DQ.dqn_forward(ps[s], x[:, s * nh:(s + 1) * nh]) for s in range(2)], dim=1).numpy()
            for b in range(B):
                if status[b] == 2:
                    continue
                key = envref.env_key(seed, b)
                for n in range(N):
                    av = avail[b, n]
                    e = eps[n >= nh]
                    if e > 0 and envref.u01(envref.rng(key, envref.ctr(episode, t, 2, n))) < np.float32(e):
                        acts[b, n] = envref.random_available(av.tolist(), envref.rng(key, envref.ctr(episode, t, 3, n)))
                        draws += 1
                        continue
                    m = np.where(av == 0, -np.inf, q[b, n])
                    srt = np.sort(m)
                    picks += 1
                    ties += int(not srt[-1] - srt[-2] > Q_TOL)
                    acts[b, n] = int(np.argmax(m))
            last[:] = 0
            np.put_along_axis(last, acts[:, :, None], 1.0, axis=2)
            for b, r in enumerate(refs):
                if status[b] == 0:
                    _, done, _ = r.step(acts[b])
                    status[b] = 1 if done else 0
                elif status[b] == 1:
                    status[b] = 2
            t += 1
    return picks, ties, draws
