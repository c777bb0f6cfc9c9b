"""The distinct-network self-play rollout cases shared by tests/test_distinct_selfplay.py (CPU: the dispatch table of
mlg_rollout_selfplay_distinct is pinned through mlg_rollout_selfplay_distinct_describe),
tests/test_gpu_distinct_selfplay.py (GPU: oracle parity per dispatch arm and edge) and
scripts/distinct_selfplay_near_ties.py (CPU: the near-tie share of the float64 oracle alone). It follows
tests/distinct_shapes.py.

A case is (id, rnn_hidden_dim, plan, obs_last_action, arm, seed, fc2_scale): ``plan`` is a name
helpers.shape_plan(name, self_play=True) resolves (nh agents per side: one tile per agent of either side, 2 nh tiles),
``arm`` what mlg_rollout_selfplay_distinct_describe reports for it, ``seed`` the stepper seed (env keys, epsilon
streams) and the seed of the home side's nh networks (distinct_ref.agent_params: numpy, so the CPU script plays the same
weights); the away side's nh networks are seeded apart, at ``seed + AWAY_SEED``. ``fc2_scale`` a factor on every fc2.

B = 37: three 16-env workgroups, the last with 5 live columns in every tile. Episode limit 30. A test-mode run of
episode 0, then a train-mode run of episode 1 at epsilon 0.525 (home) and 0.3 (away).

Seeds follow the rule of tests/distinct_shapes.py: the GPU checker accepts a greedy pick that differs from the oracle's
argmax only at a near tie (top-two masked Q within Q_TOL = 1e-4) and caps the accepted share at 1 % of a case's greedy
picks; a (seed, fc2_scale) is kept only if the float64 oracle alone, rolled out on the CPU over the oracle env at the
same B and episode limit with both sides' weights, sees at most 0.5 % of its greedy picks at such a gap.
scripts/distinct_selfplay_near_ties.py counts it; the share is written beside each case.

Arms: 2 nh tiles on min(2 nh, 8) waves, wave w owns tiles w, w + W, ...: nh 1..4 is tpw1, 5..8 tpw2, 9..12 tpw3,
13..16 tpw4; 17 agents per side are refused. With nh = 5 the 10 tiles sit on 8 waves: waves 0 and 1 own two tiles (one
of each side: tiles 0 / 8 and 1 / 9), waves 2..7 one.
"""
B, EPISODE_LIMIT = 37, 30
T_ENV = 25000
EPS = max(0.05, 1.0 - 0.95 / 50000 * T_ENV)  # 0.525, the home schedule's value at T_ENV
EPS_AWAY = 0.3                               # the away selector's own epsilon
AWAY_SEED = 50                               # away networks: distinct_ref.agent_params(i, ..., seed + AWAY_SEED)

# (id, H, plan, obs_last_action, arm, seed, fc2_scale)                            oracle near-tie share (picks)
CASES = [
    ("dxsp-n1-h64", 64, "1v1", True, "dxsp-global/tpw1", 11, 1.0),                # 0.027 % (1 / 3659)
    ("dxsp-n3-h64", 64, "small", True, "dxsp-global/tpw1", 11, 1.0),              # 0.210 % (23 / 10966)
    ("dxsp-n3-h32", 32, "small", True, "dxsp-global/tpw1", 11, 1.0),              # 0.036 % (4 / 10966)
    ("dxsp-n3-h128", 128, "small", True, "dxsp-global/tpw1", 11, 1.0),            # 0.000 % (0 / 10966)
    ("dxsp-n5-h64-nola", 64, "medium_1h_4t", False, "dxsp-global/tpw2", 11, 1.0),  # 0.159 % (29 / 18188)
    ("dxsp-n9-h64", 64, "9v9", True, "dxsp-global/tpw3", 11, 1.0),                # 0.122 % (40 / 32741)
    ("dxsp-n16-h32", 32, "16v16", True, "dxsp-global/tpw4", 11, 1.0),             # 0.088 % (51 / 58173); the last admitted shape
]
IDS = [c[0] for c in CASES]

# ring mode and equal networks against two BasicMACs: 3 and 9 agents per side (tpw1 and tpw3)
RING_CASES = ["dxsp-n3-h64", "dxsp-n9-h64"]
SHARED_CASES = ["dxsp-n3-h64", "dxsp-n9-h64"]

# the describe table of tests/test_distinct_selfplay.py: agents per side -> arm, None = refused
DESCRIBE = [(4, "dxsp-global/tpw1"), (5, "dxsp-global/tpw2"), (8, "dxsp-global/tpw2"), (9, "dxsp-global/tpw3"),
            (12, "dxsp-global/tpw3"), (13, "dxsp-global/tpw4"), (16, "dxsp-global/tpw4"), (17, None)]

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


def dims_of(spec, hidden, last_action=True, agent_id=False):
    """One side's MlgAgentDims over the self-play ``spec`` (n_agents = nh)."""
    from maleague import _native
    nh, A = spec.n_agents // 2, spec.n_actions
    return _native.MlgAgentDims(d_obs=8 * spec.U, n_actions=A, n_agents=nh, hidden=hidden,
                                d_in=8 * spec.U + (A if last_action else 0) + (nh if agent_id else 0),
                                obs_last_action=int(last_action), obs_agent_id=int(agent_id))


def side_params(nh, d_in, hidden, n_actions, seed, fc2_scale=1.0):
    """(home, away): each side's nh per-agent parameter dicts (numpy), the away side seeded apart."""
    import distinct_ref as DR
    return (DR.all_agent_params(nh, d_in, hidden, n_actions, seed, fc2_scale),
            DR.all_agent_params(nh, d_in, hidden, n_actions, seed + AWAY_SEED, fc2_scale))
