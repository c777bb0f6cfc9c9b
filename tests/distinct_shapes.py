"""The distinct-network rollout cases shared by tests/test_distinct.py (CPU: the dispatch table of mlg_rollout_distinct
is pinned through mlg_rollout_distinct_describe), tests/test_gpu_distinct.py (GPU: oracle parity per dispatch arm and
edge) and scripts/distinct_near_ties.py (CPU: the near-tie share of the float64 oracle alone).

A case is (id, rnn_hidden_dim, plan, obs_last_action, arm, seed, fc2_scale): ``plan`` is a name helpers.shape_plan
resolves (its policy team has N agents: one tile per agent), ``arm`` what mlg_rollout_distinct_describe reports for it,
``seed`` the stepper seed (env keys, epsilon stream) and the seed of the N agents' weights
(distinct_ref.agent_params: numpy, so the CPU script plays the same weights), ``fc2_scale`` a factor on every fc2.

B = 37: three 16-env workgroups, the last with 5 live columns in every tile. Episode limit 30. A test-mode run of
episode 0, then a train-mode run of episode 1 at epsilon 0.525.

Seeds follow the rule of tests/dqn_shapes.py: the GPU checker accepts a greedy pick that differs from the oracle's
argmax only at a near tie (top-two masked Q within Q_TOL = 1e-4) and caps the accepted share at 1 % of the greedy
picks; a (seed, fc2_scale) is kept only if the float64 oracle alone, rolled out on the CPU over the oracle env at the
same B and episode limit, sees at most 0.5 % of its greedy picks at such a gap. scripts/distinct_near_ties.py counts
it; the share is written beside each case.

Arms: wave w owns tiles w, w + 8, ..., so N <= 8 is tpw1, 9..16 tpw2, 17..24 tpw3, 25..32 tpw4; 33 agents are refused.
"""
B, EPISODE_LIMIT = 37, 30
T_ENV = 25000
EPS = max(0.05, 1.0 - 0.95 / 50000 * T_ENV)  # 0.525, the schedule's value at T_ENV

# (id, H, plan, obs_last_action, arm, seed, fc2_scale)                       oracle near-tie share (picks)
CASES = [
    ("dx-n1-h64", 64, "1v1", True, "dx-global/tpw1", 11, 1.0),               # 0.000 % (0 / 1696)
    ("dx-n3-h64", 64, "small", True, "dx-global/tpw1", 11, 1.0),             # 0.176 % (9 / 5109)
    ("dx-n3-h32", 32, "small", True, "dx-global/tpw1", 11, 1.0),             # 0.215 % (11 / 5109)
    ("dx-n3-h128", 128, "small", True, "dx-global/tpw1", 11, 1.0),           # 0.157 % (8 / 5109)
    ("dx-n5-h64-nola", 64, "medium_1h_4t", False, "dx-global/tpw1", 11, 1.0),  # 0.083 % (7 / 8451)
    ("dx-n9-h64", 64, "9v9", True, "dx-global/tpw2", 11, 1.0),               # 0.191 % (29 / 15192)
    ("dx-n17-h32", 32, "17v17", True, "dx-global/tpw3", 11, 1.0),            # 0.056 % (16 / 28658)
    ("dx-n25-h64", 64, "25v25", True, "dx-global/tpw4", 11, 1.0),            # 0.071 % (30 / 42181)
    ("dx-n32-h32", 32, "32v32", True, "dx-global/tpw4", 11, 1.0),            # 0.087 % (47 / 54057); the last admitted shape
]
IDS = [c[0] for c in CASES]

# ring mode: one tpw1 and one tpw3 case; shared weights against BasicMAC: 3 and 9 agents
RING_CASES = ["dx-n3-h64", "dx-n17-h32"]
SHARED_CASES = ["dx-n3-h64", "dx-n9-h64"]

# the describe table of tests/test_distinct.py: (policy agents, scripted units) -> arm, None = refused
DESCRIBE = [((8, 8), "dx-global/tpw1"), ((9, 9), "dx-global/tpw2"), ((32, 32), "dx-global/tpw4"), ((33, 31), None)]


def case(cid):
    return next(c for c in CASES if c[0] == cid)


def plan_of(n_policy, n_scripted):
    """A plan of ``n_policy`` policy agents against ``n_scripted`` scripted units (units TR AR HR TM cyclically,
    scripted team first, as helpers.shape_plan's "KvK")."""
    from helpers import _UNIT_CYCLE
    from maleague.envs.plans import team_from_codes
    codes = lambda k: " ".join(_UNIT_CYCLE[i % 4] for i in range(k))  # noqa: E731
    return [team_from_codes(codes(n_scripted), True), team_from_codes(codes(n_policy), False)]


def spec_of(plan, seed=0, grid_size=20, episode_limit=EPISODE_LIMIT):
    from helpers import shape_plan
    from maleague.envs.teams_env import TeamsEnvSpec
    return TeamsEnvSpec.from_env_args({"match_build_plan": shape_plan(plan) if isinstance(plan, str) else plan,
                                       "grid_size": grid_size, "stochastic_spawns": True, "episode_limit": episode_limit,
                                       "seed": seed})


def dims_of(spec, hidden, last_action=True, agent_id=False):
    from maleague import _native
    N, A = spec.n_agents, spec.n_actions
    return _native.MlgAgentDims(d_obs=8 * spec.U, n_actions=A, n_agents=N, hidden=hidden,
                                d_in=8 * spec.U + (A if last_action else 0) + (N if agent_id else 0),
                                obs_last_action=int(last_action), obs_agent_id=int(agent_id))
