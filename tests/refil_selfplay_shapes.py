"""The REFIL self-play cases shared by tests/test_refil_selfplay.py (CPU: dispatch names, spec, refusals),
tests/test_gpu_refil_selfplay.py (GPU: oracle parity of mlg_refil_rollout_selfplay per side) and
scripts/refil_selfplay_near_ties.py (CPU: the float64 oracle's own self-play, the seed selection rule below).

A case: both teams field the same ``codes`` (S unit slots per team, U = 2S entities, A = 5 + U actions, k ~
U{kmin..kmax} active slots per episode, the same k for both teams), ``la`` = entity_last_action, ``arm`` what
mlg_refil_rollout_selfplay_describe reports, ``seed`` the env seed (env keys, epsilon streams), ``seed_home`` /
``seed_away`` the seeds of the two sides' weights (refil_shapes.entity_agent_params: numpy, so the CPU script plays the
same policies) and ``bias_*`` = (attack_bias, move_bias, ally_bias, noop_bias) added to that side's fc3.bias
(refil_selfplay_ref.side_params): the away side is pushed towards the enemy so that the oracle's own play moves,
targets and, on refil_8, wins battles as away -- the away side's actions demonstrably reach the env.

Seeds. As tests/refil_shapes.py: the checker accepts a greedy pick that differs from the float64 oracle's argmax only at
a near tie (top-two masked Q within Q_TOL = 1e-4), the GPU tests cap the accepted share at 1 % of a case's decisions
per side, and a seed is kept only if the float64 oracle alone (B = 37, episode_limit 30, grid 20: the test-mode run of
episode 0 and the train-mode run of episode 1 at eps_home = 0.525, eps_away = 0.3) sees at most 0.5 % of either side's
decisions at such a gap. The shares scripts/refil_selfplay_near_ties.py counted are written beside each case.
"""
from collections import namedtuple

import refil_shapes as FS

B, EPISODE_LIMIT, GRID = FS.B, FS.EPISODE_LIMIT, FS.GRID
EPS_HOME, EPS_AWAY = FS.EPS, 0.3
RUNS = ((0, 0.0, 0.0), (1, EPS_HOME, EPS_AWAY))  # (episode, eps_home, eps_away): test mode, then train mode

Case = namedtuple("Case", "id codes kmin kmax la arm seed seed_home seed_away bias_home bias_away")

# (attack_bias, move_bias, ally_bias, noop_bias)
NONE, PUSH = (0.0, 0.0, 0.0, 0.0), (1.0, 0.5, 0.0, 0.0)
STAND = (-5.0, 0.0, -5.0, 5.0)   # a home side that holds its ground: the away side has to come and win
CHARGE = (5.0, 2.0, 0.0, 0.0)
APPROACH = (0.0, 1.0, 0.0, 0.0)

# Beside each case: the oracle's near-tie share home / away (near ties / decisions) and what its own play did over the two
# runs (away wins, away move actions, away target actions). With random weights alone no battle of 3+ units a side ends
# inside 30 steps on a 20-grid (the teams spawn 12+ columns apart), so refil_8 pairs a home side that holds its ground
# with a charging away side, and its env seed (5) was chosen among 1..40 as one where that away side wins a battle.
SP_CASES = [
    # 0.000 % (0 / 8831) / 0.000 % (0 / 10607); 1 win, 11074, 1030
    Case("refil_8", FS._codes(8), 3, 8, True, "sp-ro2/kc2", 5, 11, 23, STAND, CHARGE),
    # 0.033 % (2 / 6027) / 0.086 % (6 / 6937); 0 wins, 7336, 656
    Case("s5", FS._codes(5), 2, 5, True, "sp-ro2/kc2", 11, 11, 23, NONE, PUSH),
    # 0.000 % (0 / 3391) / 0.000 % (0 / 3905); 1 win, 4180, 290
    Case("s3", FS._codes(3), 1, 3, True, "sp-ro2/kc2", 11, 11, 23, NONE, PUSH),
    # 0.000 % (0 / 1696) / 0.000 % (0 / 1963); 0 wins, 2161, 59
    Case("s1", FS._codes(1), 1, 1, True, "sp-ro2/kc1", 11, 11, 23, NONE, PUSH),
    # 0.000 % (0 / 8551) / 0.000 % (0 / 10949); 0 wins, 11147, 1453
    Case("s8-nola", FS._codes(8), 3, 8, False, "sp-ro2/kc1", 11, 13, 23, APPROACH, CHARGE),
]


def case(cid):
    return next(c for c in SP_CASES if c.id == cid)


def plan(codes):
    """match_build_plan of a case: two policy teams with the same unit slots."""
    from maleague.envs.plans import team_from_codes
    return [team_from_codes(codes, False), team_from_codes(codes, False)]


def env_args(c, seed=None):
    return {"match_build_plan": plan(c.codes), "grid_size": GRID, "stochastic_spawns": True,
            "episode_limit": EPISODE_LIMIT, "min_agents": c.kmin, "max_agents": c.kmax,
            "seed": c.seed if seed is None else seed}


def spec_for(c, seed=None, self_play=True):
    from maleague.envs.entity_env import EntityEnvSpec
    return EntityEnvSpec.from_env_args(env_args(c, seed), self_play=self_play)


def side_dims(spec, la=True):
    """The MlgRefilDims of ONE side's entity agent over ``spec`` (what agent.dims() returns), without building one."""
    from maleague import _native
    return _native.MlgRefilDims(n_agents=spec.S, n_entities=spec.n_entities, entity_shape=8,
                                n_actions=spec.n_actions, entity_last_action=int(la), attn_embed_dim=64, attn_n_heads=4,
                                rnn_hidden_dim=64)
