"""The opponent-mixture cases shared by tests/test_mix.py (CPU: ABI, describe table, refusals, group assignment,
LeagueInstance on a fake experiment) and tests/test_gpu_selfplay_mix.py / tests/test_gpu_league_mix.py (GPU:
bit-identity of mlg_rollout_selfplay_mix with per-opponent mlg_rollout_selfplay launches).

Inputs. Random self-play policies almost never end an episode before the limit on the 20-cell grid, which would leave
the early-termination, final-action and tail-zeroing paths of a mixed workgroup untested. The cases therefore play
grid_size 8, episode_limit 40, env seed 11, obs_last_action / obs_agent_id on, with weights
distinct_ref.agent_params(i, d_in, H, A, 11) (i = 0: home, i = k + 1: away policy k), fc2.bias[5:] += 2.0 (prefer the
attack actions), fc2.bias[3] += 0.7 for home and fc2.bias[4] += 0.7 for the away policies (advance towards each other).
With the float64 oracle alone the envs ending before the limit in the test-mode run, per opponent, are
    small H64         B 37 table [0, 1, 2]        6 / 6 / 2 of 16 / 16 / 5     (14)
    medium_1h_4t H64  B 80 table [0, 1, 1, 2, 0]  4 / 10 / 1 of 32 / 32 / 16   (15)
    4v4 H64           B 37 table [0, 1, 2]        1 / 5 / 1                    (7)
    small H32         B 37 table [0, 1, 2]        6 / 6 / 2                    (14)
and the train-mode runs at epsilon 0.525 / 0.3 give 6, 4, 5 and 5 in total. Each GPU case asserts on its own
test-mode run: at least MIN_EARLY early-ending envs in total and at least one in the groups of two different opponents
(a condition on the inputs, not a tolerance).
"""
import numpy as np

GRID, EPISODE_LIMIT, SEED = 8, 40, 11
T_ENV = 25000
EPS_HOME = max(0.05, 1.0 - 0.95 / 50000 * T_ENV)  # 0.525, the schedule's value at T_ENV
EPS_AWAY = 0.3
N_OPPONENTS = 3
MIN_EARLY = 3
GROUP_ENVS = 16

# (id, plan, H, B, group -> opponent table, arm under the default environment)
MIX_CASES = [
    ("small-h64", "small", 64, 37, [0, 1, 2], "sp8-mix"),
    ("medium_1h_4t-h64", "medium_1h_4t", 64, 80, [0, 1, 1, 2, 0], "sp8-mix"),
    ("4v4-h64", "4v4", 64, 37, [0, 1, 2], "v1-mix"),
    ("small-h32", "small", 32, 37, [0, 1, 2], "v1-mix"),
]
# the uniform-mixture cases add H = 128 (v1-mix: the generic kernel's third width)
UNIFORM_CASES = MIX_CASES + [("small-h128", "small", 128, 37, [0, 1, 2], "v1-mix")]
# describe table: the rows above, plus the 3v3 H = 64 shape with the generic kernel forced
DESCRIBE_CASES = [(c[0], c[1], c[2], None, c[5]) for c in UNIFORM_CASES] + \
    [("small-h64-forced-v1", "small", 64, "v1", "v1-mix")]


def case(cid, cases=None):
    return next(c for c in (cases or UNIFORM_CASES) if c[0] == cid)


def arm_of(name):
    """The arm of a describe name ("v1-mix/tpw2" -> "v1-mix")."""
    return name.split("/")[0]


def env_args(plan):
    from helpers import shape_plan
    return {"match_build_plan": shape_plan(plan, self_play=True) if isinstance(plan, str) else plan,
            "grid_size": GRID, "stochastic_spawns": True, "episode_limit": EPISODE_LIMIT, "seed": SEED}


def policy_params(i, d_in, hidden, n_actions):
    """state_dict arrays of policy i (0: home, k + 1: away policy k) with the bias shifts described above."""
    from distinct_ref import agent_params
    p = agent_params(i, d_in, hidden, n_actions, SEED)
    b = p["fc2.bias"].copy()
    b[5:] += np.float32(2.0)
    b[3 if i == 0 else 4] += np.float32(0.7)
    p["fc2.bias"] = b
    return p


def flat_row(p):
    """named_parameters() order: fc1.weight, fc1.bias, gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh,
    fc2.weight, fc2.bias."""
    order = ["fc1.weight", "fc1.bias", "gru.weight_ih", "gru.weight_hh", "gru.bias_ih", "gru.bias_hh", "fc2.weight",
             "fc2.bias"]
    return np.concatenate([np.asarray(p[k], dtype=np.float32).reshape(-1) for k in order])


def group_envs(table, B):
    """opponent -> env indices of its groups."""
    out = {}
    for b in range(B):
        out.setdefault(table[b // GROUP_ENVS], []).append(b)
    return out
