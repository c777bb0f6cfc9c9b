"""The REFIL rollout shape cases shared by tests/test_refil_dispatch.py (CPU: the dispatch of mlg_refil_rollout is
pinned through mlg_refil_rollout_describe), tests/test_gpu_refil_shapes.py (GPU: oracle parity per slot count and arm)
and scripts/refil_near_ties.py (CPU: the near-tie share of the float64 oracle alone, the seed selection rule below).

A case is (id, unit codes of one side, min_agents, max_agents, env override or None, arm, seed): both teams field the
same ``codes`` (S unit slots per team, U = 2 S entities, A = 5 + U actions, k ~ U{min_agents..max_agents} active slots
per episode), ``env`` is a dict of MLG_REFIL_* variables set for the case, ``arm`` the kernel
mlg_refil_rollout_describe reports under that environment, ``seed`` the env seed (env keys, epsilon stream) and the
seed of the agent weights (entity_agent_params: numpy, so the CPU script plays the same weights).

Arms: ro4-static / ro4 (refil_ro4.inc, four envs per wave: the compile-time refil_8 shape / the runtime shape),
ro2/kc1 and ro2/kc2 (refil_rollout_kernel<1> / <2>, two envs per wave; entity input width 13 + U padded to 16 / 32).
ro2/kc3 (width 48) needs U > 19 and is not reachable from the entity env (U <= 16).

Seeds. The checker accepts a greedy pick that differs from the float64 oracle's argmax only at a near tie (top-two
masked Q within Q_TOL = 1e-4), and the GPU tests cap the accepted share at 1 % of the case's decisions (the greedy
picks with at least two available actions: a padded or dead agent has only the no-op and cannot tie) so that the escape
cannot hide a wrong kernel. That cap is a condition on the case, so a seed is kept only if the float64 oracle alone,
rolled out over the oracle env (B = 37, episode_limit 30, grid 20, the test-mode run of episode 0 and the train-mode
run of episode 1 at epsilon 0.525, as the GPU test runs them), sees at most 0.5 % of its decisions at such a gap. A
seed that misses 0.5 % is replaced, not tolerated. The share scripts/refil_near_ties.py counted is written beside
each case.
"""
import numpy as np

B, EPISODE_LIMIT, GRID = 37, 30, 20
T_ENV = 25000
EPS = max(0.05, 1.0 - 0.95 / 50000 * T_ENV)  # 0.525, the schedule's value at T_ENV

REFIL_8 = "TR AR HR AR TM AR HR AM"  # the refil_8 composition; the smaller plans are its first S slots
V1 = {"MLG_REFIL_ROLLOUT": "v1"}
GENERIC = {"MLG_REFIL_GENERIC": "1"}


def _codes(S):
    return " ".join(REFIL_8.split()[:S])


# (id, codes, min_agents, max_agents, env, arm, seed)                           oracle near-tie share (decisions)
REFIL_CASES = [
    ("s8-ro4-static", _codes(8), 3, 8, None, "ro4-static", 11),                 # 0.012 % (1 / 8053)
    ("s8-ro4", _codes(8), 3, 8, GENERIC, "ro4", 11),                            # 0.012 % (1 / 8053)
    ("s7-ro4", _codes(7), 3, 7, None, "ro4", 11),                               # 0.000 % (0 / 7431)
    ("s7-ro2", _codes(7), 3, 7, V1, "ro2/kc2", 11),                             # 0.000 % (0 / 7431)
    ("s5-ro4", _codes(5), 2, 5, None, "ro4", 11),                               # 0.000 % (0 / 5403)
    ("s5-ro2", _codes(5), 2, 5, V1, "ro2/kc2", 11),                             # 0.000 % (0 / 5403)
    ("s4-ro4", _codes(4), 4, 4, None, "ro4", 11),                               # 0.000 % (0 / 6054)
    ("s3-ro4", _codes(3), 1, 3, None, "ro4", 11),                               # 0.000 % (0 / 3130)
    ("s3-ro2", _codes(3), 1, 3, V1, "ro2/kc2", 11),                             # 0.000 % (0 / 3130)
    ("s2-ro4", _codes(2), 1, 2, None, "ro4", 11),                               # 0.081 % (2 / 2464)
    ("s1-ro2-kc1", _codes(1), 1, 1, None, "ro2/kc1", 11),                       # 0.000 % (0 / 1696)
]

ENV_VARS = ("MLG_REFIL_ROLLOUT", "MLG_REFIL_GENERIC")


def case(cid):
    return next(c for c in REFIL_CASES if c[0] == cid)


def plan(codes):
    """match_build_plan of a case: the policy team and the scripted team, the same unit slots each."""
    from maleague.envs.plans import team_from_codes
    return [team_from_codes(codes, False), team_from_codes(codes, True)]


def env_args(cid, seed=None):
    _, codes, kmin, kmax, _, _, s = case(cid)
    return {"match_build_plan": plan(codes), "grid_size": GRID, "stochastic_spawns": True,
            "episode_limit": EPISODE_LIMIT, "min_agents": kmin, "max_agents": kmax,
            "seed": s if seed is None else seed}


def spec_for(cid, seed=None):
    from maleague.envs.entity_env import EntityEnvSpec
    return EntityEnvSpec.from_env_args(env_args(cid, seed))


def refil_dims(spec):
    """The MlgRefilDims of the entity agent over ``spec`` (what agent.dims() returns), without building one."""
    from maleague import _native
    return _native.MlgRefilDims(n_agents=spec.n_agents, n_entities=spec.n_entities, entity_shape=8,
                                n_actions=spec.n_actions, entity_last_action=1, attn_embed_dim=64, attn_n_heads=4,
                                rnn_hidden_dim=64)


def entity_agent_params(d0, n_actions, seed, emb=64):
    """EntityAttentionRNNAgent parameters drawn with numpy (the same on every host and torch build) in torch's default
    ranges: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for the linear layers (in_trans has no bias) and
    U(-1 / sqrt(H), 1 / sqrt(H)) for the GRU cell. state_dict keys of the agent's parameters, float32 arrays."""
    rng = np.random.RandomState(seed)
    u = lambda bound, *shape: rng.uniform(-bound, bound, size=shape).astype(np.float32)  # noqa: E731
    k0, ke = 1.0 / np.sqrt(d0), 1.0 / np.sqrt(emb)
    return {"fc1.weight": u(k0, emb, d0), "fc1.bias": u(k0, emb),
            "attn.in_trans.weight": u(ke, 3 * emb, emb),
            "attn.out_trans.weight": u(ke, emb, emb), "attn.out_trans.bias": u(ke, emb),
            "fc2.weight": u(ke, emb, emb), "fc2.bias": u(ke, emb),
            "rnn.weight_ih": u(ke, 3 * emb, emb), "rnn.weight_hh": u(ke, 3 * emb, emb),
            "rnn.bias_ih": u(ke, 3 * emb), "rnn.bias_hh": u(ke, 3 * emb),
            "fc3.weight": u(ke, n_actions, emb), "fc3.bias": u(ke, n_actions)}
