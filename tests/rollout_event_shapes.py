"""The eventful rollout cases shared by tests/test_rollout_event_shapes.py (CPU: the arms pinned through the describe
entry points, the conditions below re-counted for the small cases), tests/test_gpu_rollout_events.py (GPU: oracle parity
per dispatch arm where episodes end early) and scripts/rollout_event_counts.py (CPU: the counts written beside the
cases).

The per-arm suites (rollout_shapes.py, dqn_shapes.py, distinct_shapes.py and their self-play tables, coma_shapes.py)
play grid_size 20 with freshly drawn weights, where nearly every env runs to the episode limit and ends in a draw. Here
the same arms play inputs on which units die, teams win and envs of one workgroup end many steps apart, as
tests/mix_shapes.py does for the opponent mixture: grid_size 8, episode_limit 40, and on every policy's fc2.bias
BIAS_ATTACK = 2.0 on the attack actions ([5:]) and BIAS_MOVE = 0.7 on one move action (index 3 for the home / only
policy, 4 for the away policy: towards each other). The per-agent networks of a distinct pool get the same shifts each.
B = 37 (the third 16-env workgroup holds 5 envs), seed 11 (env keys, epsilon streams, weights). Where a case departs
from this recipe its row says so (``grid``, ``limit``, ``seed``). Three self-play cases play another seed: with seed 11
the home side wins no env (v1sp3-9v9: 0 / 30 wins) or a single one (ffsplds3-9v9: 1 / 25, v1sp4-13v13: 1 / 20), and a
GPU run may leave the oracle's trajectory at an accepted near tie, so a lone win is no safe condition; the first seed
from 12 on with at least two wins per side was taken. Every other case meets the conditions with the recipe as it is,
the 13v13 and 16v16 self-play arms included, so the table has no exception.

A case is kept only if the float64 oracle alone, rolled over the oracle env (the test-mode run of episode 0 and the
train-mode run of episode 1 at the family's epsilons), meets all of
  * near ties (top-two masked Q within Q_TOL) at most 0.5 % of the greedy picks (the GPU tests cap at 1 %),
  * at least MIN_EARLY = 8 envs of the 74 ending before the limit,
  * at least MIN_RAGGED = 2 ragged workgroups of the 6: 16-env groups in which one env ends at least 2 steps before
    another,
  * self-play: at least one win for each side,
  * policy-wins cases (a policy-heavy plan against few scripted units): at least MIN_WINS = 8 policy wins and at least
    one env that does not end in one.
The counts of scripts/rollout_event_counts.py stand beside each case:
  early-ending envs / ragged workgroups / wins of the home (policy) side / of the away (scripted) side / draws / unit
  deaths; near ties of greedy picks.
Policy (COMA) cases: the train-mode run is a multinomial draw and the test-mode run the masked greedy pick; near ties
there are the greedy run's picks whose top two masked probabilities lie within coma_shapes.DELTA.
"""
from collections import namedtuple

import numpy as np

B, SEED, GRID, EPISODE_LIMIT = 37, 11, 8, 40
T_ENV = 25000
EPS_HOME = max(0.05, 1.0 - 0.95 / 50000 * T_ENV)  # 0.525, the schedule's value at T_ENV
EPS_AWAY = 0.3
EPS_POLICY = 0.3
BIAS_ATTACK, BIAS_MOVE = 2.0, 0.7
GROUP_ENVS = 16
MIN_EARLY, MIN_RAGGED, MIN_WINS = 8, 2, 8
ORACLE_NEAR_TIE_CAP = 0.005
AWAY_SEED = {"drqn": 1000, "ff": 50, "dx": 50}  # the away weights' seed offset of the family's existing table
POLICY_SCALE = 16.0  # the factor on fc2.weight of tests/coma_shapes.py

# family: drqn / ff / dx (distinct) / policy; sp: both teams policy-controlled; flags: (obs_last_action, obs_agent_id);
# oracle: the counts of the float64 oracle alone (ORACLE_KEYS); env: the MLG_ROLLOUT_* variables the arm needs (the
# forced-global arms); wins: a policy-wins case
Case = namedtuple("Case", "id family sp H plan arm oracle flags env wins grid limit seed")
ORACLE_KEYS = ("early", "ragged", "home_wins", "away_wins", "draws", "deaths", "near_ties", "greedy")


def _c(cid, family, sp, H, plan, arm, oracle, flags=None, env=None, wins=False, grid=GRID, limit=EPISODE_LIMIT,
       seed=SEED):
    flags = flags if flags is not None else ((True, False) if family == "dx" else (True, True))
    oracle = dict(zip(ORACLE_KEYS, oracle))
    return Case(cid, family, sp, H, plan, arm, oracle, flags, env or {}, wins, grid, limit, seed)


_G = {"env": {"MLG_ROLLOUT_GLOBAL_WEIGHTS": "1"}}  # the forced-global arms of dqn_selfplay_shapes.LDS_VS_GLOBAL
_BARE = {"flags": (False, False)}


def _section(family, sp, rows):
    return [_c(r[0], family, sp, *r[1:5], **(r[5] if len(r) > 5 else {})) for r in rows]


# (id, H, plan, arm, oracle counts[, what departs from the defaults])                                near-tie share
# oracle counts: early-ending envs, ragged workgroups, home / policy wins, away / scripted wins, draws, unit deaths
# (-1: not counted for the policy family), near ties, greedy picks
CASES = _section("drqn", False, [
    ("ev-v7-4v4", 64, "4v4", "v7", (64, 6, 0, 65, 9, 317, 0, 6685)),  # 0.000 %
    ("ev-v7static-5v5", 64, "medium_1h_4t", "v7-static", (55, 6, 1, 57, 16, 411, 6, 10154)),  # 0.059 %
    ("ev-v2-5v7", 64, "5v7", "v2", (74, 6, 0, 74, 0, 388, 2, 5864)),  # 0.034 %
    ("ev-v1lds1-7v7", 64, "7v7", "v1-lds/tpw1", (58, 6, 0, 58, 16, 558, 5, 12535)),  # 0.040 %
    ("ev-v1lds2-9v9", 32, "9v9", "v1-lds/tpw2", (70, 6, 0, 70, 4, 761, 2, 15371)),  # 0.013 %
    ("ev-v1lds3-17v17", 32, "17v17", "v1-lds/tpw3", (68, 6, 0, 71, 3, 1422, 9, 30923)),  # 0.029 %
    ("ev-v1lds4-large", 32, "large", "v1-lds/tpw4", (40, 4, 0, 41, 33, 2423, 32, 53789)),  # 0.059 %
    ("ev-v1glb1-3v3", 128, "small", "v1-global/tpw1", (65, 6, 3, 62, 9, 274, 3, 5447)),  # 0.055 %
    ("ev-v1glb2-9v9", 64, "9v9", "v1-global/tpw2", (72, 6, 0, 73, 1, 742, 8, 15058)),  # 0.053 %
    ("ev-v1glb3-17v17", 64, "17v17", "v1-global/tpw3", (68, 6, 0, 68, 6, 1430, 16, 31116)),  # 0.051 %
    ("ev-v1glb4-large", 64, "large", "v1-global/tpw4", (40, 5, 0, 46, 28, 2463, 25, 53124)),  # 0.047 %
    ("win-v7-2s5p", 64, "2s5p", "v7", (62, 6, 63, 0, 11, 231, 2, 6899), {"wins": True}),  # 0.029 %
    ("win-v1-8p3s", 128, "8p3s", "v1-global/tpw1", (65, 6, 65, 0, 9, 309, 0, 8226), {"wins": True}),  # 0.000 %
]) + _section("drqn", True, [
    ("ev-sp8-3v3", 64, "small", "sp8", (25, 6, 7, 18, 49, 228, 4, 13245)),  # 0.030 %
    ("ev-sp7-4v4", 64, "4v4", "sp7", (10, 5, 3, 7, 64, 238, 2, 18480)),  # 0.011 %
    ("ev-sp2-5v5", 32, "medium_1h_4t", "sp2", (13, 5, 3, 10, 61, 388, 12, 23440)),  # 0.051 %
    ("ev-v1sp1-3v3", 128, "small", "v1-global/tpw1", (22, 5, 10, 11, 53, 230, 0, 13387)),  # 0.000 %
    ("ev-v1sp2-7v7", 64, "7v7", "v1-global/tpw2", (12, 5, 3, 9, 62, 588, 6, 32665)),  # 0.018 %
    ("ev-v1sp3-9v9", 64, "9v9", "v1-global/tpw3", (17, 6, 8, 11, 55, 761, 14, 41426), {"seed": 12}),  # 0.034 %
    ("ev-v1sp4-13v13", 32, "13v13", "v1-global/tpw4", (26, 6, 4, 23, 47, 1258, 30, 59651), {"seed": 12}),  # 0.050 %
]) + _section("ff", False, [
    ("ev-fflds1-3v3", 64, "small", "ff-lds/tpw1", (70, 6, 0, 71, 3, 272, 1, 5213)),  # 0.019 %
    ("ev-fflds2-9v9", 64, "9v9", "ff-lds/tpw2", (74, 6, 0, 74, 0, 734, 8, 15141)),  # 0.053 %
    ("ev-fflds3-17v17", 32, "17v17", "ff-lds/tpw3", (64, 6, 0, 68, 6, 1377, 6, 31197)),  # 0.019 %
    ("ev-fflds4-25v25", 32, "25v25", "ff-lds/tpw4", (69, 6, 0, 69, 5, 2020, 3, 46071)),  # 0.007 %
    ("ev-ffglb2-14v14", 128, "14v14", "ff-global/tpw2", (73, 6, 0, 73, 1, 1171, 2, 23626)),  # 0.008 %
    ("ev-ffglb3-17v17", 128, "17v17", "ff-global/tpw3", (74, 6, 0, 74, 0, 1366, 11, 29663)),  # 0.037 %
    ("ev-ffglb4-25v25", 64, "25v25", "ff-global/tpw4", (65, 6, 0, 69, 5, 2082, 18, 47841)),  # 0.038 %
    ("win-ff-7p2s", 64, "7p2s", "ff-lds/tpw1", (73, 6, 73, 0, 1, 228, 0, 5975), {"wins": True}),  # 0.000 %
]) + _section("ff", True, [
    ("ev-ffsplds1-3v3", 64, "small", "ffsp-lds/tpw1", (20, 6, 5, 15, 54, 213, 4, 13620)),  # 0.029 %
    ("ev-ffsplds2-5v5", 64, "medium_1h_4t", "ffsp-lds/tpw2", (10, 5, 6, 7, 61, 359, 5, 23465)),  # 0.021 %
    ("ev-ffsplds3-9v9", 64, "9v9", "ffsp-lds/tpw3", (21, 6, 10, 11, 53, 823, 11, 40640), {"seed": 13}),  # 0.027 %
    ("ev-ffsplds4-16v16", 32, "16v16", "ffsp-lds/tpw4", (24, 5, 15, 9, 50, 1602, 25, 72459)),  # 0.035 %
    ("ev-ffspglb3-9v9", 128, "9v9", "ffsp-global/tpw3", (23, 5, 5, 19, 50, 785, 13, 41733)),  # 0.031 %
    ("ev-ffspglb4-13v13", 128, "13v13", "ffsp-global/tpw4", (27, 5, 2, 25, 47, 1236, 16, 59408)),  # 0.027 %
    ("ev-ffspglb1-3v3-forced", 64, "small", "ffsp-global/tpw1", (20, 6, 5, 15, 54, 213, 4, 13620), _G),  # 0.029 %
    ("ev-ffspglb2-5v5-forced", 64, "medium_1h_4t", "ffsp-global/tpw2", (10, 5, 6, 7, 61, 359, 5, 23465), _G),  # 0.021 %
]) + _section("dx", False, [
    ("ev-dx1-3v3", 64, "small", "dx-global/tpw1", (69, 6, 3, 65, 6, 260, 0, 5144)),  # 0.000 %
    ("ev-dx2-9v9", 64, "9v9", "dx-global/tpw2", (70, 6, 0, 71, 3, 715, 5, 15017)),  # 0.033 %
    ("ev-dx3-17v17", 32, "17v17", "dx-global/tpw3", (72, 6, 0, 72, 2, 1370, 5, 30131)),  # 0.017 %
    ("ev-dx4-25v25", 64, "25v25", "dx-global/tpw4", (74, 6, 0, 74, 0, 2000, 12, 45653)),  # 0.026 %
    ("win-dx-2s6p", 64, "2s6p", "dx-global/tpw1", (68, 6, 69, 0, 5, 253, 2, 7558), {"wins": True}),  # 0.026 %
]) + _section("dx", True, [
    ("ev-dxsp1-3v3", 64, "small", "dxsp-global/tpw1", (18, 6, 8, 10, 56, 209, 2, 13345)),  # 0.015 %
    ("ev-dxsp2-5v5-nola", 64, "medium_1h_4t", "dxsp-global/tpw2", (18, 6, 8, 12, 54, 395, 7, 23373), _BARE),  # 0.030 %
    ("ev-dxsp3-9v9", 64, "9v9", "dxsp-global/tpw3", (24, 5, 5, 21, 48, 807, 9, 40858)),  # 0.022 %
    ("ev-dxsp4-16v16", 32, "16v16", "dxsp-global/tpw4", (26, 5, 7, 19, 48, 1572, 25, 73505)),  # 0.034 %
]) + _section("policy", False, [
    ("ev-pol-lds1-3v3", 32, "small", "policy-lds/tpw1", (69, 6, 0, 69, 5, -1, 1, 3600)),  # 0.028 %
    ("ev-pol-glb2-9v9", 64, "9v9", "policy-global/tpw2", (73, 6, 0, 73, 1, -1, 0, 10620)),  # 0.000 %
    ("ev-pol-lds3-17v17", 32, "17v17", "policy-lds/tpw3", (72, 6, 0, 72, 2, -1, 4, 20757)),  # 0.019 %
    ("ev-pol-glb4-large", 64, "large", "policy-global/tpw4", (44, 5, 0, 45, 29, -1, 30, 37550)),  # 0.080 %
    ("win-pol-7p2s", 64, "7p2s", "policy-lds/tpw1", (64, 6, 64, 0, 10, -1, 1, 5817), {"wins": True}),  # 0.017 %
])
IDS = [c.id for c in CASES]
# the CPU test re-counts these (at most 5 units per side)
CHEAP_IDS = [c.id for c in CASES if c.plan in ("small", "4v4", "medium_1h_4t", "2s5p")]


def case(cid):
    return next(c for c in CASES if c.id == cid)


def ids(family=None, sp=None, wins=None):
    return [c.id for c in CASES if (family is None or c.family == family) and (sp is None or c.sp == sp)
            and (wins is None or c.wins == wins)]


def env_args(c):
    from helpers import shape_plan
    return {"match_build_plan": shape_plan(c.plan, self_play=c.sp), "grid_size": c.grid, "stochastic_spawns": True,
            "episode_limit": c.limit, "seed": c.seed}


def spec_of(c):
    from maleague.envs.teams_env import TeamsEnvSpec
    return TeamsEnvSpec.from_env_args(env_args(c))


def dims_of(c, spec):
    from maleague import _native
    N, A = spec.n_agents // (2 if c.sp else 1), spec.n_actions
    la, ai = c.flags
    return _native.MlgAgentDims(d_obs=8 * spec.U, n_actions=A, n_agents=N, hidden=c.H,
                                d_in=8 * spec.U + (A if la else 0) + (N if ai else 0), obs_last_action=int(la),
                                obs_agent_id=int(ai))


def describe(c):
    """(arm, dynamic LDS bytes) of the case under the current environment, through its family's host-only query."""
    from maleague import _native
    spec = spec_of(c)
    d = dims_of(c, spec)
    if c.family == "drqn":
        return _native.rollout_describe(spec.to_c(), d, c.sp)
    fn = {("ff", False): _native.rollout_ff_describe, ("ff", True): _native.rollout_selfplay_ff_describe,
          ("dx", False): _native.rollout_distinct_describe, ("dx", True): _native.rollout_selfplay_distinct_describe,
          ("policy", False): _native.rollout_policy_describe}[(c.family, c.sp)]
    return fn(spec.to_c(), d)


def shifted(p, side):
    """``p`` with the bias shifts of the recipe: the attack actions, and the move action of ``side`` (0 home, 1
    away)."""
    p = dict(p)
    b = p["fc2.bias"].copy()
    b[5:] += np.float32(BIAS_ATTACK)
    b[3 + side] += np.float32(BIAS_MOVE)
    p["fc2.bias"] = b
    return p


def side_params(c, d_in, n_agents, n_actions):
    """Per side (one, or home and away) the case's weights as state_dict arrays: one dict (drqn, ff, policy: before the
    fc2 scale) or the list of the n_agents per-agent dicts (dx), drawn as the family's existing table draws them."""
    import distinct_ref as DR
    import dqn_ref as DQ
    import rollout_shapes as RS
    out = []
    for s in range(2 if c.sp else 1):
        seed = c.seed + s * AWAY_SEED.get(c.family, 0)
        if c.family == "dx":
            out.append([shifted(p, s) for p in DR.all_agent_params(n_agents, d_in, c.H, n_actions, seed)])
        elif c.family == "ff":
            out.append(shifted(DQ.agent_params(d_in, c.H, n_actions, seed), s))
        else:
            out.append(shifted(RS.agent_params(d_in, c.H, n_actions, seed), s))
    return out


def events(ep_lens, wons, limit):
    """The event counts of a case's runs. ep_lens: per run the [B] episode lengths; wons: per run the [B, 2]
    battle_won flags (home / policy side, away / scripted side). A workgroup is 16 consecutive envs; it is ragged if
    one of its envs ends at least 2 steps before another."""
    early = ragged = 0
    for L in ep_lens:
        L = np.asarray(L).astype(np.int64)
        early += int((L < limit).sum())
        for g in range(0, len(L), GROUP_ENVS):
            ragged += int(L[g:g + GROUP_ENVS].max() - L[g:g + GROUP_ENVS].min() >= 2)
    won = np.concatenate([np.asarray(w).reshape(-1, 2) for w in wons]) != 0
    return {"early": early, "ragged": ragged, "home_wins": int(won[:, 0].sum()), "away_wins": int(won[:, 1].sum()),
            "draws": int((~won.any(axis=1)).sum())}


def conditions(c, n, early_floor=MIN_EARLY, ragged_floor=MIN_RAGGED):
    """The conditions of the module docstring on the counts ``n`` (events() plus picks and near ties, where counted),
    as a list of the violated ones."""
    bad = []
    if "greedy" in n and n["near_ties"] > ORACLE_NEAR_TIE_CAP * n["greedy"]:
        bad.append("near ties above 0.5 %")
    if n["early"] < early_floor:
        bad.append(f"early {n['early']} < {early_floor}")
    if n["ragged"] < ragged_floor:
        bad.append(f"ragged {n['ragged']} < {ragged_floor}")
    if c.sp and not (n["home_wins"] >= 1 and n["away_wins"] >= 1):
        bad.append("a side never wins")
    if c.wins and n["home_wins"] < MIN_WINS:
        bad.append(f"policy wins {n['home_wins']} < {MIN_WINS}")
    if c.wins and n["home_wins"] >= n["envs"]:
        bad.append("every env ends in a policy win")
    return bad


def _forward(c, spec, params):
    """-> (state0, step): step(state, x [B, sides * N, d_in]) -> (Q [B, sides * N, A] as numpy, state), float64."""
    import torch
    import dqn_ref as DQ
    import learner_ref as LR
    sides = 2 if c.sp else 1
    N = spec.n_agents // sides
    if c.family == "dx":
        nets = [{k: torch.from_numpy(v).double() for k, v in p.items()} for ps in params for p in ps]
    else:
        nets = [{k: torch.from_numpy(v).double() for k, v in p.items()} for p in params]

    def step(h, x):
        Bn = x.shape[0]
        qs = []
        with torch.no_grad():
            if c.family == "dx":  # network i of side s for agent slot s * N + i
                h = h if h is not None else [torch.zeros(Bn, c.H, dtype=torch.float64) for _ in nets]
                for i, p in enumerate(nets):
                    q, h[i] = LR.drqn_forward(p, x[:, i], h[i])
                    qs.append(q[:, None])
            elif c.family == "ff":
                qs = [DQ.dqn_forward(p, x[:, s * N:(s + 1) * N]) for s, p in enumerate(nets)]
            else:
                h = h if h is not None else [torch.zeros(Bn * N, c.H, dtype=torch.float64) for _ in nets]
                for s, p in enumerate(nets):
                    q, h[s] = LR.drqn_forward(p, x[:, s * N:(s + 1) * N].reshape(Bn * N, -1), h[s])
                    qs.append(q.reshape(Bn, N, -1))
        return torch.cat(qs, dim=1).numpy(), h

    return step


def oracle_counts(c, n_envs=B):
    """The float64 oracle alone over both runs of a case -> the counts: greedy picks, near ties, epsilon draws (policy
    cases: picks and near ties of the greedy run), events(), unit deaths, envs."""
    if c.family == "policy":
        return _oracle_policy_counts(c, n_envs)
    import torch
    import envref
    from helpers import Q_TOL, ref_envs_for
    spec = spec_of(c)
    sides = 2 if c.sp else 1
    NT, A = spec.n_agents, spec.n_actions
    N = NT // sides
    la, ai = c.flags
    d_in = 8 * spec.U + (A if la else 0) + (N if ai else 0)
    step = _forward(c, spec, side_params(c, d_in, N, A))
    ids_ = torch.eye(N, dtype=torch.float64).repeat(sides, 1).unsqueeze(0).expand(n_envs, NT, N)
    picks = ties = draws = deaths = 0
    ep_lens, wons = [], []
    for episode, eps in ((0, (0.0, 0.0)), (1, (EPS_HOME, EPS_AWAY if c.sp else EPS_HOME))):
        refs = ref_envs_for(spec, n_envs, seed=c.seed)
        for r in refs:
            r.episode = episode
            r.reset()
        h = None
        last = np.zeros((n_envs, NT, A))
        status = [0] * n_envs  # 0 running, 1 terminated (one more pick is recorded), 2 finished
        L, won = np.zeros(n_envs, np.int64), np.zeros((n_envs, 2), np.int64)
        t = 0
        while any(s < 2 for s in status):
            obs = torch.from_numpy(np.stack([r.obs() for r in refs]).astype(np.float64))
            avail = np.stack([r.avail() for r in refs])
            x = torch.cat([obs] + ([torch.from_numpy(last)] if la else []) + ([ids_] if ai else []), dim=2)
            q, h = step(h, x)
            acts = np.zeros((n_envs, NT), np.int64)
            for b in range(n_envs):
                if status[b] == 2:
                    continue
                key = envref.env_key(c.seed, b)
                for n in range(NT):
                    av, e = avail[b, n], eps[n >= N]
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
                    _, done, info = r.step(acts[b])
                    if done:
                        L[b], won[b], status[b] = t + 1, info["battle_won"], 1
                        deaths += int((r.hp <= 0).sum())
                elif status[b] == 1:
                    status[b] = 2
            t += 1
        ep_lens.append(L)
        wons.append(won)
    return dict(events(ep_lens, wons, c.limit), greedy=picks, near_ties=ties, epsilon_draws=draws, deaths=deaths,
                envs=2 * n_envs)


def policy_agent_params(c):
    """(d_in, H, n_actions) -> the policy case's state_dict arrays before the fc2 scale."""
    return lambda d_in, hidden, n_actions: side_params(c, d_in, None, n_actions)[0]


def _oracle_policy_counts(c, n_envs):
    import coma_shapes as CS
    spec = spec_of(c)
    ep_lens, wons, greedy = [], [], None
    for episode, mode in ((0, "greedy"), (1, "train")):
        infos = {}
        _, L, picks, near = CS.oracle_policy_run(spec, c.H, c.seed, POLICY_SCALE, True, episode, mode, n_envs=n_envs,
                                                 eps=EPS_POLICY, agent_params=policy_agent_params(c), infos=infos)
        ep_lens.append(L)
        wons.append(np.array([infos[e]["battle_won"] for e in range(n_envs)], np.int64))
        if mode == "greedy":
            greedy = (picks, near)
    return dict(events(ep_lens, wons, c.limit), greedy=greedy[0], near_ties=greedy[1], epsilon_draws=0, deaths=-1,
                envs=2 * n_envs)


def count_line(c, n):
    share = 100.0 * n["near_ties"] / max(n["greedy"], 1)
    return (f"{c.id:24s} {c.arm:18s} grid {c.grid} limit {c.limit} seed {c.seed}: early {n['early']} ragged "
            f"{n['ragged']} wins {n['home_wins']} / {n['away_wins']} draws {n['draws']} deaths {n['deaths']}; near "
            f"ties {n['near_ties']} of {n['greedy']} = {share:.3f} %")
