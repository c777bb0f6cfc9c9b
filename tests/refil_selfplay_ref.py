"""Oracle of REFIL in self-play (DESIGN.md §3b'): the two-policy entity env, the canonical view of the away side
written in numpy straight from the spec, the float64 oracle's own self-play rollout (CPU; the seed selection of
tests/refil_selfplay_shapes.py and scripts/refil_selfplay_near_ties.py), one launch of mlg_refil_rollout_selfplay and
its teacher-forced check of both sides.

The env is envref.RefEnv with ``scripted = [False, False]`` (2S agents in unit order, ``step`` returns both teams'
rewards) plus RefEntityEnv's reset (envref_reset_entity: the same k for both teams) and entities (envref_entities).
The away batch is an ordinary entity batch from the away agent's point of view, so helpers.refil_oracle_q gives its
float64 Q unchanged.
"""
import numpy as np

import envref
from helpers import Q_TOL, entity_scheme_for, np_batch, refil_args, refil_oracle_q

SIDES = ("home", "away")


class SelfPlayEntityRefEnv(envref.RefEntityEnv):
    """The entity env with both teams policy-controlled: agents = units 0..2S-1, home first."""

    def __init__(self, roles, melees, kmin, kmax, grid=20, episode_limit=100, stochastic=True, seed=0, env_index=0):
        S = len(roles)
        envref.RefEnv.__init__(self, [0] * S + [1] * S, list(roles) * 2, list(melees) * 2, [False, False], grid=grid,
                               episode_limit=episode_limit, stochastic=stochastic, seed=seed, env_index=env_index)
        self.kmin, self.kmax = int(kmin), int(kmax)
        self.k = None
        self.grid = grid


def ref_envs_for(spec, B, seed):
    return [SelfPlayEntityRefEnv(spec.roles, spec.melees, spec.min_agents, spec.max_agents, grid=spec.grid,
                                 episode_limit=spec.episode_limit, stochastic=spec.stochastic, seed=seed, env_index=b)
            for b in range(B)]


# ---- the canonical view (§3b'), each map its own inverse ---------------------------------------------------------

def pow2(grid):
    p = 1
    while p < grid:
        p <<= 1
    return p


def view_index(S):
    """Unit of canonical entity j': (j' + S) mod U."""
    U = 2 * S
    return (np.arange(U) + S) % U


def view_entities(ent, om, em, S, grid):
    """(entities [U, 8], obs_mask [U, U], entity_mask [U]) of one view -> the other view."""
    idx, P = view_index(S), np.float32(pow2(grid))
    e = np.array(ent[idx], dtype=np.float32)
    alive = e[:, 0] == 1
    x = e[:, 1] * P  # exact: x / P with P a power of two
    e[:, 1] = np.where(alive, (np.float32(grid - 1) - x) / P, np.float32(0))
    e[:, 4] = np.where(alive, np.float32(1) - e[:, 4], np.float32(0))
    return e, np.array(om[idx][:, idx]), np.array(em[idx])


def view_avail(av, S):
    """avail rows [..., A] of one view -> the other view: 3 / 4 swapped, target 5 + j' = target 5 + (j' + S) mod U."""
    out = np.array(av)
    out[..., 3], out[..., 4] = av[..., 4], av[..., 3]
    out[..., 5:] = av[..., 5:][..., view_index(S)]
    return out


def view_actions(acts, S):
    """action indices of one view -> the other view."""
    a = np.asarray(acts).astype(np.int64)
    U = 2 * S
    out = a.copy()
    out[a == 3] = 4
    out[a == 4] = 3
    tg = a >= 5
    out[tg] = 5 + (a[tg] - 5 + S) % U
    return out


def side_views(r, S):
    """Per side (entities, obs_mask, entity_mask, avail [S, A]) of oracle env ``r``'s current state."""
    ent, om, em = r.entities()
    av = r.avail()
    return (ent, om, em, av[:S]), view_entities(ent, om, em, S, r.grid) + (view_avail(av[S:], S),)


# ---- weights -----------------------------------------------------------------------------------------------------

def side_params(d0, A, S, seed, attack_bias=0.0, move_bias=0.0, ally_bias=0.0, noop_bias=0.0):
    """refil_shapes.entity_agent_params with an optional push: fc3.bias of the enemy targets (view actions 5 + S ..
    5 + 2S - 1 on either side) += attack_bias, of "move +x" (action 3: towards the enemy in either view) += move_bias,
    of the ally targets (view actions 5 .. 5 + S - 1: a healer's) += ally_bias, of the no-op (action 0) += noop_bias.
    With such biases the oracle's own play ends battles (tests/refil_selfplay_shapes.py)."""
    import refil_shapes as FS
    p = FS.entity_agent_params(d0, A, seed)
    p["fc3.bias"] = p["fc3.bias"].copy()
    p["fc3.bias"][5 + S:] += np.float32(attack_bias)
    p["fc3.bias"][3] += np.float32(move_bias)
    p["fc3.bias"][5:5 + S] += np.float32(ally_bias)
    p["fc3.bias"][0] += np.float32(noop_bias)
    return p


def d0_of(A, la):
    return 8 + (A if la else 0)


def case_params(c):
    """(home, away) state_dict arrays of case ``c`` (refil_selfplay_shapes.Case)."""
    S = len(c.codes.split())
    A = 5 + 2 * S
    return (side_params(d0_of(A, c.la), A, S, c.seed_home, *c.bias_home),
            side_params(d0_of(A, c.la), A, S, c.seed_away, *c.bias_away))


# ---- the float64 oracle's own self-play (CPU) ----------------------------------------------------------------------

def oracle_selfplay(spec, params, la, B, seed, runs):
    """Both sides played by the float64 oracle agent over the oracle env, as the kernel would: ``runs`` = [(episode,
    eps_home, eps_away), ...]. Returns per side the decisions (greedy picks with >= 2 available actions), the near ties
    among them, greedy picks and epsilon draws, plus what the play did: away wins, home wins, away move / target
    actions executed, the k values seen."""
    import torch
    import refil_ref as RR
    S, U, A = spec.S, spec.U, spec.n_actions
    args = refil_args(n_agents=S, n_entities=U, n_actions=A, entity_last_action=la, device="cpu")
    P = [{k: torch.from_numpy(np.array(v)).double() for k, v in p.items()} for p in params]
    n = {s: dict(decisions=0, near_ties=0, greedy=0, epsilon_draws=0) for s in SIDES}
    out = dict(away_wins=0, home_wins=0, away_moves=0, away_targets=0, ks=set(), steps=0)
    for episode, eps_h, eps_a in runs:
        refs = ref_envs_for(spec, B, seed)
        for r in refs:
            r.episode = episode
            r.reset()
            out["ks"].add(int(r.k))
        h = [torch.zeros(B, S, 64, dtype=torch.float64) for _ in SIDES]
        last = [np.zeros((B, U, A)) for _ in SIDES]
        status = [0] * B
        t = 0
        while any(s < 2 for s in status):
            views = [side_views(r, S) for r in refs]
            acts = np.zeros((2, B, S), np.int64)
            for s, side in enumerate(SIDES):
                ent = np.stack([v[s][0] for v in views]).astype(np.float64)
                if la:
                    ent = np.concatenate([ent, last[s]], axis=2)
                om, em = np.stack([v[s][1] for v in views]), np.stack([v[s][2] for v in views])
                with torch.no_grad():
                    q, hs = RR.entity_agent(P[s], torch.from_numpy(ent)[:, None], torch.from_numpy(om)[:, None],
                                            torch.from_numpy(em)[:, None], h[s], args)
                h[s] = hs[:, 0]
                q = q[:, 0].numpy()
                eps = (eps_h, eps_a)[s]
                for b in range(B):
                    if status[b] == 2:
                        continue
                    key = envref.env_key(seed, b)
                    for k in range(S):
                        av, stream = views[b][s][3][k], s * S + k
                        if eps > 0 and envref.u01(envref.rng(key, envref.ctr(episode, t, 2, stream))) < np.float32(eps):
                            acts[s, b, k] = envref.random_available(av.tolist(),
                                                                    envref.rng(key, envref.ctr(episode, t, 3, stream)))
                            n[side]["epsilon_draws"] += 1
                            continue
                        m = np.where(av == 0, -np.inf, q[b, k])
                        srt = np.sort(m)
                        n[side]["greedy"] += 1
                        if np.isfinite(srt[-2]):
                            n[side]["decisions"] += 1
                            n[side]["near_ties"] += int(not srt[-1] - srt[-2] > Q_TOL)
                        acts[s, b, k] = int(np.argmax(m))
                last[s][:] = 0
                np.put_along_axis(last[s][:, :S], acts[s][:, :, None], 1.0, axis=2)
            for b, r in enumerate(refs):
                if status[b] == 0:
                    aw = acts[1, b]
                    out["away_moves"] += int(((aw >= 1) & (aw <= 4)).sum())
                    out["away_targets"] += int((aw >= 5).sum())
                    out["steps"] += 1
                    _, done, info = r.step(np.concatenate([acts[0, b], view_actions(aw, S)]))
                    status[b] = 1 if done else 0
                    if done:
                        out["home_wins"] += int(info["battle_won"][0])
                        out["away_wins"] += int(info["battle_won"][1])
                elif status[b] == 1:
                    status[b] = 2
            t += 1
    return n, out


# ---- one launch of mlg_refil_rollout_selfplay ------------------------------------------------------------------------

def sp_agent(device, params, S, la=True, seed=0):
    """An ImagineEntityAttentionRNNAgent of one side (S agents among 2S entities) with ``params`` loaded (None:
    torch-seeded)."""
    import torch
    from maleague.modules.agents import REGISTRY
    U, A = 2 * S, 5 + 2 * S
    a = refil_args(n_agents=S, n_entities=U, n_actions=A, entity_last_action=la, device=str(device))
    torch.manual_seed(seed)
    ag = REGISTRY["imagine_entity_attend_rnn"](d0_of(A, la), a).to(device)
    if params is not None:
        sd = ag.state_dict()
        sd.update({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
        ag.load_state_dict(sd)
    return ag, a


def side_info(spec):
    """env_info of ONE side's batches and MAC: S agents, all 2S entities."""
    info = dict(spec.env_info())
    info["n_agents"] = spec.S
    return info


def sp_rollout(device, spec, params, la=True, B=12, eps=(0.0, 0.0), test_mode=True, st=None, full_write=(False, False),
               batches=None, extents=(None, None), agents=None):
    """One mlg_refil_rollout_selfplay launch from env state ``st`` (fresh by default; a run advances its episode
    counters). full_write[s]: side s's batch is garbage-filled and written in full-write mode (extents[s]: its slot
    extents tensor). Returns (agents, args, host batches, summary, st, device batches)."""
    import torch
    from maleague import _native
    from maleague.components.batch_view import mlg_entity_batch
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.envs.teams_env import VecEnvState
    assert spec.self_play
    if agents is None:
        agents = [sp_agent(device, p, spec.S, la) for p in params]
    scheme, groups, pre = entity_scheme_for(side_info(spec), torch)
    if st is None:
        st = VecEnvState(spec, B, device)
    if batches is None:
        batches = []
        for s in range(2):
            bt = EpisodeBatch(scheme, groups, B, spec.episode_limit + 1, preprocess=pre, device=device)
            if full_write[s]:
                for v in bt.data.transition_data.values():
                    v.fill_(7)
            batches.append(bt)
    mbs, keep = [], []
    for s in range(2):
        mb, k = mlg_entity_batch(batches[s])
        keep.append(k)
        if full_write[s]:
            mb.full_write = 1
        if extents[s] is not None:
            mb.slot_extent = extents[s].data_ptr()
        mbs.append(mb)
    run = torch.zeros(6 * B, dtype=torch.int32, device=device)
    rows = torch.zeros(1, dtype=torch.int64, device=device)
    ri = _native.MlgRunInfo(run[0:B].data_ptr(), run[4 * B:5 * B].data_ptr(), run[B:3 * B].data_ptr(),
                            run[3 * B:4 * B].data_ptr(), rows.data_ptr(), run[5 * B:6 * B].data_ptr())
    d = agents[0][0].dims()
    _native.call("mlg_refil_rollout_selfplay", _native.byref(spec.to_c()), _native.byref(st.to_c()), _native.byref(d),
                 _native.ptr(agents[0][0].packed()), _native.ptr(agents[1][0].packed()), _native.byref(mbs[0]),
                 _native.byref(mbs[1]), _native.byref(ri), float(eps[0]), float(eps[1]), int(test_mode),
                 _native.stream_ptr())
    torch.cuda.synchronize()
    r = run.cpu().numpy()
    summ = {"len": r[0:B], "won": r[B:3 * B].reshape(B, 2), "draw": r[3 * B:4 * B],
            "ret": r[4 * B:5 * B].view(np.float32), "ret_away": r[5 * B:6 * B].view(np.float32),
            "agent_rows": rows.cpu().numpy()}
    return agents, [np_batch(b) for b in batches], summ, st, batches


def check_side_picks(side, s, S, nb, q, b, t, av, eps, test_mode, seed, episode, n):
    """The picks of side s's agents at (b, t): every epsilon draw the oracle's draw (stream = global agent index, the
    k-th available action in the side's own order), every other pick an argmax of the side's masked Q up to the
    near-tie rule of helpers.refil_teacher_check. Counts into n."""
    acts = nb["actions"][b, t, :, 0]
    key = envref.env_key(seed, b)
    for k in range(S):
        stream = s * S + k
        u = envref.u01(envref.rng(key, envref.ctr(episode, t, 2, stream)))
        if not test_mode and eps > 0 and u < np.float32(eps):
            want = envref.random_available(av[k], envref.rng(key, envref.ctr(episode, t, 3, stream)))
            assert acts[k] == want, (side, b, t, k, int(acts[k]), want)
            n["epsilon_draws"] += 1
            continue
        qm = np.where(av[k] != 0, q[t, k], -np.inf)
        srt = np.sort(qm)
        assert av[k, acts[k]] != 0 and qm[acts[k]] >= qm.max() - Q_TOL, (side, b, t, k)
        if srt[-1] - srt[-2] > Q_TOL:
            assert acts[k] == int(np.argmax(qm)), (side, b, t, k, int(acts[k]), int(np.argmax(qm)))
        else:
            n["near_ties"] += 1
        n["decisions"] += int(np.isfinite(srt[-2]))
        n["greedy"] += 1


def sp_teacher_check(spec, agents, nbs, summ, B, seed, eps, test_mode, episode=0, dtype=None, envs=None):
    """Replay both sides' recorded actions (the away side's through the raw image of the canonical index) through the
    oracle env at episode index ``episode``. Per side, bit-exact: entities, obs_mask, entity_mask, avail, one-hot rows,
    reward (home team 0's, away team 1's), terminated, filled; lengths, won / draw; returns within 1e-3; picks as
    check_side_picks. Returns the counts per side."""
    S, A, T = spec.S, spec.n_actions, spec.episode_limit
    envs = list(range(B)) if envs is None else [int(e) for e in envs]
    refs = ref_envs_for(spec, B, seed)
    q = [dict(zip(envs, refil_oracle_q(agents[s][0], agents[s][1], nbs[s], envs, dtype))) for s in range(2)]
    n = {side: dict(decisions=0, near_ties=0, greedy=0, epsilon_draws=0) for side in SIDES}
    for b in envs:
        r = refs[b]
        r.episode = episode
        r.reset()
        L = int(summ["len"][b])
        assert 1 <= L <= T
        ret = [np.float32(0), np.float32(0)]
        for t in range(L + 1):
            views = side_views(r, S)
            for s, side in enumerate(SIDES):
                nb, (ent, om, em, av) = nbs[s], views[s]
                np.testing.assert_array_equal(nb["entities"][b, t], ent, err_msg=f"{side} entities b={b} t={t}")
                np.testing.assert_array_equal(nb["obs_mask"][b, t], om, err_msg=f"{side} obs_mask b={b} t={t}")
                np.testing.assert_array_equal(nb["entity_mask"][b, t], em, err_msg=f"{side} entity_mask b={b} t={t}")
                np.testing.assert_array_equal(nb["avail_actions"][b, t], av, err_msg=f"{side} avail b={b} t={t}")
                assert nb["filled"][b, t, 0] == 1, (side, b, t)
                check_side_picks(side, s, S, nb, q[s][b], b, t, av, eps[s], test_mode, seed, r.cur_episode, n[side])
                oh = np.zeros((S, A), np.float32)
                oh[np.arange(S), nb["actions"][b, t, :, 0]] = 1
                np.testing.assert_array_equal(nb["actions_onehot"][b, t], oh, err_msg=f"{side} one-hot b={b} t={t}")
            if t < L:
                raw = np.concatenate([nbs[0]["actions"][b, t, :, 0], view_actions(nbs[1]["actions"][b, t, :, 0], S)])
                rew, done, info = r.step(raw)
                for s, side in enumerate(SIDES):
                    assert nbs[s]["reward"][b, t, 0] == np.float32(rew[s]), (side, "reward", b, t)
                    assert nbs[s]["terminated"][b, t, 0] == int(done), (side, "terminated", b, t)
                    ret[s] += np.float32(rew[s])
                assert done == (t == L - 1), (b, t, L)
        assert summ["won"][b, 0] == int(info["battle_won"][0]) and summ["won"][b, 1] == int(info["battle_won"][1]), b
        assert summ["draw"][b] == int(info["draw"]), b
        assert abs(summ["ret"][b] - ret[0]) <= 1e-3 and abs(summ["ret_away"][b] - ret[1]) <= 1e-3, b
        for nb in nbs:
            assert nb["filled"][b, L + 1:].sum() == 0 and nb["reward"][b, L:].sum() == 0, b
    for s, side in enumerate(SIDES):
        assert n[side]["greedy"] > 0 and (test_mode or eps[s] == 0 or n[side]["epsilon_draws"] > 0), side
    return n
