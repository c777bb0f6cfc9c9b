"""Shared test helpers (args namespaces, spec <-> oracle env construction)."""
from types import SimpleNamespace

import numpy as np


def qmix_args(**kw):
    """Default + qmix.yaml + ma.yaml values that matter on the hot path (src/config/*.yaml)."""
    a = dict(n_agents=5, n_actions=15, state_shape=60, rnn_hidden_dim=64, obs_last_action=True, obs_agent_id=True,
             agent="rnn", agent_output_type="q", action_selector="epsilon_greedy", epsilon_start=1.0,
             epsilon_finish=0.05, epsilon_anneal_time=50000, freeze_native=False, device="cuda", mixer="qmix",
             mixing_embed_dim=32, hypernet_layers=2, hypernet_embed=64, double_q=True, gamma=0.99, lr=0.0005,
             optim_alpha=0.99, optim_eps=1e-5, grad_norm_clip=10, target_update_interval=200,
             learner_log_interval=0, batch_size_run=8, batch_size=32, buffer_size=64, seed=0,
             env_args={"match_build_plan": "medium_1h_4t", "grid_size": 20, "stochastic_spawns": True,
                       "episode_limit": 100})
    a.update(kw)
    return SimpleNamespace(**a)


def ref_envs_for(spec, B, seed=0):
    """oracle RefEnv instances matching a product TeamsEnvSpec (same unit tables, keys seed*2^32 + b)."""
    import envref
    return [envref.RefEnv(spec.team, spec.role, spec.melee, spec.scripted, grid=spec.grid,
                          episode_limit=spec.episode_limit, stochastic=spec.stochastic, seed=seed, env_index=b)
            for b in range(B)]


def scheme_for(env_info, torch):
    from maleague.components.transforms import OneHot
    scheme = {
        "state": {"vshape": env_info["state_shape"]},
        "obs": {"vshape": env_info["obs_shape"], "group": "agents"},
        "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
        "avail_actions": {"vshape": (env_info["n_actions"],), "group": "agents", "dtype": torch.int},
        "reward": {"vshape": (1,)},
        "terminated": {"vshape": (1,), "dtype": torch.uint8},
    }
    groups = {"agents": env_info["n_agents"]}
    preprocess = {"actions": ("actions_onehot", [OneHot(out_dim=env_info["n_actions"])])}
    return scheme, groups, preprocess


def np_batch(batch):
    return {k: v.detach().cpu().numpy() for k, v in batch.data.transition_data.items()}


def batch_mask_sum(filled, terminated):
    """The learners' mask sum (reference q_learner.py:58-60, 89-95 after ma_experiment.py:235-239's truncation):
    mask(b, t) = filled(b, t) * (1 - terminated(b, t - 1)) summed over t < max_t_filled - 1, as float32."""
    f = np.asarray(filled).reshape(len(filled), -1).astype(np.float32)
    term = np.asarray(terminated).reshape(len(terminated), -1).astype(np.float32)
    te = int(np.clip(f.sum(axis=1).max(), 2, f.shape[1]))
    mask = f.copy()
    mask[:, 1:] *= 1.0 - term[:, :-1]
    return np.float32(mask[:, :te - 1].sum())


def refil_args(**kw):
    """REFIL (config 5) args: entity scheme + imagine agent + flex_qmix (REFIL defaults)."""
    a = dict(n_agents=8, n_entities=16, n_actions=21, entity_shape=8, entity_last_action=True, attn_embed_dim=64,
             attn_n_heads=4, rnn_hidden_dim=64, hypernet_embed=64, mixing_embed_dim=32, pooling_type=None,
             softmax_mixing_weights=False, mixer="flex_qmix", entity_scheme=True, agent="imagine_entity_attend_rnn",
             mac="entity", learner="refil", agent_output_type="q", action_selector="epsilon_greedy",
             epsilon_start=1.0, epsilon_finish=0.05, epsilon_anneal_time=50000, double_q=True, gamma=0.99, lr=5e-4,
             optim_alpha=0.99, optim_eps=1e-5, weight_decay=0, grad_norm_clip=10, target_update_interval=200,
             learner_log_interval=0, lmbda=0.5, device="cuda", freeze_native=False, obs_last_action=False,
             obs_agent_id=False, batch_size_run=8, batch_size=32, buffer_size=64, seed=0, runner="parallel",
             env_args={"match_build_plan": "refil_8", "grid_size": 20, "stochastic_spawns": True,
                       "episode_limit": 100, "min_agents": 3, "max_agents": 8})
    a.update(kw)
    return SimpleNamespace(**a)


def entity_scheme_for(env_info, torch):
    from maleague.components.transforms import OneHot
    NE, ED, A = env_info["n_entities"], env_info["entity_shape"], env_info["n_actions"]
    scheme = {
        "entities": {"vshape": (NE, ED)},
        "obs_mask": {"vshape": (NE, NE), "dtype": torch.uint8},
        "entity_mask": {"vshape": (NE,), "dtype": torch.uint8},
        "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
        "avail_actions": {"vshape": (A,), "group": "agents", "dtype": torch.int},
        "reward": {"vshape": (1,)},
        "terminated": {"vshape": (1,), "dtype": torch.uint8},
    }
    groups = {"agents": env_info["n_agents"]}
    preprocess = {"actions": ("actions_onehot", [OneHot(out_dim=A)])}
    return scheme, groups, preprocess


def ref_entity_envs_for(spec, B, seed=0):
    import envref
    return [envref.RefEntityEnv(spec.roles, spec.melees, spec.min_agents, spec.max_agents, grid=spec.grid,
                                episode_limit=spec.episode_limit, stochastic=spec.stochastic, seed=seed, env_index=b)
            for b in range(B)]


_UNIT_CYCLE = ("TR", "AR", "HR", "TM")


def shape_plan(name, self_play=False):
    """match_build_plan for the rollout shape tests: a built-in plan name, or "KvK" (K units per side, unit k of a
    side is TR AR HR TM cyclically, scripted team first), "5v7" (5 policy agents against 7 scripted units, scripted
    team first) or "3v5" (3 policy agents listed first, team 0, against 5 scripted units). self_play: both teams
    policy-controlled (symmetric plans only). Policy-heavy plans name both teams in the order they are listed, a count
    and "p" (policy) or "s" (scripted) each: "7p2s" is 7 policy units listed first (team 0) against 2 scripted units,
    "2s7p" the same teams with the scripted one listed first."""
    import re
    from maleague.envs.plans import available, builtin_plan, team_from_codes
    if name in available():
        return builtin_plan(name, self_play=True) if self_play else name
    codes = lambda k: " ".join(_UNIT_CYCLE[i % 4] for i in range(k))  # noqa: E731
    heavy = re.fullmatch(r"(\d+)([ps])(\d+)([ps])", name)
    if heavy:
        (k0, c0), (k1, c1) = heavy.group(1, 2), heavy.group(3, 4)
        assert not self_play and {c0, c1} == {"p", "s"}, name
        policy, scripted = (int(k0), int(k1)) if c0 == "p" else (int(k1), int(k0))
        assert policy > scripted > 0, name
        return [team_from_codes(codes(int(k0)), c0 == "s"), team_from_codes(codes(int(k1)), c1 == "s")]
    if name == "5v7":
        assert not self_play
        return [team_from_codes(codes(7), True), team_from_codes(codes(5), False)]
    if name == "3v5":
        assert not self_play
        return [team_from_codes(codes(3), False), team_from_codes(codes(5), True)]
    k, k2 = (int(x) for x in name.split("v"))
    assert k == k2, name
    return [team_from_codes(codes(k), not self_play), team_from_codes(codes(k), False)]


def drqn_dims(spec, hidden, self_play=False):
    """The MlgAgentDims of a BasicMAC's DRQN agent (obs_last_action and obs_agent_id on) over the env ``spec``: what
    agent.dims() returns on a built stepper, without building one."""
    from maleague import _native
    N = spec.n_agents // 2 if self_play else spec.n_agents
    return _native.MlgAgentDims(d_obs=8 * spec.U, n_actions=spec.n_actions, n_agents=N, hidden=hidden,
                                d_in=8 * spec.U + spec.n_actions + N, obs_last_action=1, obs_agent_id=1)


Q_TOL = 1e-4  # the project's bar for Q values and hidden states (fp32 kernels vs the oracle)


def build_stepper(device, plan="medium_1h_4t", B=48, episode_limit=40, seed=5, grid_size=20, **kw):
    """A ParallelStepper over ``plan`` (a built-in name or a list of two team dicts) with a freshly seeded BasicMAC."""
    import torch
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import ParallelStepper
    args = qmix_args(batch_size_run=B, seed=seed, env_args={"match_build_plan": plan, "grid_size": grid_size,
                                                            "stochastic_spawns": True, "episode_limit": episode_limit},
                     **kw)
    stepper = ParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"], info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(info, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    torch.manual_seed(seed)
    mac = BasicMAC(proto.scheme, groups, args)
    stepper.initialize(scheme, groups, preprocess, mac)
    return stepper, mac, args


def oracle_q(mac, tb, N, T, dtype=None):
    """The oracle DRQN's Q [B, T, N, A] along a recorded batch (LR.mac_unroll) with ``mac``'s parameters: fp32 by
    default, or params, inputs and h0 cast to ``dtype`` (torch.float64: strictly more precise than the kernels)."""
    import torch
    import learner_ref as LR
    params = {k: v.detach().cpu() for k, v in mac.agent.state_dict().items()}
    h0 = None
    if dtype is not None:
        params = {k: v.to(dtype) for k, v in params.items()}
        tb = {k: tb[k].to(dtype) for k in ("obs", "actions_onehot")}
        h0 = torch.zeros(tb["obs"].shape[0] * N, params["gru.weight_hh"].shape[1], dtype=dtype)
    with torch.no_grad():
        q, _ = LR.mac_unroll(params, tb, N, T=T, h0=h0)
    return q.numpy()


def check_run(stepper, mac, args, batch, infos, episode, test_mode, eps, envs=None, dtype=None, nb=None):
    """Teacher-forced env replay + oracle agent check of a run; ``envs``: the env indices to check (all by
    default; a subset for the 4096-env headline shape). ``dtype``: the oracle unroll's precision (oracle_q).
    ``nb``: the recorded batch as host arrays when it is not ``batch``'s own copy. Returns the counts (greedy picks
    checked, near ties among them, epsilon draws)."""
    import envref
    import torch
    spec = stepper.spec
    B, N, A, T1 = stepper.batch_size, spec.n_agents, spec.n_actions, stepper.episode_limit + 1
    sub = list(range(B)) if envs is None else [int(e) for e in envs]
    nb = np_batch(batch) if nb is None else nb
    ep_len = stepper.last_run["ep_len"].numpy()
    rets = stepper.last_run["returns"].numpy()
    assert (ep_len >= 1).all() and (ep_len <= stepper.episode_limit).all()
    assert stepper.t == ep_len.max()
    # --- env side, teacher forced: replay the recorded actions through the C oracle ---
    refs = ref_envs_for(spec, B, seed=args.seed)
    assert len(infos) == B
    # infos come in termination order: by episode length, then env index
    place = np.empty(B, np.int64)
    place[np.lexsort((np.arange(B), ep_len))] = np.arange(B)
    for b in sub:
        r = refs[b]
        r.episode = episode
        r.reset()
        L = int(ep_len[b])
        np.testing.assert_array_equal(nb["obs"][b, 0], r.obs())
        np.testing.assert_array_equal(nb["state"][b, 0], r.state())
        np.testing.assert_array_equal(nb["avail_actions"][b, 0], r.avail())
        ret = 0.0
        for t in range(L):
            rew, done, info = r.step(nb["actions"][b, t, :, 0])
            ret += rew[0]
            assert nb["reward"][b, t, 0] == np.float32(rew[0]), ("reward", b, t)
            assert nb["terminated"][b, t, 0] == int(done) and done == (t == L - 1), ("terminated", b, t, L)
            np.testing.assert_array_equal(nb["obs"][b, t + 1], r.obs(), err_msg=f"obs env {b} t {t + 1}")
            np.testing.assert_array_equal(nb["state"][b, t + 1], r.state(), err_msg=f"state env {b} t {t + 1}")
            np.testing.assert_array_equal(nb["avail_actions"][b, t + 1], r.avail(),
                                          err_msg=f"avail_actions env {b} t {t + 1}")
        assert rets[b] == np.float32(ret), ("returns", b)
        np.testing.assert_array_equal(nb["filled"][b, :, 0], (np.arange(T1) <= L).astype(np.int64),
                                      err_msg=f"filled env {b}")
        # actions recorded for t = 0..L (the final one after termination), zero beyond
        assert (nb["actions"][b, L + 1:] == 0).all() and (nb["actions_onehot"][b, L + 1:] == 0).all()
        oh = np.zeros((L + 1, N, A), np.float32)
        oh[np.arange(L + 1)[:, None], np.arange(N)[None, :], nb["actions"][b, :L + 1, :, 0]] = 1
        np.testing.assert_array_equal(nb["actions_onehot"][b, :L + 1], oh)
        assert (nb["reward"][b, L:] == 0).all() and (nb["terminated"][b, L:] == 0).all()
        assert infos[int(place[b])] == info, (b, L, infos[int(place[b])], info)  # the oracle's info of the last step
    # --- agent side: oracle Q on the recorded batch; greedy / epsilon picks bit-exact ---
    tb = {k: torch.from_numpy(v[sub]) for k, v in nb.items()}
    Tm = int(ep_len[sub].max()) + 1
    q = dict(zip(sub, oracle_q(mac, tb, N, Tm, dtype)))
    n_checked = n_random = n_tie = 0
    for b in sub:
        for t in range(int(ep_len[b]) + 1):
            for n in range(N):
                a = int(nb["actions"][b, t, n, 0])
                av = nb["avail_actions"][b, t, n]
                if not test_mode and eps > 0:
                    key = envref.env_key(args.seed, b)
                    r1 = envref.rng(key, envref.ctr(episode, t, 2, n))
                    if envref.u01(r1) < np.float32(eps):
                        r2 = envref.rng(key, envref.ctr(episode, t, 3, n))
                        assert a == envref.random_available(av.tolist(), r2)
                        n_random += 1
                        continue
                m = np.where(av == 0, -np.inf, q[b][t, n])
                g = int(np.argmax(m))
                srt = np.sort(m)
                if srt[-1] - srt[-2] > Q_TOL:
                    assert a == g, (b, t, n, a, g)
                else:  # near-tie within fp32 tolerance: chosen must be (numerically) a max
                    assert m[a] >= srt[-1] - Q_TOL
                    n_tie += 1
                n_checked += 1
    assert n_checked > 0
    if not test_mode and eps > 0.2:
        assert n_random > 0
    return {"greedy": n_checked, "near_ties": n_tie, "epsilon_draws": n_random}


def sp_args(B, episode_limit, seed, plan="medium_1h_4t", grid_size=20, **kw):
    from maleague.envs.plans import builtin_plan
    mbp = builtin_plan(plan, self_play=True) if isinstance(plan, str) else plan
    return qmix_args(batch_size_run=B, seed=seed,
                     env_args={"match_build_plan": mbp, "grid_size": grid_size,
                               "stochastic_spawns": True, "episode_limit": episode_limit}, **kw)


def build_selfplay(device, plan="medium_1h_4t", B=48, episode_limit=40, seed=5, grid_size=20, **kw):
    """A SelfPlayParallelStepper over ``plan`` (both teams policy-controlled) with two freshly seeded BasicMACs."""
    import torch
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import SelfPlayParallelStepper
    args = sp_args(B, episode_limit, seed, plan, grid_size=grid_size, **kw)
    stepper = SelfPlayParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    assert info["n_agents"] % 2 == 0
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    sinfo = dict(info, n_agents=args.n_agents)
    scheme, groups, preprocess = scheme_for(sinfo, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    torch.manual_seed(seed)
    home = BasicMAC(proto.scheme, groups, args)
    away = BasicMAC(proto.scheme, groups, args)
    stepper.initialize(scheme, groups, preprocess, home, away)
    return stepper, home, away, args


def check_sides(stepper, macs, args, batches, infos, episode, test_mode, eps, envs=None, dtype=None):
    """Teacher-forced env replay of both sides + oracle agent check. ``envs``: the env indices to check (all by
    default; a spread subset at the 4096-env config-3 shape). ``dtype``: the oracle unroll's precision (oracle_q).
    Returns the counts (greedy picks checked, near ties, epsilon draws)."""
    import envref
    import stepper_ref
    import torch
    spec = stepper.spec
    B, N, A, T1 = stepper.batch_size, spec.n_agents // 2, spec.n_actions, stepper.episode_limit + 1
    sub = np.arange(B) if envs is None else np.asarray(envs, dtype=np.int64)
    nbs = [np_batch(b) for b in batches]
    ep_len = stepper.last_run["ep_len"].numpy()
    assert (ep_len >= 1).all() and (ep_len <= stepper.episode_limit).all()
    # --- env side + bookkeeping, teacher forced through the oracle self-play stepper ---
    all_refs = ref_envs_for(spec, B, seed=args.seed)
    refs = [all_refs[int(b)] for b in sub]
    for r in refs:
        r.episode = episode
    pol = [lambda t, run, b, s=s: nbs[s]["actions"][sub[run], t, :, 0] for s in range(2)]
    out = stepper_ref.run_self_play(stepper_ref.RefVecEnv(refs), pol[0], pol[1], len(sub), T1, N, A, 8 * spec.U,
                                    6 * spec.U, test_mode=test_mode)
    for s, key in enumerate(("home", "away")):
        for k, v in out[key].items():
            np.testing.assert_array_equal(nbs[s][k][sub], v, err_msg=f"{key}[{k}]")
    np.testing.assert_array_equal(stepper.last_run["returns"].numpy()[sub], np.float32(out["returns"][0]))
    np.testing.assert_array_equal(stepper.last_run["away_returns"].numpy()[sub], np.float32(out["returns"][1]))
    if envs is None:
        assert stepper.t == out["t"]
        assert [infos[i] for i in range(B)] == out["env_infos"]
        if not test_mode:
            assert int(ep_len.sum()) == out["env_steps"]
    else:
        assert stepper.t == ep_len.max() and len(infos) == B
    # --- agent side per side: oracle Q on the recorded batch; greedy / epsilon picks bit-exact ---
    n_random = n_greedy = n_tie = 0
    for s, (mac, nb) in enumerate(zip(macs, nbs)):
        tb = {k: torch.from_numpy(v[sub]) for k, v in nb.items()}
        q = dict(zip(sub.tolist(), oracle_q(mac, tb, N, int(ep_len[sub].max()) + 1, dtype)))
        for b in sub.tolist():
            for t in range(int(ep_len[b]) + 1):
                for n in range(N):
                    a = int(nb["actions"][b, t, n, 0])
                    av = nb["avail_actions"][b, t, n]
                    if not test_mode and eps[s] > 0:
                        key = envref.env_key(args.seed, b)
                        r1 = envref.rng(key, envref.ctr(episode, t, 2, s * N + n))
                        if envref.u01(r1) < np.float32(eps[s]):
                            r2 = envref.rng(key, envref.ctr(episode, t, 3, s * N + n))
                            assert a == envref.random_available(av.tolist(), r2)
                            n_random += 1
                            continue
                    m = np.where(av == 0, -np.inf, q[b][t, n])
                    srt = np.sort(m)
                    n_greedy += 1
                    if srt[-1] - srt[-2] > Q_TOL:
                        assert a == int(np.argmax(m)), (s, b, t, n)
                    else:
                        assert m[a] >= srt[-1] - Q_TOL
                        n_tie += 1
    if not test_mode and max(eps) > 0.2:
        assert n_random > 0
    return {"greedy": n_greedy, "near_ties": n_tie, "epsilon_draws": n_random}


def assert_near_tie_divergence(ref_sides, got_sides, q_sides, B, tol=1e-5):
    """two kernels that agree in fp32 up to summation order must produce the same episodes except where a
    near-tie flips an argmax. For every episode that differs (over every side of a self-play pair), the first differing
    step t must have identical pre-transition data (state, obs, avail, filled: the env states agree up to t) and differ
    in the actions, and each differing pick must be a near-tie of the fp32 oracle's Q along the recorded trajectory
    (|Q[a_got] - Q[a_ref]| <= tol, both available). Returns the number of differing episodes."""
    import numpy as np
    pre_keys = ("state", "obs", "avail_actions", "filled")
    n_diff = 0
    for b in range(B):
        t_first = None
        T1 = got_sides[0]["actions"].shape[1]
        for t in range(T1):
            if any(not np.array_equal(r[k][b, t], g[k][b, t]) for r, g in zip(ref_sides, got_sides) for k in g):
                t_first = t
                break
        if t_first is None:
            continue
        n_diff += 1
        flips = 0
        for r, g, q in zip(ref_sides, got_sides, q_sides):
            for k in pre_keys:
                if k in g:
                    assert np.array_equal(r[k][b, t_first], g[k][b, t_first]), (b, t_first, k)
            av = g["avail_actions"][b, t_first].astype(bool)
            for n in np.nonzero(r["actions"][b, t_first, :, 0] != g["actions"][b, t_first, :, 0])[0]:
                ag, ar = int(g["actions"][b, t_first, n, 0]), int(r["actions"][b, t_first, n, 0])
                assert av[n, ag] and av[n, ar], (b, t_first, n)
                assert abs(float(q[b, t_first, n, ag]) - float(q[b, t_first, n, ar])) <= tol, (b, t_first, n, ag, ar)
                flips += 1
        assert flips > 0, f"episode {b} diverges at t={t_first} without an action flip"
    return n_diff


# ---- REFIL (entity env) rollout: one launch of mlg_refil_rollout and its teacher-forced check ---------------------

def refil_agent(device, params=None, seed=0, **kw):
    """An ImagineEntityAttentionRNNAgent on ``device`` (refil_args(**kw)): torch-seeded, or with ``params`` loaded
    (state_dict keys -> arrays)."""
    import torch
    from maleague.modules.agents import REGISTRY
    a = refil_args(**kw)
    torch.manual_seed(seed)
    ag = REGISTRY["imagine_entity_attend_rnn"](a.entity_shape + a.n_actions, a).to(device)
    if params is not None:
        sd = ag.state_dict()
        assert set(params) <= set(sd), set(params) - set(sd)
        sd.update({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
        ag.load_state_dict(sd)
    return ag, a


def refil_rollout(device, B=12, T=40, seed=5, eps=0.0, test_mode=True, ring=None, agent_seed=1, st=None, kmin=3, kmax=8,
                  batch=None, extent=None, plan="refil_8", agent_params=None, grid=20):
    """One mlg_refil_rollout launch over ``plan`` (a built-in name or a list of two team dicts) from the env state
    ``st`` (fresh by default; a run advances its episode counters). The agent: torch-seeded with ``agent_seed``, or
    ``agent_params`` -- a callable (d0, n_actions) -> state_dict arrays, or such a dict. ring: full-write mode over a
    garbage-filled batch; extent: the slot extents tensor of full-write mode."""
    import torch
    from maleague import _native
    from maleague.components.batch_view import mlg_entity_batch
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.envs.entity_env import EntityEnvSpec
    from maleague.envs.teams_env import VecEnvState
    spec = EntityEnvSpec.from_env_args({"match_build_plan": plan, "episode_limit": T, "seed": seed, "grid_size": grid,
                                        "min_agents": kmin, "max_agents": kmax})
    info = spec.env_info()
    if callable(agent_params):
        agent_params = agent_params(info["entity_shape"] + info["n_actions"], info["n_actions"])
    ag, a = refil_agent(device, agent_params, seed=agent_seed, n_agents=info["n_agents"],
                        n_entities=info["n_entities"], n_actions=info["n_actions"])
    scheme, groups, pre = entity_scheme_for(info, torch)
    if st is None:
        st = VecEnvState(spec, B, device)
    if batch is None:
        batch = EpisodeBatch(scheme, groups, B, T + 1, preprocess=pre, device=device)
        if ring is not None:
            for v in batch.data.transition_data.values():
                v.fill_(7)
    mb, keep = mlg_entity_batch(batch)
    if ring is not None:
        mb.full_write = 1
    if extent is not None:
        mb.slot_extent = extent.data_ptr()
    run = torch.zeros(6 * B, dtype=torch.int32, device=device)
    ri = _native.MlgRunInfo(run[0:B].data_ptr(), run[4 * B:5 * B].data_ptr(), run[B:3 * B].data_ptr(),
                            run[3 * B:4 * B].data_ptr(), None, None)
    _native.call("mlg_refil_rollout", _native.byref(spec.to_c()), _native.byref(st.to_c()), _native.byref(ag.dims()),
                 _native.ptr(ag.packed()), _native.byref(mb), _native.byref(ri), float(eps), int(test_mode),
                 _native.stream_ptr())
    torch.cuda.synchronize()
    r = run.cpu().numpy()
    summary = {"len": r[0:B], "won": r[B:3 * B].reshape(B, 2), "draw": r[3 * B:4 * B],
               "ret": r[4 * B:5 * B].view(np.float32)}
    if extent is not None:
        refil_rollout.last_batch = batch
    return spec, ag, a, np_batch(batch), summary, st


def refil_oracle_q(ag, a, nb, envs=None, dtype=None):
    """The oracle EntityMAC's Q [len(envs), T1, NA, A] along a recorded batch (refil_ref.mac_forward) with the agent's
    parameters: fp32 by default, or parameters and inputs cast to ``dtype`` (torch.float64: strictly more precise than
    the kernels)."""
    import torch
    import refil_ref as RR
    p = {k: v.detach().cpu() for k, v in ag.state_dict().items()}
    sel = slice(None) if envs is None else envs
    keys = ("entities", "obs_mask", "entity_mask", "actions_onehot")  # what EntityMAC._build_inputs reads
    tb = {k: torch.from_numpy(np.array(nb[k][sel])) for k in keys}    # copies: the host arrays may be read-only
    if dtype is not None:
        p = {k: v.to(dtype) if v.is_floating_point() else v for k, v in p.items()}
        tb = {k: v.to(dtype) if k in ("entities", "actions_onehot") else v for k, v in tb.items()}
    with torch.no_grad():
        return RR.mac_forward(p, tb, a)[0].numpy()


def refil_teacher_check(spec, ag, a, nb, summ, B, T, seed, eps, test_mode, envs=None, dtype=None, episode=0):
    """Replay the recorded actions of ``envs`` (default: all) through the oracle entity env at episode index
    ``episode``: entities, masks, avail, reward, terminated, filled, one-hot rows, lengths, won / draw bit-exact
    (returns within 1e-3); every epsilon draw the oracle's draw from the counter RNG; every other pick an argmax of the oracle's
    masked Q (``dtype``: refil_oracle_q), a different pick passing only where the top-two gap is within Q_TOL and the
    pick within Q_TOL of the maximum. Returns the counts: greedy picks, decisions (greedy picks with at least two
    available actions), near ties among them, epsilon draws."""
    import envref
    envs = list(range(B)) if envs is None else [int(e) for e in envs]
    refs = ref_entity_envs_for(spec, B, seed=seed)
    NA, A = spec.n_agents, spec.n_actions
    qref = dict(zip(envs, refil_oracle_q(ag, a, nb, envs, dtype)))
    n_rand = n_greedy = n_dec = n_tie = 0
    for b in envs:
        r = refs[b]
        r.episode = episode
        r.reset()
        L = int(summ["len"][b])
        assert 1 <= L <= T
        ret = np.float32(0)
        for t in range(L + 1):
            ent, om, em = r.entities()
            np.testing.assert_array_equal(nb["entities"][b, t], ent, err_msg=f"entities b={b} t={t}")
            np.testing.assert_array_equal(nb["obs_mask"][b, t], om, err_msg=f"obs_mask b={b} t={t}")
            np.testing.assert_array_equal(nb["entity_mask"][b, t], em)
            av = r.avail()
            np.testing.assert_array_equal(nb["avail_actions"][b, t], av)
            assert nb["filled"][b, t, 0] == 1
            acts = nb["actions"][b, t, :, 0]
            for n in range(NA):
                key = envref.env_key(seed, b)
                u = envref.u01(envref.rng(key, envref.ctr(r.cur_episode, t, 2, n)))
                coin = not test_mode and eps > 0 and u < np.float32(eps)  # the kernel compares in fp32
                if coin:
                    want = envref.random_available(av[n], envref.rng(key, envref.ctr(r.cur_episode, t, 3, n)))
                    assert acts[n] == want
                    n_rand += 1
                else:
                    qm = np.where(av[n] != 0, qref[b][t, n], -np.inf)
                    srt = np.sort(qm)
                    assert av[n, acts[n]] != 0 and qm[acts[n]] >= qm.max() - Q_TOL, (b, t, n)
                    if srt[-1] - srt[-2] > Q_TOL:
                        assert acts[n] == int(np.argmax(qm)), (b, t, n, int(acts[n]), int(np.argmax(qm)))
                    else:
                        n_tie += 1
                    n_dec += int(np.isfinite(srt[-2]))
                    n_greedy += 1
            oh = np.zeros((NA, A), np.float32)
            oh[np.arange(NA), acts] = 1
            np.testing.assert_array_equal(nb["actions_onehot"][b, t], oh)
            if t < L:
                rew, done, info = r.step(acts)
                assert nb["reward"][b, t, 0] == np.float32(rew[0])
                assert nb["terminated"][b, t, 0] == int(done)
                assert done == (t == L - 1)
                ret += np.float32(rew[0])
        assert summ["won"][b, 0] == int(info["battle_won"][0]) and summ["won"][b, 1] == int(info["battle_won"][1])
        assert summ["draw"][b] == int(info["draw"])
        assert abs(summ["ret"][b] - ret) <= 1e-3
        assert nb["filled"][b, L + 1:].sum() == 0 and nb["reward"][b, L:].sum() == 0
    assert n_greedy > 0 and (test_mode or n_rand > 0)
    return {"greedy": n_greedy, "decisions": n_dec, "near_ties": n_tie, "epsilon_draws": n_rand}


# ---- COMA: args, the policy rollout checker, the critic harness, random batches ----

DELTA = 2e-4
NEAR_TIE_CAP = 0.02


def coma_args(**kw):
    a = dict(agent_output_type="pi_logits", action_selector="multinomial", epsilon_start=0.5, epsilon_finish=0.01,
             epsilon_anneal_time=100000, mask_before_softmax=False, critic_lr=0.0005, td_lambda=0.8, learner="coma",
             critic_train_mode="seq", q_nstep=0, test_greedy=True, target_update_interval=200, mixer=None)
    a.update(kw)
    return qmix_args(**a)


def _golden_batch(b, device):
    import torch
    from maleague.components.episode_batch import EpisodeBatch
    B, T, N, _ = b["obs"].shape
    info = {"state_shape": b["state"].shape[-1], "obs_shape": b["obs"].shape[-1],
            "n_actions": b["avail_actions"].shape[-1], "n_agents": N}
    scheme, groups, preprocess = scheme_for(info, torch)
    eb = EpisodeBatch(scheme, groups, B, T, preprocess=preprocess, device=device)
    for k, v in b.items():
        eb.data.transition_data[k].copy_(torch.as_tensor(v))
    return eb


def _policy_stepper(device, plan, H, mask, B=17, episode_limit=12, seed=5, agent_params=None, fc2_scale=8.0,
                    test_greedy=True, grid_size=20):
    """A ParallelStepper with a pi_logits BasicMAC (epsilon 0.3 flat). The agent: torch-seeded, or ``agent_params``, a
    callable (d_in, H, n_actions) -> state_dict arrays; fc2.weight is multiplied by ``fc2_scale`` either way."""
    import torch
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import ParallelStepper
    args = coma_args(batch_size_run=B, seed=seed, rnn_hidden_dim=H, mask_before_softmax=mask, epsilon_start=0.3,
                     epsilon_finish=0.3, test_greedy=test_greedy,
                     env_args={"match_build_plan": plan, "grid_size": grid_size, "stochastic_spawns": True,
                               "episode_limit": episode_limit})
    stepper = ParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"], info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(info, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    torch.manual_seed(seed)
    mac = BasicMAC(proto.scheme, groups, args)
    if agent_params is not None:
        d = mac.agent.dims()
        mac.agent.load_state_dict({k: torch.from_numpy(v) for k, v in agent_params(d.d_in, H, d.n_actions).items()})
    with torch.no_grad():  # a sharper policy than the initialisation's near-uniform one: few near-tie rows
        mac.agent.fc2.weight.mul_(fc2_scale)
    mac.agent.mark_dirty()
    stepper.initialize(scheme, groups, preprocess, mac)
    return stepper, mac, args, (scheme, groups, preprocess)


def _check_policy_run(stepper, mac, args, batch, episode, test_mode, mask, test_greedy=True, stats=None):
    """Env tensors bit-exact against the C env under teacher forcing; every pick against the float64 policy along the
    recorded batch: a draw (train mode, or test mode without test_greedy: the floor-less probabilities) within DELTA
    of the restated cdf, a greedy pick the argmax but for near ties (at most NEAR_TIE_CAP of the rows). ``stats``: a
    dict that receives rows, near_ties and the largest distance of a draw's threshold outside its cdf interval."""
    import torch
    import coma_ref as CR
    import envref
    import learner_ref as LR
    spec = stepper.spec
    B, N, A, T1 = stepper.batch_size, spec.n_agents, spec.n_actions, stepper.episode_limit + 1
    nb = np_batch(batch)
    ep_len = stepper.last_run["ep_len"].numpy()
    refs = ref_envs_for(spec, B, seed=args.seed)
    for b, r in enumerate(refs):  # env tensors bit-exact against the C env, teacher forced with the recorded actions
        r.episode = episode
        r.reset()
        L = int(ep_len[b])
        np.testing.assert_array_equal(nb["obs"][b, 0], r.obs())
        np.testing.assert_array_equal(nb["avail_actions"][b, 0], r.avail())
        for t in range(L):
            rew, done, _ = r.step(nb["actions"][b, t, :, 0])
            assert nb["reward"][b, t, 0] == np.float32(rew[0])
            assert nb["terminated"][b, t, 0] == int(done) and done == (t == L - 1)
            np.testing.assert_array_equal(nb["obs"][b, t + 1], r.obs())
            np.testing.assert_array_equal(nb["state"][b, t + 1], r.state())
            np.testing.assert_array_equal(nb["avail_actions"][b, t + 1], r.avail())
        np.testing.assert_array_equal(nb["filled"][b, :, 0], (np.arange(T1) <= L).astype(np.int64))
        assert (nb["actions"][b, L + 1:] == 0).all() and (nb["actions_onehot"][b, L + 1:] == 0).all()
        oh = np.zeros((L + 1, N, A), np.float32)
        oh[np.arange(L + 1)[:, None], np.arange(N)[None, :], nb["actions"][b, :L + 1, :, 0]] = 1
        np.testing.assert_array_equal(nb["actions_onehot"][b, :L + 1], oh)
    params = {k: v.detach().cpu().double() for k, v in mac.agent.state_dict().items()}
    tb = {k: torch.from_numpy(nb[k]).double() for k in ("obs", "actions_onehot")}
    Tm = int(ep_len.max()) + 1
    with torch.no_grad():
        logits, _ = LR.mac_unroll(params, tb, N, T=Tm, h0=torch.zeros(B * N, args.rnn_hidden_dim, dtype=torch.float64))
    probs = CR.softmax_policy(logits.numpy(), nb["avail_actions"][:, :Tm], 0.3, mask, test_mode)
    m = np.where(nb["avail_actions"][:, :Tm] != 0, probs, 0.0)
    rows = near = 0
    greedy, worst = test_mode and test_greedy, 0.0
    for b in range(B):
        key = envref.env_key(args.seed, b)
        for t in range(int(ep_len[b]) + 1):
            for n in range(N):
                a = int(nb["actions"][b, t, n, 0])
                assert nb["avail_actions"][b, t, n, a] != 0, (b, t, n, a)
                rows += 1
                if greedy:
                    srt = np.sort(m[b, t, n])
                    if srt[-1] - srt[-2] < DELTA:
                        near += 1
                        assert m[b, t, n, a] >= srt[-1] - DELTA
                    else:
                        assert a == int(np.argmax(m[b, t, n])), (b, t, n)
                    continue
                cdf = np.cumsum(m[b, t, n])
                thr = float(CR.policy_u(key, episode, t, n)) * cdf[-1]
                lo = cdf[a - 1] if a > 0 else 0.0
                worst = max(worst, lo - thr, thr - cdf[a])
                assert lo - DELTA <= thr < cdf[a] + DELTA, (b, t, n, a, lo, thr, cdf[a])
    assert rows == int((ep_len + 1).sum()) * N
    if stats is not None:
        stats.update(rows=rows, near_ties=near, cdf_excess=worst)
    if greedy:
        assert near <= NEAR_TIE_CAP * rows, f"{near} near-tie rows of {rows}"
    return rows


class CriticHarness:
    """Flat device buffers around mlg_coma_critic_train / mlg_coma_target_update."""

    def __init__(self, params, device, B, T, N, A, d_obs, S, interval=200, ws_fill=float("nan")):
        import torch
        import coma_ref as CR
        from maleague import _native
        self.n = _native
        self.cfg = _native.MlgComaCfg(B=B, T=T, N=N, A=A, d_obs=d_obs, S=S, hidden=128, lr=5e-4, optim_alpha=0.99,
                                      optim_eps=1e-5, grad_norm_clip=10.0, gamma=0.99, td_lambda=0.8)
        lib = _native.load(require_gpu=True)
        flat = np.concatenate([np.asarray(params[k], np.float32).reshape(-1) for k in CR.CRITIC_KEYS])
        assert lib.mlg_coma_param_count(_native.byref(self.cfg)) == flat.size
        self.params = torch.tensor(flat, device=device)
        self.target = self.params.clone()
        self.grads, self.sq = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.ws = torch.full((lib.mlg_coma_workspace_floats(_native.byref(self.cfg)),), ws_fill, device=device)
        self.q_vals = torch.full((B, T - 1, N, A), float("nan"), device=device)
        self.targets = torch.full((B, T - 1, N), float("nan"), device=device)
        self.stats = torch.full((6,), float("nan"), device=device)
        self.counters = torch.zeros(2, dtype=torch.int64, device=device)
        self.interval = interval
        self.ws_fill = ws_fill

    def refill(self):
        """The workspace and the outputs back to their fill values: a call must not read what the last one left."""
        self.ws.fill_(self.ws_fill)
        for v in (self.q_vals, self.targets, self.stats):
            v.fill_(float("nan"))

    def train(self, eb, rows=None):
        from maleague.components.batch_view import mlg_batch
        n = self.n
        mb, keep = mlg_batch(eb)
        if rows is not None:
            mb.B, mb.rows = len(rows), rows.data_ptr()
        bufs = n.MlgComaBufs(mb, self.params.data_ptr(), self.grads.data_ptr(), self.sq.data_ptr(),
                             self.target.data_ptr(), self.ws.data_ptr(), self.q_vals.data_ptr(),
                             self.targets.data_ptr(), self.stats.data_ptr(), self.counters.data_ptr())
        n.call("mlg_coma_critic_train", n.byref(self.cfg), n.byref(bufs), n.stream_ptr())
        n.call("mlg_coma_target_update", self.params.data_ptr(), self.target.data_ptr(), self.params.numel(),
               self.counters.data_ptr(), self.interval, n.stream_ptr())
        del keep
        return self.q_vals.cpu().numpy(), self.targets.cpu().numpy(), self.stats.cpu().numpy()


def _random_batch(B, T, N, A, d_obs, S, lengths, seed):
    rng = np.random.RandomState(seed)
    b = {"state": np.zeros((B, T, S), np.float32), "obs": np.zeros((B, T, N, d_obs), np.float32),
         "actions": np.zeros((B, T, N, 1), np.int64), "avail_actions": np.zeros((B, T, N, A), np.int32),
         "reward": np.zeros((B, T, 1), np.float32), "terminated": np.zeros((B, T, 1), np.uint8),
         "actions_onehot": np.zeros((B, T, N, A), np.float32), "filled": np.zeros((B, T, 1), np.int64)}
    for e, L in enumerate(lengths):
        n = min(L + 1, T)
        b["state"][e, :n] = rng.randn(n, S)
        b["obs"][e, :n] = rng.randn(n, N, d_obs)
        b["avail_actions"][e, :n] = 1
        acts = rng.randint(A, size=(n, N))
        b["actions"][e, :n, :, 0] = acts
        b["actions_onehot"][e, :n] = np.eye(A, dtype=np.float32)[acts]
        b["filled"][e, :n] = 1
        b["reward"][e, :min(L, T)] = rng.randn(min(L, T), 1)
        if L <= T - 1:
            b["terminated"][e, L - 1] = 1
    return b


def _random_critic(D, A, seed):
    rng = np.random.RandomState(seed)
    shapes = {"fc1.weight": (128, D), "fc1.bias": (128,), "fc2.weight": (128, 128), "fc2.bias": (128,),
              "fc3.weight": (A, 128), "fc3.bias": (A,)}
    return {k: (rng.uniform(-1, 1, s) / np.sqrt(s[-1] if len(s) > 1 else 128)).astype(np.float32)
            for k, s in shapes.items()}


