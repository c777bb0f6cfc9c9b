"""GPU parity of every rollout entry point where episodes end early: mlg_rollout, mlg_rollout_selfplay, mlg_rollout_ff,
mlg_rollout_selfplay_ff, mlg_rollout_distinct, mlg_rollout_selfplay_distinct and mlg_rollout_policy, one eventful case
per dispatch arm (tests/rollout_event_shapes.py holds the cases, the recipe that makes them eventful and what the
float64 oracle alone sees on them; tests/test_rollout_event_shapes.py pins the arms and the small cases' counts on the CPU).

The per-arm suites play a 20-cell grid on which nearly every env runs to the limit. Here units die, teams win and the
envs of a workgroup end many steps apart, so the shrinking running list, the action recorded after termination while
other envs keep stepping, the win reward and battle_won flags, the dead agents' rows and the tail zeroing of full-write
mode all see non-trivial inputs on every arm.

Per case: the arm is the table's (stepper.describe_rollout); a test-mode and a train-mode run go through the family's
checker (helpers.check_run / check_sides / _check_policy_run) against the float64 oracle with the 1 % near-tie cap, the
infos against the oracle's final info per env in termination order; the run itself must be eventful (at least half the
early-ending envs the oracle alone sees and never fewer than 2, a ragged workgroup, the case's win conditions); and a
run written in full-write mode over ring slots that hold an earlier, longer episode equals the plain run bit for bit.
Kernel pairs that agree bit for bit today do so on one eventful case each, and the split-bf16 arms leave their fp32
arm's episodes only at near ties. Each test prints its arm, near-tie counts and event counts (`pytest -s`).
"""
import numpy as np
import pytest
import torch

import distinct_ref as DR
import dqn_selfplay_shapes as FSP
import helpers
import rollout_event_shapes as ES
from helpers import (_check_policy_run, _policy_stepper, assert_near_tie_divergence, np_batch, oracle_q, qmix_args,
                     scheme_for, shape_plan)

pytestmark = pytest.mark.gpu

NEAR_TIE_CAP = 0.01
F64 = torch.float64
# episodes (of 37, test mode) of a split-bf16 arm that leave the fp32 arm's trajectory at a near-tie argmax flip on the
# eventful case: the measured count plus the margin of 2 that V7_MAX_DIVERGING / SP7_MAX_DIVERGING use
MAX_DIVERGING = {
    "ev-v7-4v4": 2,        # measured 0 (v7 vs v2)
    "ev-v7static-5v5": 2,  # measured 0 (v7-static vs v2)
    "ev-sp7-4v4": 2,       # measured 0 (sp7 vs sp2)
    "ev-sp8-3v3": 2,       # measured 0 (sp8 vs sp2)
}
Q_IDS = [c.id for c in ES.CASES if c.family != "policy"]
POLICY_IDS = ES.ids(family="policy")


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    for k in ("MLG_ROLLOUT_KERNEL", "MLG_ROLLOUT_GENERIC", "MLG_ROLLOUT_GLOBAL_WEIGHTS"):
        monkeypatch.delenv(k, raising=False)


def _case(cid, monkeypatch):
    """The case, with its environment set and the checkers' oracle swapped for its family's."""
    c = ES.case(cid)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    if c.family == "ff":
        monkeypatch.setattr(helpers, "oracle_q", FSP.oracle_q)
    elif c.family == "dx":
        monkeypatch.setattr(helpers, "oracle_q", DR.oracle_q)
    return c


def _build(device, c, params=None):
    """The case's stepper (ParallelStepper, or the family's self-play stepper) with one MAC per side holding the
    case's weights, or ``params`` (per side a state dict, for a DistinctMAC the list of its networks' dicts)."""
    from maleague import steppers as S
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC, DistinctMAC
    from maleague.custom_logging import MainLogger
    la, ai = c.flags
    kw = {"ff": {"agent": "dqn"}, "dx": {"mac": "distinct"}}.get(c.family, {})
    env_args = {k: v for k, v in ES.env_args(c).items() if k != "seed"}
    args = qmix_args(batch_size_run=ES.B, seed=c.seed, rnn_hidden_dim=c.H, obs_last_action=la, obs_agent_id=ai,
                     env_args=env_args, **kw)
    cls = {"drqn": S.SelfPlayParallelStepper, "ff": S.SelfPlayFFParallelStepper,
           "dx": S.SelfPlayDistinctParallelStepper}[c.family] if c.sp else S.ParallelStepper
    stepper = cls(args, MainLogger())
    info = stepper.get_env_info()
    sides = 2 if c.sp else 1
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // sides, info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(dict(info, n_agents=args.n_agents), torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    macs = [(DistinctMAC if c.family == "dx" else BasicMAC)(proto.scheme, groups, args) for _ in range(sides)]
    d_in = macs[0].input_shape if c.family == "dx" else macs[0].agent.input_shape
    params = params if params is not None else ES.side_params(c, d_in, args.n_agents, args.n_actions)
    for mac, p in zip(macs, params):
        if c.family == "dx":
            DR.load_agents(mac, p)
            mac.cuda()
        else:
            mac.agent.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
            mac.agent.to(device)
    if c.sp:  # the away policy is a frozen snapshot with its own selector state
        macs[1].action_selector.schedule.eval = lambda t_env: ES.EPS_AWAY
    stepper.initialize(scheme, groups, preprocess, *macs)
    return stepper, macs, args, (scheme, groups, preprocess)


def _build_policy(device, c):
    stepper, mac, args, sch = _policy_stepper(device, shape_plan(c.plan), c.H, True, B=ES.B, episode_limit=c.limit,
                                              seed=c.seed, agent_params=ES.policy_agent_params(c),
                                              fc2_scale=ES.POLICY_SCALE, grid_size=c.grid)
    return stepper, [mac], args, sch


def _summary(stepper):
    """(ep_len [B], won [B, 2]) of the last run, from the run's own summary."""
    stepper.flush()
    torch.cuda.synchronize()
    B = stepper.batch_size
    info = stepper.last_run_info().cpu().numpy()
    ep_len = stepper.last_run["ep_len"].numpy()
    np.testing.assert_array_equal(info[0:B], ep_len)
    return ep_len.copy(), info[B:3 * B].reshape(B, 2).copy()


def _cap(c, mode, n):
    print(f"{c.id} [{mode}]: {n}  ({100.0 * n['near_ties'] / n['greedy']:.3f} % near ties, cap 1 %)")
    assert n["near_ties"] <= NEAR_TIE_CAP * n["greedy"], (c.id, mode, n)


def _assert_eventful(c, lens, wons):
    """The event conditions on the GPU runs themselves: a condition on the inputs, not a tolerance."""
    n = dict(ES.events(lens, wons, c.limit), envs=sum(len(L) for L in lens))
    floor = max(2, (c.oracle["early"] + 1) // 2)
    print(f"{c.id}: GPU runs: {n['early']} early-ending envs of {n['envs']} (oracle alone {c.oracle['early']}, at "
          f"least {floor}), {n['ragged']} ragged workgroups, wins {n['home_wins']} / {n['away_wins']}, "
          f"{n['draws']} draws")
    bad = ES.conditions(c, n, early_floor=floor, ragged_floor=1)
    assert not bad, (c.id, bad, n)


# ---- 1. parity, infos and the event conditions per case -------------------------------------------------------------

@pytest.mark.parametrize("cid", Q_IDS)
def test_eventful_parity(device, cid, monkeypatch):
    c = _case(cid, monkeypatch)
    stepper, macs, args, _ = _build(device, c)
    name, lds = stepper.describe_rollout()
    print(f"{cid}: arm {name}, {lds} B of LDS, B = {ES.B}, grid {c.grid}, limit {c.limit}")
    assert name == c.arm
    lens, wons = [], []
    for episode, test_mode in ((0, True), (1, False)):
        if not test_mode:
            assert stepper.t_env == 0
            stepper.t_env = ES.T_ENV
        out = stepper.run(test_mode=test_mode)
        if c.sp:
            eps = (0.0, 0.0) if test_mode else (ES.EPS_HOME, ES.EPS_AWAY)
            n = helpers.check_sides(stepper, macs, args, out[:2], out[2], episode=episode, test_mode=test_mode,
                                    eps=eps, dtype=F64)
        else:
            n = helpers.check_run(stepper, macs[0], args, out[0], out[1], episode=episode, test_mode=test_mode,
                                  eps=0.0 if test_mode else ES.EPS_HOME, dtype=F64)
        _cap(c, "test" if test_mode else "train", n)
        L, won = _summary(stepper)
        lens.append(L)
        wons.append(won)
    assert n["epsilon_draws"] > 0
    assert stepper.t_env == ES.T_ENV + int(lens[1].sum())
    _assert_eventful(c, lens, wons)


def test_checker_rejects_infos_out_of_termination_order(device, monkeypatch):
    """check_run compares the infos with the oracle's final info per env in termination order: two infos that differ,
    swapped, must raise (the 3v3 H = 128 case ends in policy wins, scripted wins and draws)."""
    c = _case("ev-v1glb1-3v3", monkeypatch)
    stepper, macs, args, _ = _build(device, c)
    batch, infos = stepper.run(test_mode=True)
    helpers.check_run(stepper, macs[0], args, batch, infos, episode=0, test_mode=True, eps=0.0, dtype=F64)
    wrong = list(infos)
    assert len({str(i) for i in wrong}) == 3, "policy wins, scripted wins and draws expected"
    j = next(j for j in range(1, len(wrong)) if wrong[j] != wrong[0])
    wrong[0], wrong[j] = wrong[j], wrong[0]
    with pytest.raises(AssertionError) as exc:
        helpers.check_run(stepper, macs[0], args, batch, wrong, episode=0, test_mode=True, eps=0.0, dtype=F64)
    assert "battle_won" in str(exc.value), exc.value  # raised by the infos comparison


def _policy_infos(stepper, args, batch, infos, episode):
    """The infos of a policy run against the oracle env's final info per env (replayed with the recorded actions), in
    termination order: by episode length, then env index."""
    nb = np_batch(batch)
    ep_len = stepper.last_run["ep_len"].numpy()
    B = stepper.batch_size
    assert len(infos) == B
    order = np.lexsort((np.arange(B), ep_len))
    refs = helpers.ref_envs_for(stepper.spec, B, seed=args.seed)
    final = []
    for b, r in enumerate(refs):
        r.episode = episode
        r.reset()
        for t in range(int(ep_len[b])):
            _, done, info = r.step(nb["actions"][b, t, :, 0])
        assert done
        final.append(info)
    for i, b in enumerate(order):
        assert infos[i] == final[b], (i, int(b), infos[i], final[b])


@pytest.mark.parametrize("cid", POLICY_IDS)
def test_eventful_policy_parity(device, cid, monkeypatch):
    """Episode 0 in masked-greedy test mode, episode 1 in train mode (a draw at epsilon 0.3)."""
    c = _case(cid, monkeypatch)
    stepper, (mac,), args, _ = _build_policy(device, c)
    name, lds = stepper.describe_rollout()
    print(f"{cid}: arm {name}, {lds} B of LDS, B = {ES.B}, grid {c.grid}, limit {c.limit}")
    assert name == c.arm
    lens, wons = [], []
    for episode, test_mode in ((0, True), (1, False)):
        batch, infos = stepper.run(test_mode=test_mode)
        st = {}
        _check_policy_run(stepper, mac, args, batch, episode, test_mode, True, test_greedy=True, stats=st)
        _policy_infos(stepper, args, batch, infos, episode)
        if test_mode:
            print(f"{cid} [greedy]: {st['near_ties']} near ties of {st['rows']} rows "
                  f"({100.0 * st['near_ties'] / st['rows']:.3f} %, cap 1 %)")
            assert st["near_ties"] <= NEAR_TIE_CAP * st["rows"], (cid, st)
        else:
            print(f"{cid} [train]: {st['rows']} rows, largest distance of a draw outside its cdf interval "
                  f"{max(st['cdf_excess'], 0.0):.3g}")
        L, won = _summary(stepper)
        lens.append(L)
        wons.append(won)
    _assert_eventful(c, lens, wons)


# ---- 2. full-write (ring) mode over slots that hold an earlier, longer episode --------------------------------------

def _clone(batch):
    return {k: batch[k].clone() for k in batch.data.transition_data}


@pytest.mark.parametrize("cid", ES.IDS)
def test_eventful_ring_mode_equals_plain_run(device, cid, monkeypatch):
    """Three train-mode runs (episodes 0, 1, 2 from fresh env state) written straight into a replay ring of B + 5
    slots: the first over foreign bytes, the second and third over the episodes the earlier runs left (slots 37..41,
    0..31, then 32..41, 0..26). Each equals the plain run into a zero-initialised batch bit for bit, key by key, tails
    included; slot extents follow. The reused slots must hold a filled row of an earlier, longer episode past the new
    episode's end in at least 2 envs over the two reusing runs: there the tail has to be zeroed, and one such env
    already shows a tail left behind. (Asked of each reusing run at first; on the 5v5 self-play cases, where about 5 of
    37 envs end early per run, the third run met no longer episode: 3 / 0, 3 / 0 and 6 / 0 envs. A condition on the
    inputs; the bit equality held in every run.) Self-play: the away episodes go
    in full-write mode into the reused away batch, over foreign bytes first, then over the previous run's episodes."""
    from maleague.components.replay_buffer import ReplayBuffer
    from maleague.envs.teams_env import VecEnvState
    c = _case(cid, monkeypatch)
    stepper, macs, args, (scheme, groups, preprocess) = _build_policy(device, c) if c.family == "policy" \
        else _build(device, c)
    assert stepper.describe_rollout()[0] == c.arm
    B, size, T1 = ES.B, ES.B + 5, c.limit + 1
    ring = ReplayBuffer(scheme, groups, size, T1, preprocess=preprocess, device=device)
    for v in ring.data.transition_data.values():
        v.fill_(7)
    longer = []
    for it in range(3):
        runs = []
        for use_ring in (False, True):
            st = VecEnvState(stepper.spec, B, device)
            st.episode.fill_(it)
            stepper.envs = st
            stepper.t_env = ES.T_ENV
            stepper._ring = None
            if c.sp:
                stepper.args.reuse_away_batch = use_ring  # plain: a fresh zero-initialised away batch per run
            if use_ring:
                slots = (torch.arange(B) + ring.buffer_index) % size
                held = ring["filled"][slots.to(device)].cpu()[:, :, 0]  # what the slots hold before the run
                L = runs[0][2]
                longer.append(sum(int(held[b, int(L[b]) + 1:].eq(1).any()) for b in range(B)))
                assert stepper.attach_replay(ring)
                if c.sp and it == 0 and stepper._away_buf is not None:  # written from outside: every row unknown
                    for v in stepper._away_buf.data.transition_data.values():
                        v.fill_(7)
                    stepper._away_extent.fill_(T1)
            out = stepper.run(test_mode=False)
            stepper.flush()
            runs.append(([_clone(b) for b in out[:-1]], out[0], stepper.last_run["ep_len"].clone()))
        plain, ringed = runs
        assert torch.equal(plain[2], ringed[2]), (cid, it)
        for side, (p, r) in enumerate(zip(plain[0], ringed[0])):
            for k in p:
                assert torch.equal(p[k], r[k]), (cid, it, side, k)
        ring.insert_episode_batch(ringed[1])
        slots = (torch.arange(B) + ringed[1].slot0) % size
        want = (ringed[2] + 1).to(torch.int32)
        assert torch.equal(ring.slot_extent.cpu()[slots], want), (cid, it)
        if c.sp:
            assert torch.equal(stepper._away_extent.cpu(), want), (cid, it)
    print(f"{cid}: arm {c.arm}, reused slots holding an earlier, longer episode per run: {longer}")
    assert longer[0] == 0 and sum(longer[1:]) >= 2, (cid, longer)


# ---- 3. kernel against kernel, bit for bit --------------------------------------------------------------------------

def _two_runs(stepper, device):
    """A test-mode run of episode 0 and a train-mode run of episode 1 from fresh env state: per run everything it
    stores (the batches, ep_len, won, draw and the returns as int32 bits)."""
    from maleague.envs.teams_env import VecEnvState
    B = stepper.batch_size
    if hasattr(stepper.args, "reuse_away_batch"):
        stepper.args.reuse_away_batch = False
    snaps = []
    for episode, test_mode in ((0, True), (1, False)):
        st = VecEnvState(stepper.spec, B, device)
        st.episode.fill_(episode)
        stepper.envs = st
        stepper.t_env = ES.T_ENV
        out = stepper.run(test_mode=test_mode)
        stepper.flush()
        torch.cuda.synchronize()
        snap = {f"{side}.{k}": v for side, b in zip(("home", "away"), out[:-1]) for k, v in _clone(b).items()}
        snap["summary"] = stepper.last_run_info().cpu().clone()
        snaps.append(snap)
    return snaps


def _assert_same_runs(a, b, what):
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            assert torch.equal(x[k], y[k]), (what, k)


def _early(snaps, c):
    B = ES.B
    return [int((s["summary"][0:B] < c.limit).sum()) for s in snaps]


@pytest.mark.parametrize("cid,forced,arm", [("ev-v2-5v7", "v1", "v1-"), ("ev-sp2-5v5", "v1", "v1-global")],
                         ids=["v2-equals-v1", "sp2-equals-v1"])
def test_eventful_compacted_kernel_equals_generic(device, cid, forced, arm, monkeypatch):
    """v2 = v1 and sp2 = v1 (the same arithmetic order): both runs of the default arm and of
    MLG_ROLLOUT_KERNEL=v1 store the same bits, on envs that end early."""
    c = _case(cid, monkeypatch)
    stepper, macs, args, _ = _build(device, c)
    assert stepper.describe_rollout()[0] == c.arm
    default = _two_runs(stepper, device)
    monkeypatch.setenv("MLG_ROLLOUT_KERNEL", forced)
    assert stepper.describe_rollout()[0].startswith(arm)
    generic = _two_runs(stepper, device)
    print(f"{cid}: {c.arm} against {stepper.describe_rollout()[0]}, early-ending envs per run {_early(default, c)}")
    assert min(_early(default, c)) >= 2
    _assert_same_runs(default, generic, cid)


def test_eventful_ff_lds_equals_global(device, monkeypatch):
    """ffsp-lds = ffsp-global: the arms differ in where a weight is read from, not in the order of any sum."""
    c = _case("ev-ffsplds1-3v3", monkeypatch)
    forced = ES.case("ev-ffspglb1-3v3-forced")
    stepper, macs, args, _ = _build(device, c)
    assert stepper.describe_rollout()[0] == c.arm
    lds = _two_runs(stepper, device)
    for k, v in forced.env.items():
        monkeypatch.setenv(k, v)
    assert stepper.describe_rollout()[0] == forced.arm
    glob = _two_runs(stepper, device)
    print(f"{c.id}: {c.arm} against {forced.arm}, early-ending envs per run {_early(lds, c)}")
    assert min(_early(lds, c)) >= 2
    _assert_same_runs(lds, glob, c.id)


def test_eventful_equal_networks_equal_basic_mac_on_the_generic_kernel(device, monkeypatch):
    """distinct = generic with equal networks: N copies of network 0 in a DistinctMAC store, bit for bit, what a
    BasicMAC (obs_agent_id off) with those weights stores under MLG_ROLLOUT_KERNEL=v1, on envs that end early."""
    c = _case("ev-dx1-3v3", monkeypatch)
    monkeypatch.setenv("MLG_ROLLOUT_KERNEL", "v1")
    spec = ES.spec_of(c)
    ps = ES.side_params(c, ES.dims_of(c, spec).d_in, spec.n_agents, spec.n_actions)[0]
    stepper, _, _, _ = _build(device, c, params=[[ps[0]] * spec.n_agents])
    ref_stepper, _, _, _ = _build(device, c._replace(family="drqn"), params=[ps[0]])
    assert stepper.describe_rollout()[0] == c.arm and ref_stepper.describe_rollout()[0].startswith("v1-")
    got, want = _two_runs(stepper, device), _two_runs(ref_stepper, device)
    print(f"{c.id}: {c.arm} against {ref_stepper.describe_rollout()[0]}, early-ending envs per run {_early(want, c)}")
    assert min(_early(want, c)) >= 2
    _assert_same_runs(got, want, c.id)


# ---- 4. the split-bf16 arms against their fp32 arm ------------------------------------------------------------------

def _test_run(stepper, device, kernel, monkeypatch):
    from maleague.envs.teams_env import VecEnvState
    if kernel is None:  # the default arm
        monkeypatch.delenv("MLG_ROLLOUT_KERNEL", raising=False)
    else:
        monkeypatch.setenv("MLG_ROLLOUT_KERNEL", kernel)
    arm = stepper.describe_rollout()[0]
    stepper.envs = VecEnvState(stepper.spec, stepper.batch_size, device)
    out = stepper.run(test_mode=True)
    return [np_batch(b) for b in out[:-1]], stepper.last_run["ep_len"].numpy().copy(), arm


@pytest.mark.parametrize("cid,fp32,split", [("ev-v7-4v4", "v2", "v7"), ("ev-v7static-5v5", "v2", "v7"),
                                            ("ev-sp7-4v4", "sp2", "sp7"), ("ev-sp8-3v3", "sp2", None)],
                         ids=["v7-vs-v2", "v7static-vs-v2", "sp7-vs-sp2", "sp8-vs-sp2"])
def test_eventful_split_bf16_arm_matches_fp32_arm(device, cid, fp32, split, monkeypatch):
    """As test_rollout_v7_runtime_shape_matches_v2 on eventful inputs: along the split-bf16 arm's own test-mode
    trajectory every recorded action is an available argmax of the fp32 oracle up to a 1e-5 tie, and the arm
    reproduces the fp32 arm's episodes bit for bit except where a near tie flips an argmax."""
    c = _case(cid, monkeypatch)
    stepper, macs, args, _ = _build(device, c)
    ref, L_ref, arm32 = _test_run(stepper, device, fp32, monkeypatch)
    got, L, arm16 = _test_run(stepper, device, split, monkeypatch)
    assert (arm32, arm16) == (fp32, c.arm)
    qs, worst = [], 0.0
    for mac, nb in zip(macs, got):
        q = oracle_q(mac, {k: torch.from_numpy(v) for k, v in nb.items()}, args.n_agents, nb["obs"].shape[1])
        qs.append(q)
        av = nb["avail_actions"].astype(bool)
        for b in range(ES.B):
            for t in range(int(L[b]) + 1):
                qm = np.where(av[b, t], q[b, t], -np.inf)
                chosen = np.take_along_axis(qm, nb["actions"][b, t], axis=-1)[:, 0]
                assert np.isfinite(chosen).all(), (b, t)
                worst = max(worst, float((qm.max(axis=-1) - chosen).max()))
    assert worst <= 1e-5, worst
    n_diff = assert_near_tie_divergence(ref, got, qs, ES.B)
    print(f"{cid}: {arm16} vs {arm32}: {n_diff} of {ES.B} episodes diverge (near-tie flips), allowance "
          f"{MAX_DIVERGING[cid]}; early-ending envs {int((L < c.limit).sum())} / {int((L_ref < c.limit).sum())}")
    assert int((L < c.limit).sum()) >= 2
    assert n_diff <= MAX_DIVERGING[cid], n_diff
