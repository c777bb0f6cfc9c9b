"""Self-play steppers (API of src/steppers/self_play_parallel_stepper.py:14-201 and
src/steppers/self_play_stepper.py:9-147).

Both plan teams are policy-controlled: the home MAC acts for the first team, a frozen away MAC for the
second (the reference hands the opponent's actions to the env as ``cat(home, away)``,
self_play_parallel_stepper.py:108). One launch of ``mlg_rollout_selfplay`` runs the whole batched
episode with both policies: each side's agents use their own weights and epsilon and are recorded into
their own EpisodeBatch (obs / avail of that side's agents, the shared global state, ``reward[0]`` for
home and ``reward[1]`` for away; stepper_utils.build_pre_transition_data, stepper_utils.py:4-24).
``run()`` returns ``(home_batch, away_batch, env_infos)`` like the reference.

Opponent mixture (``set_opponent_mix``): one launch of ``mlg_rollout_selfplay_mix`` plays the home policy against one
away policy -- and one roster -- per group of 16 envs; env b runs exactly as in the plain launch against its group's
opponent.

Two ``pi_logits`` MACs (COMA in self-play and the league): ``SelfPlayPolicyParallelStepper`` / ``SelfPlayPolicyStepper``
(``SELF_POLICY_REGISTRY``) make the same run with one launch of ``mlg_rollout_selfplay_policy``: each side's outputs go
through the policy softmax with that side's epsilon floor and the action is drawn by the multinomial rule.

Two ``DistinctMAC``s (mac: distinct, one DRQN per agent slot on both sides): ``SelfPlayDistinctParallelStepper`` /
``SelfPlayDistinctStepper`` (``SELF_DISTINCT_REGISTRY``) make the same run with one launch of
``mlg_rollout_selfplay_distinct``: agent ln of side s acts with network ln of side s's MAC.

Two feed-forward MACs (agent: dqn on both sides): ``SelfPlayFFParallelStepper`` / ``SelfPlayFFStepper``
(``SELF_FF_REGISTRY``) make the same run with one launch of ``mlg_rollout_selfplay_ff``: selection is epsilon-greedy over
Q values as in SelfPlayParallelStepper, and no hidden state is carried.

Two ``EntityMAC``s (REFIL, attn_qmix, attn_vdn: ``entity_scheme``): ``SelfPlayEntityParallelStepper`` /
``SelfPlayEntityStepper`` (``SELF_ENTITY_REGISTRY``) run the two-policy entity env (DESIGN.md §3b') with one launch of
``mlg_refil_rollout_selfplay``: both batches are entity batches, the away one in the canonical view, so a network
trained as home plays away unchanged.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from .. import _native
from ..components.batch_view import mlg_entity_batch
from ..components.replay_buffer import RingEpisodeBatch
from ..controllers.distinct_controller import DistinctMAC
from ..controllers.entity_controller import EntityMAC
from ..envs.entity_env import EntityEnvSpec
from ..envs.teams_env import _enum_name, load_match_build_plan
from ..exceptions import MultiAgentControllerNotInitialized
from ..modules.agents import DQNAgentNetwork, DRQNAgentNetwork
from .parallel_stepper import LazyEnvInfos, ParallelStepper


GROUP_ENVS = 16  # envs per mixture group (one rollout workgroup)


@dataclass
class OpponentMix:
    """The away side of a mixture launch. ``rows``: float32 [K, n_params] device tensor of flat agent parameters
    (named_parameters() order, any row stride; read when the mix is set). ``group_opponent``: int [G] row of ``rows``
    for each group of 16 envs, G = ceil(B / 16). ``plans``: optionally one match_build_plan per opponent (K of them):
    group g then plays under ``plans[group_opponent[g]]``; None: every group plays the stepper's current plan."""
    rows: torch.Tensor
    group_opponent: Sequence[int]
    plans: Optional[Sequence] = None


def n_groups(batch_size: int) -> int:
    return (int(batch_size) + GROUP_ENVS - 1) // GROUP_ENVS


class SelfPlayParallelStepper(ParallelStepper):
    # zero-copy run summaries as ParallelStepper: the league's record_runs kernel reads each run's wins straight from
    # the pinned summary slot (LeagueInstance.play -> last_run_info)
    _SELFPLAY = True

    def __init__(self, args, logger, log_start_t=0):
        super().__init__(args, logger, log_start_t)
        if self.spec.n_policy_teams != 2 or self.spec.n_agents % 2:
            raise ValueError(f"A total of {self.spec.n_agents} agents in the env do not fit in the symmetric "
                             "two-team scenario. Ensure the Self-Play scenario has two teams set to is_scripted=False")
        self.away_batch = None
        self._away_buf = None
        self._mix = None  # set_opponent_mix: the packed pool and the group / spec tables of the mixture launches

    def set_opponent_mix(self, mix: Optional[OpponentMix]):
        """Play the next runs against a mixture of frozen opponents, one per group of 16 envs (None: back to the away
        MAC's own parameters and the plain launch). The rows are packed here (mlg_pack_agent_pool), so later changes
        of ``mix.rows`` do not reach the launches. The away MAC still gives the architecture and the away epsilon."""
        if mix is None:
            self._mix = None
            return
        if self.home_mac is None or self.away_mac is None:
            raise MultiAgentControllerNotInitialized()
        rows = mix.rows
        if rows.dim() != 2 or rows.dtype != torch.float32 or not rows.is_cuda or \
                (rows.shape[0] > 1 and rows.stride(1) != 1) or rows.shape[0] < 1:
            raise ValueError("set_opponent_mix: rows must be float32 [K >= 1, n_params] on the device with contiguous "
                             f"rows, got {rows.dtype} {tuple(rows.shape)} on {rows.device}")
        K, G = int(rows.shape[0]), n_groups(self.batch_size)
        table = [int(k) for k in mix.group_opponent]
        if len(table) != G:
            raise ValueError(f"set_opponent_mix: group_opponent has {len(table)} entries, {self.batch_size} envs are "
                             f"{G} groups of {GROUP_ENVS}")
        if any(k < 0 or k >= K for k in table):
            raise ValueError(f"set_opponent_mix: group_opponent entries must be rows of the [{K}, n_params] pool")
        dims = self.away_mac.agent.dims()
        n_params = sum(p.numel() for p in self.away_mac.agent.parameters())
        if int(rows.shape[1]) != n_params:
            raise ValueError(f"set_opponent_mix: rows of {int(rows.shape[1])} floats for an agent of {n_params}")
        plans = list(mix.plans) if mix.plans is not None else None
        if plans is not None and len(plans) != K:
            raise ValueError(f"set_opponent_mix: {len(plans)} plans for {K} opponents (one per opponent)")
        lib = _native.load(require_gpu=True)
        psize = int(lib.mlg_packed_agent_size(_native.byref(dims)))
        if psize < 0:
            raise _native.NativeError(lib.mlg_last_error().decode())
        packed = torch.empty(K * psize, dtype=torch.float32, device=self.device)
        _native.call("mlg_pack_agent_pool", _native.byref(dims), rows.data_ptr(), int(rows.stride(0)), K,
                     packed.data_ptr(), _native.stream_ptr(self.device))
        groups = (_native.MlgMixGroup * G)(*[_native.MlgMixGroup(k, k if plans is not None else 0) for k in table])
        m = {"packed": packed, "K": K, "G": G, "groups": groups, "table": table,
             "dev_groups": torch.frombuffer(bytearray(bytes(groups)), dtype=torch.uint8).to(self.device),
             "specs": [self._spec_of_plan(p)[1] for p in plans] if plans is not None else None}
        self._mix = m
        self._mix_specs()

    def _mix_specs(self):
        """The spec array of the mixture (host + device copy): the opponents' plans, else the stepper's current spec
        (rebuilt when set_match_build_plan swapped it since)."""
        m = self._mix
        if m.get("cspecs") is not None and (m["specs"] is not None or m["spec_src"] is self._cspec):
            return
        cs = [s.to_c() for s in m["specs"]] if m["specs"] is not None else [self._cspec]
        m["cspecs"] = (_native.MlgEnvSpec * len(cs))(*cs)
        m["dev_specs"] = torch.frombuffer(bytearray(bytes(m["cspecs"])), dtype=torch.uint8).to(self.device)
        m["spec_src"] = self._cspec

    def describe_rollout(self):
        if self._mix is not None:
            if self.home_mac is None:
                raise MultiAgentControllerNotInitialized()
            return _native.rollout_selfplay_mix_describe(self._cspec, self.home_mac.agent.dims())
        return super().describe_rollout()

    def initialize(self, scheme, groups, preprocess, home_mac, away_mac=None):
        if away_mac is None:
            raise ValueError("self-play needs an away MAC (initialize(..., home_mac, away_mac))")
        for side, mac in (("home", home_mac), ("away", away_mac)):
            if isinstance(mac, DistinctMAC):
                raise NotImplementedError(f"{type(self).__name__} does not support mac='distinct' (one network per "
                                          f"agent slot; the {side} MAC): it drives parameter-shared MACs (mac='basic') "
                                          "only. Two DistinctMACs are SelfPlayDistinctParallelStepper, "
                                          "steppers.SELF_DISTINCT_REGISTRY['parallel']")
            self._check_output_type(side, mac)
            agent = getattr(mac, "agent", None)
            if agent is not None and not isinstance(agent, DRQNAgentNetwork):
                raise NotImplementedError(f"self-play rollouts run the recurrent agent (agent='rnn') only: the {side} "
                                          f"MAC's {type(agent).__name__} is not supported (agent='dqn' and the other "
                                          "non-DRQN agents in self-play are out of scope)")
        ParallelStepper.initialize(self, scheme, groups, preprocess, home_mac)
        self.away_mac = away_mac
        self._away_buf = None

    def _check_output_type(self, side, mac):
        if getattr(mac, "agent_output_type", "q") != "q":
            raise NotImplementedError(f"self-play rollouts select epsilon-greedy over Q values: the {side} MAC's "
                                      f"agent_output_type={mac.agent_output_type!r} is not supported (COMA in "
                                      "self-play is out of scope for SelfPlayParallelStepper; two pi_logits MACs are "
                                      "SelfPlayPolicyParallelStepper, steppers.SELF_POLICY_REGISTRY['parallel'])")

    @property
    def epsilons(self):
        return (getattr(self.home_mac.action_selector, "epsilon", None),
                getattr(self.away_mac.action_selector, "epsilon", None))

    def _epsilon_of(self, mac, test_mode):
        return self._epsilon(mac, test_mode)

    def run(self, test_mode=False):
        if self.home_mac is None or self.away_mac is None:
            raise MultiAgentControllerNotInitialized()
        self.reset()
        self.logger.test_mode = test_mode
        self.home_mac.init_hidden(batch_size=self.batch_size)
        self.away_mac.init_hidden(batch_size=self.batch_size)
        eps_h = self._epsilon_of(self.home_mac, test_mode)
        eps_a = self._epsilon_of(self.away_mac, test_mode)
        keep = []
        ring = self._ring if not test_mode else None
        if ring is not None and ring.has_outstanding():
            # the previous train-mode run's episodes still occupy the ring's next slots (not inserted yet):
            # this run goes to a fresh batch, as in the reference, which leaves the buffer untouched until insert
            ring = None
        if ring is not None:
            slot0 = ring.buffer_index
            mb_h, k = self._to_mlg(ring)
            keep.append(k)
            mb_h.B, mb_h.ring_slot0, mb_h.ring_size, mb_h.full_write = self.batch_size, slot0, ring.buffer_size, 1
            mb_h.slot_extent = ring.extent_ptr()
            self.home_batch = RingEpisodeBatch(ring, slot0, self.batch_size)
        else:
            self.home_batch = self.new_batch_fn()
            mb_h, k = self._to_mlg(self.home_batch)
            keep.append(k)
        if getattr(self.args, "reuse_away_batch", True):
            # one away batch, rewritten in full-write mode by every run (every byte of its B slots is stored,
            # zeros past each episode's end): no per-run allocation and ~1 GB zero fill. The batch returned by
            # run k is therefore overwritten by run k + 1; reuse_away_batch=False gives the reference's fresh
            # batch per run (self_play_parallel_stepper.py:95).
            if self._away_buf is None:
                self._away_buf = self.new_batch_fn()
                # rows of each slot that may be non-zero (T1 = unknown): later runs zero only what the slot's
                # previous episode wrote past the new episode's end
                self._away_extent = torch.full((self.batch_size,), self.episode_limit + 1, dtype=torch.int32,
                                               device=self.device)
            self.away_batch = self._away_buf
            mb_a, k = self._to_mlg(self.away_batch)
            mb_a.full_write = 1
            mb_a.slot_extent = self._away_extent.data_ptr()
        else:
            self.away_batch = self.new_batch_fn()
            mb_a, k = self._to_mlg(self.away_batch)
        keep.append(k)
        h_agent, a_agent = self._packers()
        d, d_a = h_agent.dims(), a_agent.dims()
        if any(getattr(d, f) != getattr(d_a, f) for f, _ in d._fields_):
            raise ValueError("home and away agents must have the same architecture")
        st = self.envs.to_c()
        run_info = self._run_info()
        p_h, p_a = h_agent.packed(), a_agent.packed()  # re-packs (parameters changed) before the timed window
        ev = None
        if self._timed_launch():
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        if self._mix is not None:
            m = self._mix
            self._mix_specs()
            cmix = _native.MlgOpponentMix(m["packed"].data_ptr(), m["K"], m["G"], m["dev_groups"].data_ptr(),
                                          ctypes.addressof(m["groups"]), m["dev_specs"].data_ptr(),
                                          ctypes.addressof(m["cspecs"]), len(m["cspecs"]))
            _native.call("mlg_rollout_selfplay_mix", _native.byref(self._cspec), _native.byref(st), _native.byref(d),
                         _native.ptr(p_h), _native.byref(cmix), _native.byref(mb_h), _native.byref(mb_a),
                         _native.byref(run_info), float(eps_h), float(eps_a), int(bool(test_mode)),
                         _native.stream_ptr(self.device))
        else:
            self._launch_selfplay(st, d, p_h, p_a, mb_h, mb_a, run_info, eps_h, eps_a, test_mode)
        if ev is not None:
            ev[1].record()
            self.timing.append(ev)
            self._last_end_ev = ev[1]
        del keep
        self._queue_summary(test_mode)
        self._finish_post()
        return self.home_batch, self.away_batch, LazyEnvInfos(self, self._run_id)


    def _packers(self):
        """What gives each side's dims() and packed() weights: the shared agent network."""
        return self.home_mac.agent, self.away_mac.agent

    def _launch_selfplay(self, st, d, p_h, p_a, mb_h, mb_a, run_info, eps_h, eps_a, test_mode):
        _native.call("mlg_rollout_selfplay", _native.byref(self._cspec), _native.byref(st), _native.byref(d),
                     _native.ptr(p_h), _native.ptr(p_a), _native.byref(mb_h),
                     _native.byref(mb_a), _native.byref(run_info), float(eps_h), float(eps_a),
                     int(bool(test_mode)), _native.stream_ptr(self.device))


class _SingleEnv:
    """B = 1 form of a self-play stepper (self_play_stepper.py:9-147): returns the final env_info dict."""

    def __init__(self, args, logger, log_start_t=0):
        assert args.batch_size_run == 1
        super().__init__(args, logger, log_start_t)

    def run(self, test_mode=False):
        home, away, infos = super().run(test_mode)
        eh, ea = self.epsilons
        self.logger.log_stat("home_epsilon", eh, self.log_t)
        self.logger.log_stat("away_epsilon", ea, self.log_t)
        return home, away, infos[-1]


class SelfPlayStepper(_SingleEnv, SelfPlayParallelStepper):
    """Single-env self-play stepper (self_play_stepper.py:9-147): B = 1, returns the final env_info dict."""


class SelfPlayPolicyParallelStepper(SelfPlayParallelStepper):
    """Self-play of two ``pi_logits`` MACs (COMA; in the reference the self-play steppers only call
    ``mac.select_actions``, so they run any registered algorithm): one launch of ``mlg_rollout_selfplay_policy`` per
    run. Each side's epsilon floor comes from its own selector's schedule, ``mask_before_softmax`` / ``test_greedy``
    from args (one value for both sides). Batches, rewards, run summary and ring / away-batch reuse are
    SelfPlayParallelStepper's."""

    def _check_output_type(self, side, mac):
        if getattr(mac, "agent_output_type", "q") != "pi_logits":
            raise NotImplementedError(f"policy self-play rollouts draw from the policy softmax: the {side} MAC's "
                                      f"agent_output_type={getattr(mac, 'agent_output_type', 'q')!r} is not supported "
                                      "(both MACs must be 'pi_logits'; one Q side against one policy side is out of "
                                      "scope, two Q MACs are steppers.SELF_REGISTRY)")

    def set_opponent_mix(self, mix):
        if mix is None:
            return
        raise NotImplementedError("opponent mixtures with agent_output_type='pi_logits' are not supported "
                                  "(mlg_rollout_selfplay_mix selects epsilon-greedy over Q values; a pi_logits match "
                                  "plays one opponent)")

    def describe_rollout(self):
        if self.home_mac is None:
            raise MultiAgentControllerNotInitialized()
        return _native.rollout_selfplay_policy_describe(self._cspec, self.home_mac.agent.dims())

    def _launch_selfplay(self, st, d, p_h, p_a, mb_h, mb_a, run_info, eps_h, eps_a, test_mode):
        a = self.args
        sel = self.home_mac.action_selector
        _native.call("mlg_rollout_selfplay_policy", _native.byref(self._cspec), _native.byref(st), _native.byref(d),
                     _native.ptr(p_h), _native.ptr(p_a), _native.byref(mb_h), _native.byref(mb_a),
                     _native.byref(run_info), float(eps_h), float(eps_a), int(bool(test_mode)),
                     int(bool(getattr(a, "mask_before_softmax", True))),
                     int(bool(getattr(a, "test_greedy", getattr(sel, "test_greedy", True)))),
                     _native.stream_ptr(self.device))


class SelfPlayPolicyStepper(_SingleEnv, SelfPlayPolicyParallelStepper):
    """Single-env form of SelfPlayPolicyParallelStepper: B = 1, returns the final env_info dict."""


class SelfPlayDistinctParallelStepper(SelfPlayParallelStepper):
    """Self-play of two ``DistinctMAC``s (mac: distinct): one launch of ``mlg_rollout_selfplay_distinct`` per run, agent
    ln of side s acting with network ln of side s's packed pool (``DistinctMAC.packed()``). Selection is
    SelfPlayParallelStepper's (epsilon-greedy over Q values, one epsilon per side, the same counter-RNG streams), and so
    are the batches, rewards, run summary and ring / away-batch reuse."""

    def initialize(self, scheme, groups, preprocess, home_mac, away_mac=None):
        if away_mac is None:
            raise ValueError("self-play needs an away MAC (initialize(..., home_mac, away_mac))")
        for side, mac in (("home", home_mac), ("away", away_mac)):
            if not isinstance(mac, DistinctMAC):
                raise NotImplementedError(f"{type(self).__name__} drives two DistinctMACs (mac='distinct'): the {side} "
                                          f"MAC is a {type(mac).__name__} (a distinct side against a parameter-shared "
                                          "side is out of scope; two parameter-shared MACs are steppers.SELF_REGISTRY)")
        d, d_a = home_mac.dims(), away_mac.dims()
        if any(getattr(d, f) != getattr(d_a, f) for f, _ in d._fields_):
            raise ValueError("home and away DistinctMACs must have the same architecture (equal agent dims)")
        ParallelStepper.initialize(self, scheme, groups, preprocess, home_mac)
        self.away_mac = away_mac
        self._away_buf = None

    def set_opponent_mix(self, mix):
        if mix is None:
            return
        raise NotImplementedError("opponent mixtures with mac='distinct' are not supported (mlg_rollout_selfplay_mix "
                                  "reads one parameter-shared network per opponent; a match of DistinctMACs plays one "
                                  "opponent)")

    def describe_rollout(self):
        if self.home_mac is None:
            raise MultiAgentControllerNotInitialized()
        return _native.rollout_selfplay_distinct_describe(self._cspec, self.home_mac.dims())

    def _packers(self):
        return self.home_mac, self.away_mac  # a DistinctMAC has dims() and packed() itself (the pool of N networks)

    def _launch_selfplay(self, st, d, p_h, p_a, mb_h, mb_a, run_info, eps_h, eps_a, test_mode):
        _native.call("mlg_rollout_selfplay_distinct", _native.byref(self._cspec), _native.byref(st), _native.byref(d),
                     _native.ptr(p_h), _native.ptr(p_a), _native.byref(mb_h), _native.byref(mb_a),
                     _native.byref(run_info), float(eps_h), float(eps_a), int(bool(test_mode)),
                     _native.stream_ptr(self.device))


class SelfPlayDistinctStepper(_SingleEnv, SelfPlayDistinctParallelStepper):
    """Single-env form of SelfPlayDistinctParallelStepper: B = 1, returns the final env_info dict."""


class SelfPlayFFParallelStepper(SelfPlayParallelStepper):
    """Self-play of two feed-forward MACs (agent: dqn, ``DQNAgentNetwork`` on both sides): one launch of
    ``mlg_rollout_selfplay_ff`` per run. Selection is SelfPlayParallelStepper's (epsilon-greedy over Q values, one
    epsilon per side, the same counter-RNG streams), and so are the batches, rewards, run summary and ring / away-batch
    reuse; ``init_hidden`` of a feed-forward MAC holds nothing the launch reads."""

    def initialize(self, scheme, groups, preprocess, home_mac, away_mac=None):
        if away_mac is None:
            raise ValueError("self-play needs an away MAC (initialize(..., home_mac, away_mac))")
        for side, mac in (("home", home_mac), ("away", away_mac)):
            if isinstance(mac, DistinctMAC):
                raise NotImplementedError(f"{type(self).__name__} does not support mac='distinct' (the {side} MAC): "
                                          "agent='dqn' under mac='distinct' is out of scope; two DistinctMACs of "
                                          "recurrent networks are SelfPlayDistinctParallelStepper, "
                                          "steppers.SELF_DISTINCT_REGISTRY['parallel']")
            if getattr(mac, "agent_output_type", "q") != "q":
                raise NotImplementedError(f"{type(self).__name__} selects epsilon-greedy over Q values: the {side} "
                                          f"MAC's agent_output_type={mac.agent_output_type!r} is not supported (COMA "
                                          "over agent='dqn' is out of scope; two recurrent pi_logits MACs are "
                                          "SelfPlayPolicyParallelStepper, steppers.SELF_POLICY_REGISTRY['parallel'])")
            agent = getattr(mac, "agent", None)
            if isinstance(agent, DRQNAgentNetwork):
                raise NotImplementedError(f"{type(self).__name__} drives two feed-forward MACs (agent='dqn'): the "
                                          f"{side} MAC's agent is a DRQNAgentNetwork (a feed-forward side against a "
                                          "recurrent side is out of scope; two recurrent MACs are "
                                          "SelfPlayParallelStepper, steppers.SELF_REGISTRY['parallel'])")
            if not isinstance(agent, DQNAgentNetwork):
                raise NotImplementedError(f"{type(self).__name__} drives two feed-forward MACs (agent='dqn'): the "
                                          f"{side} MAC's {type(agent).__name__} is not supported")
        ParallelStepper.initialize(self, scheme, groups, preprocess, home_mac)
        self.away_mac = away_mac
        self._away_buf = None

    def set_opponent_mix(self, mix):
        if mix is None:
            return
        raise NotImplementedError("opponent mixtures with agent='dqn' are not supported (mlg_rollout_selfplay_mix packs "
                                  "and reads DRQN blocks; a match of feed-forward MACs plays one opponent)")

    def describe_rollout(self):
        if self.home_mac is None:
            raise MultiAgentControllerNotInitialized()
        return _native.rollout_selfplay_ff_describe(self._cspec, self.home_mac.agent.dims())

    def _launch_selfplay(self, st, d, p_h, p_a, mb_h, mb_a, run_info, eps_h, eps_a, test_mode):
        _native.call("mlg_rollout_selfplay_ff", _native.byref(self._cspec), _native.byref(st), _native.byref(d),
                     _native.ptr(p_h), _native.ptr(p_a), _native.byref(mb_h), _native.byref(mb_a),
                     _native.byref(run_info), float(eps_h), float(eps_a), int(bool(test_mode)),
                     _native.stream_ptr(self.device))


class SelfPlayFFStepper(_SingleEnv, SelfPlayFFParallelStepper):
    """Single-env form of SelfPlayFFParallelStepper: B = 1, returns the final env_info dict."""


class SelfPlayEntityParallelStepper(SelfPlayParallelStepper):
    """Self-play of two ``EntityMAC``s over the two-policy entity env (DESIGN.md §3b'): one launch of
    ``mlg_refil_rollout_selfplay`` per run. The home batch is what EntityParallelStepper records; the away batch is the
    same run in the canonical view (own team first, x mirrored, team flipped, actions remapped) with team 1's reward.
    Selection is SelfPlayParallelStepper's (epsilon-greedy over Q values, one epsilon per side, the same counter-RNG
    streams), and so are the run summary and the ring / away-batch reuse. The entity spec has one roster for both teams
    and no opponent pool: mixtures and plans whose two teams differ are refused."""

    _batch_keys = ("entities", "obs_mask", "entity_mask", "actions", "avail_actions", "reward", "terminated",
                   "actions_onehot", "filled")

    def _build_spec(self, env_args, config_dir):
        return EntityEnvSpec.from_env_args(env_args, config_dir, self_play=True)

    def _to_mlg(self, batch):
        return mlg_entity_batch(batch)

    def initialize(self, scheme, groups, preprocess, home_mac, away_mac=None):
        if away_mac is None:
            raise ValueError("self-play needs an away MAC (initialize(..., home_mac, away_mac))")
        for side, mac in (("home", home_mac), ("away", away_mac)):
            if not isinstance(mac, EntityMAC):
                raise NotImplementedError(f"{type(self).__name__} drives two EntityMACs (mac='entity_mac'): the {side} "
                                          f"MAC is a {type(mac).__name__} (an entity side against an obs / state side "
                                          "is out of scope; two BasicMACs are steppers.SELF_REGISTRY)")
            if getattr(mac, "agent_output_type", "q") != "q":
                raise NotImplementedError(f"{type(self).__name__} selects epsilon-greedy over Q values: the {side} "
                                          f"MAC's agent_output_type={mac.agent_output_type!r} is not supported")
        d, d_a = home_mac.agent.dims(), away_mac.agent.dims()
        if any(getattr(d, f) != getattr(d_a, f) for f, _ in d._fields_):
            raise ValueError("home and away EntityMACs must have the same architecture (equal agent dims)")
        ParallelStepper.initialize(self, scheme, groups, preprocess, home_mac)
        self.away_mac = away_mac
        self._away_buf = None

    def set_opponent_mix(self, mix):
        if mix is None:
            return
        raise NotImplementedError(f"{type(self).__name__}.set_opponent_mix: opponent mixtures over entity agents are "
                                  "not supported (mlg_rollout_selfplay_mix packs DRQN blocks and reads one roster per "
                                  "opponent; the entity env spec has one roster: a match of EntityMACs plays one "
                                  "opponent)")

    def _spec_of_plan(self, plan):
        if not (isinstance(plan, str) and plan in ("refil_8",)):
            teams = load_match_build_plan(plan, getattr(self.args, "config_dir", None))
            rosters = [[(_enum_name(u["role"]), _enum_name(u.get("attack_type", "RANGED"))) for u in t["units"]]
                       for t in teams]
            if any(r != rosters[0] for r in rosters[1:]):
                raise NotImplementedError(f"{type(self).__name__}.set_match_build_plan: the plan's two teams differ "
                                          f"({rosters[0]} vs {next(r for r in rosters[1:] if r != rosters[0])}); the "
                                          "entity env spec has one roster for both teams (per-team rosters are out of "
                                          "scope)")
        return super()._spec_of_plan(plan)

    def describe_rollout(self):
        """(arm name, dynamic LDS bytes) of the launch run() would make (mlg_refil_rollout_selfplay_describe: host
        only)."""
        if self.home_mac is None:
            raise MultiAgentControllerNotInitialized()
        return _native.refil_rollout_selfplay_describe(self._cspec, self.home_mac.agent.dims())

    def _launch_selfplay(self, st, d, p_h, p_a, mb_h, mb_a, run_info, eps_h, eps_a, test_mode):
        _native.call("mlg_refil_rollout_selfplay", _native.byref(self._cspec), _native.byref(st), _native.byref(d),
                     _native.ptr(p_h), _native.ptr(p_a), _native.byref(mb_h), _native.byref(mb_a),
                     _native.byref(run_info), float(eps_h), float(eps_a), int(bool(test_mode)),
                     _native.stream_ptr(self.device))


class SelfPlayEntityStepper(_SingleEnv, SelfPlayEntityParallelStepper):
    """Single-env form of SelfPlayEntityParallelStepper: B = 1, returns the final env_info dict."""
