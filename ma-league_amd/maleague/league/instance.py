"""One league player per rank: the training loop of a league instance.

Restates the per-process loop of src/league/processes/training/matchmaking_league_instance.py:19-71 and
role_based_league_instance.py:21-53 (with LeagueExperimentInstance, league_experiment_process.py:57-105):
  1. (optional) pre-train the home policy against the mirrored scripted AI     (:21-25)
  2. share the home agent's parameters with the league                          (:26)
  3. per league iteration: get a match (matchmaker or league role), load the adversary's parameters, play
     ``iterations_per_match`` self-play training iterations recording every episode's result, share.
With ``opponents_per_match = K > 1`` a match draws K opponents and every rollout launch plays all of them, one per
contiguous block of 16-env groups (an opponent mixture, SelfPlayParallelStepper.set_opponent_mix): PFSP and the role
branch mixes are realised inside a match, the results land in K payoff cells and the replay buffer holds K opponents.
Processes, queues and the coordinator are replaced by one rank per GPU and DistributedLeague collectives.
The self-play experiment is built once per instance and its adversary swapped between matches (the
reference rebuilds LeagueExperiment -- replay buffer, optimizer state -- for every match).
``DistinctLeagueInstance`` is the same loop for ``mac: distinct`` (one network per agent slot): a player's pool row is
its N networks back to back; ``league_instance_for`` picks the class by ``args.mac``.
"""
from __future__ import annotations

import copy

import numpy as np
import torch
import torch.distributed as dist

from ..envs.plans import mirror_plan
from ..exceptions import refuse_entity_league
from ..runs import LeagueExperiment, MultiAgentExperiment
from ..runs.sp_ma_experiment import agent_vector, load_agent_vector
from .distributed import DistributedLeague
from .matchmaking import REGISTRY as matchmaking_REGISTRY
from .roles import ROLES, Historical, LeagueView, alphastar_roles
from .teams import match_plan


def group_count(batch_size: int) -> int:
    """16-env groups of a rollout launch (one workgroup, one opponent of a mixture each)."""
    return (int(batch_size) + 15) // 16


def group_assignment(K: int, G: int) -> list:
    """The draw of every group: draw j of K (clipped to G) gets the contiguous groups [floor(j G / K),
    floor((j + 1) G / K)), so every draw gets at least one group and the block sizes differ by at most one."""
    K = max(1, min(int(K), int(G)))
    out = []
    for j in range(K):
        out.extend([j] * ((j + 1) * G // K - j * G // K))
    return out


class LeagueInstance:
    """``mode``: "matchmaking" (args.matchmaking in pfsp/uniform/random/fsp/adversaries, every player a
    learner) or "rolebased" (``role`` in simple/main/main_exploiter/league_exploiter)."""

    def __init__(self, args, logger, league: DistributedLeague, mode="matchmaking", role=None, seed=0,
                 experiment=None, teams=None, opponents_per_match: int = 1):
        """``teams``: the league's Team of every player (index = pid; league.teams.compose_league_teams, one team
        per player as CentralWorker assigns them, central_worker.py:84-93). Each match then puts this player's team
        against the opponent's (a historical snapshot plays its parent's team). None: every player plays the
        env config's own plan, mirrored. ``opponents_per_match``: opponents drawn per sync() (clipped to the number
        of 16-env groups of a launch); 1 is the single-adversary match."""
        if int(opponents_per_match) < 1:
            raise ValueError(f"opponents_per_match={opponents_per_match} must be >= 1")
        self.opponents_per_match = int(opponents_per_match)
        refuse_entity_league(args, type(self).__name__)
        if self.opponents_per_match > 1 and getattr(args, "agent_output_type", "q") == "pi_logits":
            raise NotImplementedError(f"LeagueInstance(opponents_per_match={self.opponents_per_match}): opponent "
                                      "mixtures with agent_output_type='pi_logits' are not supported (a pi_logits "
                                      "match plays one opponent)")
        if self.opponents_per_match > 1 and getattr(args, "agent", "rnn") == "dqn":
            raise NotImplementedError(f"LeagueInstance(opponents_per_match={self.opponents_per_match}): opponent "
                                      "mixtures with agent='dqn' are not supported (mlg_rollout_selfplay_mix packs "
                                      "DRQN blocks; a match of feed-forward agents plays one opponent)")
        self.opponents = []      # the draws of the current match (pids; equal draws repeat)
        self.group_draw = None   # mixture match: the draw (index into opponents) of every 16-env group
        self._check_mac(args)
        self.args, self.logger, self.league = args, logger, league
        self.pid = league.player()
        self.mode = mode
        if teams is not None and len(teams) != league.n:
            raise ValueError(f"{len(teams)} teams for a league of {league.n} players (one team per player)")
        self.teams = list(teams) if teams is not None else None
        self.home_team = self.teams[self.pid] if self.teams is not None else None
        self.away_team = None
        self.away_teams = []  # the away roster (codes) of every match, in order
        rng = np.random.RandomState(seed * 1000 + self.pid)
        if mode == "rolebased":
            roles = role if isinstance(role, (list, tuple)) else [role or "simple"] * league.n
            kw = dict(checkpoint_min_steps=float(getattr(args, "league_checkpoint_min_steps", 2e9)),
                      checkpoint_max_steps=float(getattr(args, "league_checkpoint_max_steps", 4e9)))
            # every rank holds the full player table (roles are needed by the others' matchmaking)
            self.players = [ROLES[r](pid, np.random.RandomState(seed * 1000 + pid), **kw) for pid, r in enumerate(roles)]
            self.me = self.players[self.pid]
            self.matchmaker = None
        else:
            self.players = [ROLES["simple"](pid) for pid in range(league.n)]
            self.me = self.players[self.pid]
            self.matchmaker = matchmaking_REGISTRY[getattr(args, "matchmaking", "pfsp")](
                rng, record_match=league.record_match)
        if experiment is None:
            sp_args = copy.deepcopy(args)
            sp_args.env_args = dict(args.env_args)
            sp_args.env_args["match_build_plan"] = self._plan(ai=False)
            experiment = LeagueExperiment(sp_args, logger)
            experiment._init_stepper()
        self.experiment = experiment
        self.opponent = None
        self.history = []  # (league iteration, opponent pid, historical?)
        self.episode = 0

    def _check_mac(self, args):
        if getattr(args, "mac", "basic") == "distinct":
            raise NotImplementedError("LeagueInstance shares one parameter-shared agent per player with the league: "
                                      "mac='distinct' is not supported here (a league over distinct MACs is "
                                      "DistinctLeagueInstance, league.instance.league_instance_for)")

    def _counter_agent(self, mac):
        """The network whose trained-steps counter is this player's."""
        return mac.agent

    def _agent_state(self, mac):
        """What load_home_agent takes from a pre-trained MAC."""
        return mac.agent.state_dict()

    def _plan(self, ai: bool):
        """The home team mirrored (league_experiment_process.py:57-62 with away=None): this player's league team,
        or the env config's own plan when the league has no team compositions."""
        if self.home_team is not None:
            return match_plan(self.home_team, ai=ai)
        return mirror_plan(self.args.env_args["match_build_plan"], ai=ai, config_dir=getattr(self.args, "config_dir", None))

    def team_of(self, pid: int):
        """The Team a league pid plays: a player's own, a historical snapshot its parent's (None without teams)."""
        if self.teams is None:
            return None
        if pid < self.league.n:
            return self.teams[pid]
        parents = [p for h, p, _ in self.league.historical_meta if h == pid]
        if not parents:
            raise KeyError(f"league pid {pid} is neither a player nor a stored historical snapshot")
        return self.teams[parents[0]]

    # ---- phases -------------------------------------------------------------------------------------------
    def pretrain_vs_ai(self, iterations: int = 0, play_time_seconds: float = None):
        """matchmaking_league_instance.py:21-25: initial play against the mirrored scripted AI, for ``iterations``
        training iterations or ``play_time_seconds`` of wall time (the reference's play_time_mins)."""
        if iterations <= 0 and not play_time_seconds:
            return
        ai_args = copy.deepcopy(self.args)
        ai_args.env_args = dict(self.args.env_args)
        ai_args.env_args["match_build_plan"] = self._plan(ai=True)
        exp = MultiAgentExperiment(ai_args, self.logger)
        load_agent_vector(exp.home_mac, agent_vector(self.experiment.home_mac))
        if play_time_seconds:
            exp.start(play_time_seconds=play_time_seconds)
        else:
            exp.start(max_iterations=iterations)
        self.experiment.load_home_agent(self._agent_state(exp.home_mac))
        del exp

    def view(self) -> LeagueView:
        hist = [Historical(pid, parent, steps) for pid, parent, steps in self.league.historical_meta]
        # the host copy of this league iteration's payoff (DistributedLeague.host_snapshot) when there is one
        pay = self.league.payoff_host if self.league.payoff_host is not None else self.league.payoff
        return LeagueView(pay, self.players, hist)

    def sync(self):
        """League iteration boundary: payoff all_reduce, parameter / checkpoint all_gather, barrier, next match.
        Returns (opponent pid, historical?) or None when the matchmaker ends the league for this player."""
        home = self.experiment.home_mac
        self.league.sync_payoff()
        # payoff + this player's trained steps in one device -> host read (matchmaking then runs on the host copy)
        agent = self._counter_agent(home)
        counter = agent.trained_counter(self.league.device) if hasattr(agent, "trained_counter") else None
        dev_steps = self.league.host_snapshot(counter)
        steps = agent.trained_steps_with(dev_steps) if counter is not None else int(agent.trained_steps)
        self.me.trained_steps = steps
        ckpt = self.me.ready_to_checkpoint(self.view()) if self.mode == "rolebased" else False
        taken = self.league.exchange(agent_vector(home), steps, ckpt)
        if ckpt and any(parent == self.pid for _, parent in taken):
            self.me.checkpoint()  # only when the snapshot exists (max_historical > 0): otherwise it asks again
        self.league.barrier()
        view = self.view()
        K = 1 if self.opponents_per_match == 1 else \
            min(self.opponents_per_match, group_count(self.experiment.stepper.batch_size))
        if K > 1:
            return self._sync_mix(view, K)
        if self.matchmaker is not None:
            opp, hist = self.matchmaker.get_match(self.pid, view), False
        else:
            opp, hist = self.me.get_match(view)
            self.league.record_match(self.pid, opp)
        # the league ends for everybody once one player has no match left (keeps the collectives aligned)
        if self._any(opp is None):
            return None
        self.opponent = int(opp)
        self.opponents, self.group_draw = [self.opponent], None
        self.experiment.load_adversary_vector(self.league.params_of(self.opponent))
        if self.teams is not None:  # the adversary's roster (matchmaking_league_instance.py:52, :61-62)
            self.away_team = self.team_of(self.opponent)
            self.away_teams.append(self.away_team.codes())
            self.experiment.configure_match(self.home_team, self.away_team)
        self.history.append((len(self.history), self.opponent, bool(hist)))
        return self.opponent, hist

    def _sync_mix(self, view, K: int):
        """The match of sync() with K > 1 draws: K calls of the matchmaker (or of the role's get_match), one
        record_match per draw, draw j on the contiguous groups [floor(j G / K), floor((j + 1) G / K)). Equal draws
        share a payoff column. With teams every opponent plays ``team_of(pid)``'s roster."""
        draws = []
        for _ in range(K):
            if self.matchmaker is not None:
                opp, hist = self.matchmaker.get_match(self.pid, view), False
            else:
                opp, hist = self.me.get_match(view)
                if opp is not None:
                    self.league.record_match(self.pid, opp)
            draws.append((opp, bool(hist)))
        # the league ends for everybody once one player has no match left (keeps the collectives aligned)
        if self._any(any(opp is None for opp, _ in draws)):
            return None
        self.opponents = [int(opp) for opp, _ in draws]
        self.opponent = self.opponents[0]
        self.group_draw = group_assignment(K, group_count(self.experiment.stepper.batch_size))
        # the away MAC keeps a real opponent (architecture check, away epsilon); the launches read the pool rows
        self.experiment.load_adversary_vector(self.league.params_of(self.opponent))
        rows = torch.stack([self.league.params_of(o) for o in self.opponents])
        if self.teams is not None:
            aways = [self.team_of(o) for o in self.opponents]
            self.away_team = aways[0]
            self.away_teams.extend(t.codes() for t in aways)
            self.experiment.configure_match(self.home_team, self.away_team)
            self.experiment.load_adversary_mix(rows, self.group_draw, teams=aways, home=self.home_team)
        else:
            self.experiment.load_adversary_mix(rows, self.group_draw)
        for opp, hist in draws:
            self.history.append((len(self.history), int(opp), hist))
        return self.opponent, draws[0][1]

    def _any(self, flag: bool) -> bool:
        if not self.league._dist:
            return bool(flag)
        t = torch.tensor([1.0 if flag else 0.0],
                         device="cpu" if dist.get_backend() == "gloo" else self.league.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return bool(t.item() > 0)

    def play(self, iterations: int):
        """Self-play training iterations against the current opponent, every episode's result recorded into
        the local payoff delta on the device (league_experiment_process.py:96-105 via on_episode_end)."""
        exp, st = self.experiment, self.experiment.stepper
        B = st.batch_size
        for _ in range(iterations):
            exp._train_episode(self.episode)
            info = st.last_run_info() if hasattr(st, "last_run_info") else st._info
            if self.group_draw is not None:  # mixture match: every env books into its group's opponent
                self.league.record_runs_mix(self.pid, self.opponents, self.group_draw, info[B:3 * B].view(B, 2),
                                            info[3 * B:4 * B])
            else:
                self.league.record_runs(self.pid, self.opponent, info[B:3 * B].view(B, 2), info[3 * B:4 * B])
            self.episode += B

    def play_for(self, seconds: float, max_iterations: int = None) -> int:
        """A match of ``seconds`` wall time (the reference's ``start(play_time_seconds=play_time_mins * 60)``,
        matchmaking_league_instance.py:64): training iterations until the time is up (at least one), or
        ``max_iterations``. Returns the iterations played. Ranks play their matches independently; they meet
        again at the next sync()."""
        import time
        t0, n = time.perf_counter(), 0
        while n == 0 or (time.perf_counter() - t0 < seconds and (max_iterations is None or n < max_iterations)):
            self.play(1)
            n += 1
        return n

    def evaluate_pool(self, episodes: int, pids=None):
        """Cross-play evaluation of the league's pool (league.evaluation): every player and stored historical snapshot
        (or ``pids``) as home against every one of them as away, greedy, ``episodes`` games per pair, each side with
        the roster ``team_of`` gives it, all pairs of this rank in one launch. With a process group rank r plays
        ``pairs[r::world]`` and the per-cell totals are summed over the ranks (host-staged under gloo, as
        sync_payoff). Returns the CrossPlayResult (rows / columns in ``pids`` order) and logs
        ``league_eval_win_rate_mean`` per home pid. The training payoff is not touched."""
        from .evaluation import CrossPlayResult, build_pairs, evaluator_for
        lg = self.league
        if lg.current is None:
            raise RuntimeError("evaluate_pool: the league's agent pool is empty (no exchange yet)")
        if pids is None:
            pids = list(range(lg.n)) + sorted(h for h, _, _ in lg.historical_meta)
        pids = [int(p) for p in pids]
        known = set(range(lg.n)) | {h for h, _, _ in lg.historical_meta}
        if not set(pids) <= known:
            raise KeyError(f"evaluate_pool: pids {sorted(set(pids) - known)} are neither players nor stored snapshots")
        # a pid is its row in [current | historical] (params_of)
        table = build_pairs(pids, pids, self.team_of if self.teams is not None else None)
        if getattr(self, "_evaluator", None) is None:
            self._evaluator = evaluator_for(self.experiment.args, lg.device)  # by agent_output_type
        mine = table[lg.rank::lg.world] if lg._dist else table
        totals = self._evaluator.evaluate([lg.current, lg.historical], mine, episodes).totals
        if lg._dist:
            if lg._host_staged() or lg.device.type != "cuda":
                dist.all_reduce(totals, op=dist.ReduceOp.SUM)
            else:
                dev = totals.to(lg.device)
                dist.all_reduce(dev, op=dist.ReduceOp.SUM)
                totals = dev.cpu()
        result = CrossPlayResult(totals)
        for r, pid in enumerate(pids):
            self.logger.log_stat("league_eval_win_rate_mean", float(result.win_rate[r].mean()), pid)
        return result

    def run(self, league_iterations: int, iterations_per_match: int, pretrain_iterations: int = 0):
        self.pretrain_vs_ai(pretrain_iterations)
        for _ in range(league_iterations):
            if self.sync() is None:
                break
            self.play(iterations_per_match)
        self.league.sync_payoff()
        return self.history


class DistinctLeagueInstance(LeagueInstance):
    """LeagueInstance for ``mac: distinct``: every player is a DistinctMAC (one DRQN per agent slot -- the league's
    heterogeneous rosters are the case for it), its pool row the N networks back to back, agent 0 first, each in
    named_parameters() order (``N x n_params`` floats: agent_vector / load_agent_vector). Matches run through
    SelfPlayDistinctParallelStepper (one mlg_rollout_selfplay_distinct launch per run), the home side trains in the
    fused learner (cfg.distinct = 1) and evaluate_pool plays DistinctCrossPlayEvaluator. One opponent per match."""

    def __init__(self, args, logger, league: DistributedLeague, mode="matchmaking", role=None, seed=0,
                 experiment=None, teams=None, opponents_per_match: int = 1):
        if int(opponents_per_match) > 1:
            raise NotImplementedError(f"DistinctLeagueInstance(opponents_per_match={opponents_per_match}): opponent "
                                      "mixtures with mac='distinct' are not supported (a match of DistinctMACs plays "
                                      "one opponent)")
        super().__init__(args, logger, league, mode=mode, role=role, seed=seed, experiment=experiment, teams=teams,
                         opponents_per_match=opponents_per_match)

    def _check_mac(self, args):
        if getattr(args, "mac", "basic") != "distinct":
            raise NotImplementedError(f"DistinctLeagueInstance runs mac='distinct' only, got mac="
                                      f"{getattr(args, 'mac', 'basic')!r} (parameter-shared MACs are LeagueInstance)")

    def _counter_agent(self, mac):
        return mac.agents[0]  # the learner's one optimizer launch counts for all N networks: their counters are equal

    def _agent_state(self, mac):
        return [a.state_dict() for a in mac.agents]


def league_instance_for(args, logger, league, **kw) -> LeagueInstance:
    """The league instance of ``args.mac``: DistinctLeagueInstance for 'distinct', else LeagueInstance."""
    refuse_entity_league(args, "league_instance_for")
    cls = DistinctLeagueInstance if getattr(args, "mac", "basic") == "distinct" else LeagueInstance
    return cls(args, logger, league, **kw)


def league_roles_for(world: int, args) -> list:
    """Config 3 (2 learners): PFSP self-play between simple players; config 4 (>= 4 ranks): AlphaStar roles
    (half main players, half main exploiters unless league_main_agents / league_main_exploiters say otherwise)."""
    if world < 4:
        return ["simple"] * world
    return alphastar_roles(world, getattr(args, "league_main_agents", None),
                           getattr(args, "league_main_exploiters", None),
                           int(getattr(args, "league_league_exploiters", 0)))
