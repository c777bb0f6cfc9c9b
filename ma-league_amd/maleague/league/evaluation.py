"""League cross-play evaluation: who beats whom among a pool of policies, greedy, on equal terms.

Joint-policy-correlation evaluation of the reference (``src/runs/evaluation/jpc_eval_run.py:62-89``: every instance's
home policy against every instance's away policy, ``evaluate_mean_returns`` per pair) and ``src/eval/methods.py:8-18``.
The reference -- and ``SelfPlayMultiAgentExperiment.evaluate_mean_returns`` here -- plays one pair per rollout through
the training stepper. ``CrossPlayEvaluator`` plays every (home, away, roster) pair of a pool in ONE launch of
``mlg_crossplay_rollout``: each workgroup reads its two policies from the packed pool by index, no EpisodeBatch is
written, and a second kernel reduces the per-env results to one summary row per pair. Every pair sees the same
``episodes`` spawn draws (env index e, episode counter ``episode0 + launch``): common random numbers.

``PolicyCrossPlayEvaluator`` is the same evaluation for ``pi_logits`` policies (COMA): ``mlg_crossplay_rollout_policy``
picks with the policy softmax in test mode (greedy, or a draw with ``test_greedy=False``); ``evaluator_for`` picks
the class by ``args.agent_output_type``. ``DistinctCrossPlayEvaluator`` is the evaluation for ``mac: distinct`` policies
(one DRQN per agent slot, a pool row being a policy's N networks back to back): ``mlg_crossplay_rollout_distinct``.
``FFCrossPlayEvaluator`` is the evaluation for feed-forward policies (agent: dqn, a pool row being fc1 and fc2 flat):
``mlg_ff_pack_pool`` and ``mlg_crossplay_rollout_ff``.

The training payoff (``DistributedLeague.payoff``) holds epsilon-greedy training games of the pairs the matchmaker
drew; this table is separate and never written into it.
"""
from __future__ import annotations

import ctypes
import json
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import torch

from .. import _native
from ..envs.plans import mirror_plan
from ..exceptions import refuse_entity_league
from ..envs.teams_env import TeamsEnvSpec
from .teams import match_plan

# columns of a summary row (mlg_crossplay_rollout's summary[n_pairs][8])
GAMES, WINS, LOSSES, DRAWS, RET_HOME, RET_AWAY, EP_LEN = range(7)
SUMMARY_COLS = 8


@dataclass
class PairTable:
    """The (home, away, roster) pairs of an evaluation.

    ``pairs``  int32 [n, 3] host tensor: pool row of the home policy, pool row of the away policy, index into ``plans``
    ``cells``  int64 [n, 2]: the (row, column) of the result matrix each pair belongs to
    ``shape``  (homes, aways) of the result matrix
    ``plans``  the distinct match_build_plans (``None``: the env config's own plan, mirrored)
    """
    pairs: torch.Tensor
    cells: torch.Tensor
    shape: tuple
    plans: list

    def __len__(self) -> int:
        return int(self.pairs.shape[0])

    def __getitem__(self, idx) -> "PairTable":
        """A subset of the pairs (``table[rank::world]``) over the same matrix and plans."""
        if isinstance(idx, int):
            idx = slice(idx, idx + 1)
        return PairTable(self.pairs[idx], self.cells[idx], self.shape, self.plans)


def build_pairs(home_pids: Sequence[int], away_pids: Sequence[int],
                team_of: Optional[Callable[[int], object]] = None) -> PairTable:
    """Every home pid against every away pid, home-major (pair k = (home_pids[k // Pa], away_pids[k % Pa])). A pid is
    the policy's row in the pool. With ``team_of`` each pair plays ``match_plan(team_of(home), team_of(away))``, the
    distinct plans de-duplicated in order of first use; without teams every pair plays the env config's mirrored plan
    (one spec, ``plans == [None]``). Pure host function."""
    home_pids, away_pids = [int(p) for p in home_pids], [int(p) for p in away_pids]
    plans, index, rows, cells = [], {}, [], []
    for r, h in enumerate(home_pids):
        for c, a in enumerate(away_pids):
            if team_of is None:
                key, plan = None, None
            else:
                plan = match_plan(team_of(h), team_of(a))
                key = json.dumps(plan, sort_keys=True, default=str)
            if key not in index:
                index[key] = len(plans)
                plans.append(plan)
            rows.append((h, a, index[key]))
            cells.append((r, c))
    return PairTable(torch.tensor(rows, dtype=torch.int32).reshape(-1, 3),
                     torch.tensor(cells, dtype=torch.int64).reshape(-1, 2), (len(home_pids), len(away_pids)), plans)


def avg_proportional_loss(jpc: torch.Tensor):
    """Average proportional loss of a joint-policy-correlation matrix (eval/methods.py:8-18): (D - O) / D with D the
    mean of the diagonal (policies with their training partners) and O the mean off the diagonal. A negative D is not
    defined there either (NotImplementedError)."""
    jpc = torch.as_tensor(jpc)
    d = torch.diagonal(jpc).mean()
    off = ~torch.eye(*jpc.shape, dtype=torch.bool, device=jpc.device)
    o = jpc[off].mean()
    if d < 0:
        raise NotImplementedError("avg_proportional_loss: negative diagonal mean")
    if d - o < 0:
        print("Off-Diagonal-Mean greater than Diagonal-Mean")
    return (d - o) / d


class CrossPlayResult:
    """[homes, aways] evaluation tables, built from the per-cell totals [homes, aways, 8] (summary columns)."""

    def __init__(self, totals: torch.Tensor):
        self.totals = totals
        g = totals[..., GAMES]
        self.games, self.wins, self.losses, self.draws = g, totals[..., WINS], totals[..., LOSSES], totals[..., DRAWS]
        per_game = lambda x: torch.where(g > 0, x / g.clamp(min=1), torch.zeros_like(x))  # noqa: E731
        self.mean_return_home = per_game(totals[..., RET_HOME])
        self.mean_return_away = per_game(totals[..., RET_AWAY])
        self.mean_ep_len = per_game(totals[..., EP_LEN])

    @property
    def win_rate(self) -> torch.Tensor:
        """(wins + draws / 2) / games, 0.5 where no game was played (PayoffWrapper.win_rates)."""
        g = self.games
        return torch.where(g > 0, (self.wins + 0.5 * self.draws) / g.clamp(min=1), torch.full_like(g, 0.5))

    @property
    def jpc_matrix(self) -> torch.Tensor:
        """Home + away mean return per pair (jpc_eval_run.py:89)."""
        return self.mean_return_home + self.mean_return_away

    def avg_proportional_loss(self):
        return avg_proportional_loss(self.jpc_matrix)


def aggregate(summary: torch.Tensor, pairs, shape) -> CrossPlayResult:
    """Summary rows [n, 8] of ``pairs`` (a PairTable, or an int [n, >= 2] tensor whose first two columns are the
    matrix row and column) summed into the cells of a ``shape`` matrix. Pure torch; rows of a repeated pair add up."""
    cells = pairs.cells if isinstance(pairs, PairTable) else torch.as_tensor(pairs)[:, :2]
    cells = cells.to(device=summary.device, dtype=torch.int64)
    rows, cols = int(shape[0]), int(shape[1])
    if cells.numel() and (int(cells[:, 0].max()) >= rows or int(cells[:, 1].max()) >= cols or int(cells.min()) < 0):
        raise ValueError(f"aggregate: pair cells outside the {rows} x {cols} matrix")
    totals = torch.zeros(rows * cols, SUMMARY_COLS, dtype=summary.dtype, device=summary.device)
    totals.index_add_(0, cells[:, 0] * cols + cells[:, 1], summary.reshape(-1, SUMMARY_COLS))
    return CrossPlayResult(totals.reshape(rows, cols, SUMMARY_COLS))


class CrossPlayEvaluator:
    """Holds the packed pool, workspace and output tensors of the evaluation launches (created on first use, reused,
    grown when a call needs more). ``args``: the experiment's arguments (env_args, rnn_hidden_dim, obs_last_action,
    obs_agent_id, seed / league_eval_seed, config_dir). ``episodes_per_launch``: E of one launch (default
    ``args.league_eval_batch`` or 512)."""

    def __init__(self, args, device, episodes_per_launch: Optional[int] = None):
        self.args = args
        self.device = torch.device(device)
        refuse_entity_league(args, type(self).__name__)
        self._check_output_type(args)
        self._check_agent(args)
        self._check_mac(args)
        self.E = int(episodes_per_launch or getattr(args, "league_eval_batch", 512))
        if self.E < 1:
            raise ValueError(f"episodes_per_launch={self.E}")
        self._buf = {}
        self.launches = 0
        self.last = None  # per-env outputs and summary of the last launch (device views)

    def _check_output_type(self, args):
        if getattr(args, "agent_output_type", "q") != "q":
            raise NotImplementedError("cross-play evaluation plays greedy over Q values: agent_output_type="
                                      f"{args.agent_output_type!r} is not supported (COMA in the league is out of scope "
                                      "for CrossPlayEvaluator; pi_logits policies are PolicyCrossPlayEvaluator)")

    def _check_agent(self, args):
        if getattr(args, "agent", "rnn") != "rnn":
            raise NotImplementedError("cross-play evaluation runs the recurrent agent (agent='rnn') only: "
                                      f"agent={args.agent!r} is not supported (agent='dqn' and the other non-DRQN "
                                      "agents in cross-play are out of scope)")

    def _check_mac(self, args):
        if getattr(args, "mac", "basic") == "distinct":
            raise NotImplementedError(f"{type(self).__name__} packs one parameter-shared network per policy: "
                                      "mac='distinct' is not supported here (cross-play over distinct MACs is "
                                      "DistinctCrossPlayEvaluator, league.evaluation.evaluator_for)")

    def _launch(self, dims, c, stream):
        _native.call("mlg_crossplay_rollout", _native.byref(dims), _native.byref(c), stream)

    def _packed_size(self, lib, dims) -> int:
        """Floats of one packed block (negative: the native error is set)."""
        return int(lib.mlg_packed_agent_size(_native.byref(dims)))

    def _workspace_floats(self, lib, dims, n_pairs, E) -> int:
        """Workspace floats of one launch (negative: the native error is set)."""
        return int(lib.mlg_crossplay_workspace_floats(_native.byref(dims), n_pairs, E))

    def _pack_pool(self, dims, t, dst_ptr, stream):
        """Pack the policies of one pool tensor [P, row] to ``dst_ptr``; returns the blocks written per policy."""
        _native.call("mlg_pack_agent_pool", _native.byref(dims), t.data_ptr(), int(t.stride(0)), int(t.shape[0]),
                     dst_ptr, stream)
        return 1

    # ---- specs / dims ---------------------------------------------------------------------------------------
    def spec_of(self, plan) -> TeamsEnvSpec:
        a = self.args
        cdir = getattr(a, "config_dir", None)
        env_args = dict(a.env_args)
        seed = getattr(a, "league_eval_seed", None)
        env_args["seed"] = int(seed) if seed is not None else env_args.get("seed", getattr(a, "seed", 0))
        env_args["match_build_plan"] = plan if plan is not None else \
            mirror_plan(a.env_args["match_build_plan"], ai=False, config_dir=cdir)
        return TeamsEnvSpec.from_env_args(env_args, cdir)

    def dims_of(self, spec: TeamsEnvSpec) -> _native.MlgAgentDims:
        a = self.args
        nh, d_obs, A = max(spec.n_agents // 2, 1), 8 * spec.U, spec.n_actions
        la, ai = bool(getattr(a, "obs_last_action", True)), bool(getattr(a, "obs_agent_id", True))
        return _native.MlgAgentDims(d_obs=d_obs, n_actions=A, n_agents=nh, hidden=int(a.rnn_hidden_dim),
                                    d_in=d_obs + (A if la else 0) + (nh if ai else 0), obs_last_action=int(la),
                                    obs_agent_id=int(ai))

    def _blocks(self, dims) -> int:
        """Packed blocks per policy (one shared network)."""
        return 1

    def _tensor(self, name, numel, dtype):
        t = self._buf.get(name)
        if t is None or t.numel() < numel:
            t = torch.empty(max(int(numel), 1), dtype=dtype, device=self.device)
            self._buf[name] = t
        return t

    def bytes_allocated(self) -> int:
        return sum(t.numel() * t.element_size() for t in self._buf.values())

    # ---- the evaluation -------------------------------------------------------------------------------------
    def evaluate(self, pool, pairs, episodes: int, episode0: int = 0) -> CrossPlayResult:
        """``pool``: a [P, n_params] device tensor of flat agent parameters (named_parameters order), or a list of such
        tensors whose rows follow each other (``[league.current, league.historical]``); rows are read in place.
        ``pairs``: a PairTable, or an int32 [n, 3] tensor (home row, away row, spec 0 = the mirrored env config plan).
        Plays ``episodes`` games per pair (launches of at most ``episodes_per_launch``, launch k with episode counter
        ``episode0 + k``) and returns the [homes, aways] tables. One device -> host copy."""
        lib = _native.load(require_gpu=True)
        if not isinstance(pairs, PairTable):
            p = torch.as_tensor(pairs).to(torch.int32).reshape(-1, 3).cpu()
            shape = (int(p[:, 0].max()) + 1, int(p[:, 1].max()) + 1) if p.numel() else (0, 0)
            pairs = PairTable(p, p[:, :2].to(torch.int64), shape, [None])
        episodes = int(episodes)
        if episodes < 1:
            raise ValueError(f"evaluate: episodes={episodes}")
        n = len(pairs)
        if n == 0:
            return aggregate(torch.zeros(0, SUMMARY_COLS), pairs, pairs.shape)
        pools = [pool] if torch.is_tensor(pool) else list(pool)
        specs = [self.spec_of(plan) for plan in pairs.plans]
        dims = self.dims_of(specs[0])
        stream = _native.stream_ptr(self.device)
        # ---- the pool, packed (one launch per pool tensor; rows read in place through their stride) ----
        psize = self._packed_size(lib, dims)
        if psize < 0:
            raise _native.NativeError(lib.mlg_last_error().decode())
        P = sum(int(t.shape[0]) for t in pools)
        packed = self._tensor("packed_pool", P * psize * self._blocks(dims), torch.float32)
        row = 0
        for t in pools:
            if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or (t.shape[0] > 1 and t.stride(1) != 1):
                raise _native.NativeError("evaluate: pool tensors must be float32 [P, n_params] on the device with "
                                          f"contiguous rows, got {t.dtype} {tuple(t.shape)} on {t.device}")
            if t.shape[0] == 0:
                continue
            row += int(t.shape[0]) * self._pack_pool(dims, t, packed.data_ptr() + row * psize * 4, stream)
        # ---- pair and spec tables: host copies for validation, device copies for the launch ----
        host_pairs = pairs.pairs.to(torch.int32).contiguous()
        dev_pairs = host_pairs.to(self.device)
        cspecs = (_native.MlgEnvSpec * len(specs))(*[s.to_c() for s in specs])
        dev_specs = torch.frombuffer(bytearray(bytes(cspecs)), dtype=torch.uint8).to(self.device)
        E_max = min(self.E, episodes)
        ws_floats = self._workspace_floats(lib, dims, n, E_max)
        if ws_floats < 0:
            raise _native.NativeError(lib.mlg_last_error().decode())
        ws = self._tensor("workspace", ws_floats, torch.float32)
        ep_len = self._tensor("ep_len", n * E_max, torch.int32)
        ret = self._tensor("ret", n * E_max, torch.float32)
        ret_away = self._tensor("ret_away", n * E_max, torch.float32)
        won = self._tensor("won", 2 * n * E_max, torch.int32)
        draw = self._tensor("draw", n * E_max, torch.int32)
        summary = self._tensor("summary", n * SUMMARY_COLS, torch.float32)
        total, done, k = None, 0, 0
        while done < episodes:
            E = min(E_max, episodes - done)
            c = _native.MlgCrossplay(packed.data_ptr(), P, n, dev_pairs.data_ptr(), host_pairs.data_ptr(),
                                     dev_specs.data_ptr(), ctypes.addressof(cspecs), len(specs), E,
                                     (int(episode0) + k) & 0xFFFFFFFF, ws.data_ptr(), ws.numel(), ep_len.data_ptr(),
                                     ret.data_ptr(), ret_away.data_ptr(), won.data_ptr(), draw.data_ptr(),
                                     summary.data_ptr())
            self._launch(dims, c, stream)
            self.launches += 1
            self.last = {"E": E, "ep_len": ep_len[:n * E].view(n, E), "ret": ret[:n * E].view(n, E),
                         "ret_away": ret_away[:n * E].view(n, E), "won": won[:2 * n * E].view(n, E, 2),
                         "draw": draw[:n * E].view(n, E), "summary": summary[:n * SUMMARY_COLS].view(n, SUMMARY_COLS)}
            done += E
            k += 1
            if done < episodes or total is not None:  # more than one launch: sum the rows on the device
                total = self.last["summary"].clone() if total is None else total.add_(self.last["summary"])
        host = (total if total is not None else self.last["summary"]).cpu()  # the one device -> host copy
        return aggregate(host, pairs, pairs.shape)


class PolicyCrossPlayEvaluator(CrossPlayEvaluator):
    """CrossPlayEvaluator for ``pi_logits`` policies (COMA): every pair in one launch of
    ``mlg_crossplay_rollout_policy``, the pick being the policy rollout's in test mode -- the first-index argmax of the
    masked probabilities with ``args.test_greedy`` (default), else a draw from the floor-less probabilities on the
    counter RNG with the launch's episode counter. ``args.mask_before_softmax`` as in training."""

    def _check_output_type(self, args):
        if getattr(args, "agent_output_type", "q") != "pi_logits":
            raise NotImplementedError("policy cross-play evaluation picks from the policy softmax: agent_output_type="
                                      f"{getattr(args, 'agent_output_type', 'q')!r} is not supported (Q policies are "
                                      "CrossPlayEvaluator)")

    def _launch(self, dims, c, stream):
        a = self.args
        _native.call("mlg_crossplay_rollout_policy", _native.byref(dims), _native.byref(c),
                     int(bool(getattr(a, "mask_before_softmax", True))), int(bool(getattr(a, "test_greedy", True))),
                     stream)


class DistinctCrossPlayEvaluator(CrossPlayEvaluator):
    """CrossPlayEvaluator for ``mac: distinct`` policies (one DRQN per agent slot): every pair in one launch of
    ``mlg_crossplay_rollout_distinct``. A pool row is a policy's ``nh`` networks back to back, agent 0 first, each in
    named_parameters() order (``nh x n_params`` floats: runs.sp_ma_experiment.agent_vector of a DistinctMAC); a pool
    tensor is packed with one ``mlg_pack_agent_pool`` call over its ``P * nh`` rows of stride ``n_params``."""

    def _check_mac(self, args):
        if getattr(args, "mac", "basic") != "distinct":
            raise NotImplementedError(f"DistinctCrossPlayEvaluator evaluates mac='distinct' policies only, got mac="
                                      f"{getattr(args, 'mac', 'basic')!r} (parameter-shared policies are "
                                      "CrossPlayEvaluator)")

    def dims_of(self, spec: TeamsEnvSpec) -> _native.MlgAgentDims:
        a = self.args
        nh, d_obs, A = max(spec.n_agents // 2, 1), 8 * spec.U, spec.n_actions
        la = bool(getattr(a, "obs_last_action", True))
        # distinct networks take no agent id (network i is agent i)
        return _native.MlgAgentDims(d_obs=d_obs, n_actions=A, n_agents=nh, hidden=int(a.rnn_hidden_dim),
                                    d_in=d_obs + (A if la else 0), obs_last_action=int(la), obs_agent_id=0)

    def _blocks(self, dims) -> int:
        return int(dims.n_agents)

    def _pack_pool(self, dims, t, dst_ptr, stream):
        nh, H, A = int(dims.n_agents), int(dims.hidden), int(dims.n_actions)
        n_params = H * int(dims.d_in) + H + 6 * H * H + 6 * H + A * H + A
        P = int(t.shape[0])
        if int(t.shape[1]) != nh * n_params:
            raise _native.NativeError(f"evaluate: pool rows of {int(t.shape[1])} floats for {nh} networks of "
                                      f"{n_params} parameters each ({nh * n_params})")
        if P > 1 and int(t.stride(0)) != nh * n_params:
            raise _native.NativeError("evaluate: distinct pool tensors must be contiguous (row stride "
                                      f"{int(t.stride(0))} != {nh * n_params})")
        _native.call("mlg_pack_agent_pool", _native.byref(dims), t.data_ptr(), n_params, P * nh, dst_ptr, stream)
        return nh

    def _launch(self, dims, c, stream):
        _native.call("mlg_crossplay_rollout_distinct", _native.byref(dims), _native.byref(c), stream)


class FFCrossPlayEvaluator(CrossPlayEvaluator):
    """CrossPlayEvaluator for feed-forward policies (agent: dqn): every pair in one launch of
    ``mlg_crossplay_rollout_ff``. A pool row is a policy's four tensors flat in ``DQNAgentNetwork.PARAM_ORDER``
    (runs.sp_ma_experiment.agent_vector of a feed-forward MAC); a pool tensor is packed by one ``mlg_ff_pack_pool``
    launch into rows of ``mlg_ff_packed_size`` floats."""

    def _check_agent(self, args):
        if getattr(args, "agent", "rnn") != "dqn":
            raise NotImplementedError("FFCrossPlayEvaluator evaluates feed-forward policies (agent='dqn') only, got "
                                      f"agent={getattr(args, 'agent', 'rnn')!r} (recurrent policies are "
                                      "CrossPlayEvaluator)")

    def _packed_size(self, lib, dims) -> int:
        return int(lib.mlg_ff_packed_size(_native.byref(dims)))

    def _workspace_floats(self, lib, dims, n_pairs, E) -> int:
        return int(lib.mlg_crossplay_ff_workspace_floats(_native.byref(dims), n_pairs, E))

    def _pack_pool(self, dims, t, dst_ptr, stream):
        H, A = int(dims.hidden), int(dims.n_actions)
        n_params = H * int(dims.d_in) + H + A * H + A
        if int(t.shape[1]) != n_params:
            raise _native.NativeError(f"evaluate: pool rows of {int(t.shape[1])} floats for a feed-forward agent of "
                                      f"{n_params} parameters")
        _native.call("mlg_ff_pack_pool", _native.byref(dims), t.data_ptr(), int(t.stride(0)), int(t.shape[0]),
                     dst_ptr, stream)
        return 1

    def _launch(self, dims, c, stream):
        _native.call("mlg_crossplay_rollout_ff", _native.byref(dims), _native.byref(c), stream)


def evaluator_for(args, device, episodes_per_launch: Optional[int] = None) -> CrossPlayEvaluator:
    """The evaluator of ``args``: DistinctCrossPlayEvaluator for mac 'distinct' with agent_output_type 'q',
    FFCrossPlayEvaluator for agent 'dqn' with mac 'basic' and agent_output_type 'q', else by
    ``args.agent_output_type``: PolicyCrossPlayEvaluator for 'pi_logits', else CrossPlayEvaluator."""
    refuse_entity_league(args, "evaluator_for")
    out = getattr(args, "agent_output_type", "q")
    if getattr(args, "mac", "basic") == "distinct" and out == "q":
        cls = DistinctCrossPlayEvaluator
    elif getattr(args, "agent", "rnn") == "dqn" and getattr(args, "mac", "basic") == "basic" and out == "q":
        cls = FFCrossPlayEvaluator
    else:
        cls = PolicyCrossPlayEvaluator if out == "pi_logits" else CrossPlayEvaluator
    return cls(args, device, episodes_per_launch)


__all__ = ["PairTable", "build_pairs", "aggregate", "avg_proportional_loss", "CrossPlayResult", "CrossPlayEvaluator",
           "PolicyCrossPlayEvaluator", "DistinctCrossPlayEvaluator", "FFCrossPlayEvaluator", "evaluator_for",
           "GAMES", "WINS", "LOSSES", "DRAWS", "RET_HOME", "RET_AWAY", "EP_LEN"]
