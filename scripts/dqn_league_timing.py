"""Time of the feed-forward agent's self-play launch and cross-play evaluation next to the recurrent agent's.

    python scripts/dqn_league_timing.py [--out profiles/dqn_league] [--commit <hash>] [--envs 4096] [--runs 8]

Shape: the league bench's (5v5 medium_1h_4t mirrored, H = 64, episode_limit 100, grid 20, 4096 envs), freshly
initialised agents on both sides, train mode at the start of the epsilon schedule (epsilon 1.0 at home and away: every
pick is a random available action, so all four routes play the same games and differ only in the agent phase).

  ffsp-lds       SelfPlayFFParallelStepper.run: mlg_rollout_selfplay_ff, both weight images in LDS
  ffsp-global    the same with MLG_ROLLOUT_GLOBAL_WEIGHTS=1: weights read from global memory
  drqn-v1        SelfPlayParallelStepper.run with MLG_ROLLOUT_KERNEL=v1: mlg_rollout_selfplay's generic fp32 arm
  drqn-default   SelfPlayParallelStepper.run as shipped (the static-shape split-bf16 kernel at this shape)

Launch time: the stepper's own HIP events around the rollout launch (``stepper.timing``), `runs` launches per window,
`repeats` windows per route, the routes alternating; the figure is the median over all timed launches of a route. The
home batch is a fresh batch per run and the away batch the reused full-write batch, as in training.

Cross-play: P = 8 policies (flat vectors uniform in [-0.1, 0.1]), 64 pairs x 512 greedy games,
FFCrossPlayEvaluator.evaluate next to CrossPlayEvaluator.evaluate (the DRQN) over the same shape in alternating
windows between two HIP events that end in a synchronise: pool packing, one launch, the summary kernel and the one
device -> host copy. Needs a GPU; nothing falls back.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ma-league_amd"))

ENV = {"ffsp-lds": {}, "ffsp-global": {"MLG_ROLLOUT_GLOBAL_WEIGHTS": "1"}, "drqn-v1": {"MLG_ROLLOUT_KERNEL": "v1"},
       "drqn-default": {}}


def experiment(agent, envs, episode_limit):
    from maleague.custom_logging import MainLogger
    from maleague.envs.plans import builtin_plan
    from maleague.runs import LeagueExperiment
    from maleague.utils.config import build_config, to_args
    cfg = build_config("qmix", "ma", overrides=[f"agent={agent}", f"batch_size_run={envs}", "runner=parallel",
                                                "buffer_cpu_only=False", "buffer_size=32", "batch_size=32",
                                                f"env_args.episode_limit={episode_limit}", "zero_copy_insert=False",
                                                "show_exp_parameters=False", "t_max=1000000000000",
                                                "test_interval=1000000000000", "log_interval=1000000000",
                                                "runner_log_interval=1000000000", "learner_log_interval=1000000000"])
    cfg["env_args"]["match_build_plan"] = builtin_plan("medium_1h_4t", self_play=True)
    exp = LeagueExperiment(to_args(cfg), MainLogger())
    exp._init_stepper()
    return exp


class environ:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_league"))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episode-limit", dest="episode_limit", type=int, default=100)
    ap.add_argument("--runs", type=int, default=8, help="launches per window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pool", type=int, default=8)
    ap.add_argument("--episodes", type=int, default=512)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dqn_league_timing needs a ROCm GPU")
    from maleague.league.evaluation import CrossPlayEvaluator, FFCrossPlayEvaluator, build_pairs
    from maleague.runs.sp_ma_experiment import agent_vector
    dev = torch.device("cuda:0")
    exps = {"dqn": experiment("dqn", a.envs, a.episode_limit), "rnn": experiment("rnn", a.envs, a.episode_limit)}
    steppers = {k: exps["dqn" if k.startswith("ffsp") else "rnn"].stepper for k in ENV}
    arms, ms, ep_len = {}, {k: [] for k in ENV}, {}

    def launches(route, n):
        st = steppers[route]
        with environ(ENV[route]):
            arms[route] = st.describe_rollout()[0]
            st.timing = []
            for _ in range(n):
                st.t_env = 0
                st.run(test_mode=False)
            st.flush()
            torch.cuda.synchronize()
            out = [s.elapsed_time(e) for s, e in st.timing]
            st.timing = None
            ep_len[route] = float(st.last_run["ep_len"].double().mean())
        return out

    for route in ENV:  # warm-up of every route
        launches(route, 2)
    for _ in range(a.repeats):
        for route in ENV:
            ms[route] += launches(route, a.runs)

    # ---- cross-play ----
    P, E = a.pool, a.episodes
    table = build_pairs(range(P), range(P))
    cp, cp_ms, cp_out = {}, {"dqn": [], "rnn": []}, {}
    for k, cls in (("dqn", FFCrossPlayEvaluator), ("rnn", CrossPlayEvaluator)):
        n_params = agent_vector(exps[k].home_mac).numel()
        rows = []
        for p in range(P):
            g = torch.Generator().manual_seed(100 + p)
            rows.append((torch.rand(n_params, generator=g) * 2 - 1) * 0.1)
        cp[k] = (cls(exps[k].args, dev, episodes_per_launch=E), torch.stack(rows).to(dev))
        cp[k][0].evaluate(cp[k][1], table, E)  # warm-up
    for _ in range(a.repeats):
        for k, (ev, pool) in cp.items():
            t, cp_out[k] = window(lambda: ev.evaluate(pool, table, E))
            cp_ms[k].append(t)

    med = {k: statistics.median(v) for k, v in ms.items()}
    summary = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "envs": a.envs,
               "episode_limit": a.episode_limit, "runs_per_window": a.runs, "repeats": a.repeats,
               "launch": {k: {"arm": arms[k], "median_ms": med[k], "min_ms": min(ms[k]), "max_ms": max(ms[k]),
                              "n": len(ms[k]), "mean_ep_len": ep_len[k]} for k in ENV},
               "crossplay": {k: {"median_ms": statistics.median(v), "windows_ms": v,
                                 "mean_ep_len": float(cp_out[k].mean_ep_len.mean()),
                                 "buffer_bytes": cp[k][0].bytes_allocated()} for k, v in cp_ms.items()},
               "pool": P, "episodes_per_pair": E}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "timing.json"), "w") as f:
        json.dump(summary, f, indent=2)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
