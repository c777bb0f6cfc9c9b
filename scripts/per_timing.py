#!/usr/bin/env python
"""GPU: the measured figures of profiles/per/README.md (prioritized episode replay).

  replay    HIP-event time of mlg_per_sample at 5000 slots / 32 draws (the bench's replay ring and batch), of
            mlg_per_insert over 4096 slots and of mlg_per_update over 32 rows: each timed as a burst of --burst launches
            between two events (one launch is a few microseconds, below an event pair's resolution), the burst repeated;
            median and spread of the per-launch time.
  learner   one QLearner.train call (qmix) at the bench's learner shape, 32 episodes x 5 agents on a train-mode
            rollout's own batch, without and with importance weights (cfg.per = 0 / 1) on learners of their own with
            equal weights, the calls alternating: HIP events around the call, median and spread.

    python scripts/per_timing.py [--reps 30] [--warmup 5] [--burst 200] [--out FILE.json]

  --default-only times the unweighted call alone and touches nothing this feature added, so the same file runs in a
  checkout of the parent commit: the default path against its parent on the same box, alternating the two checkouts.

  launches  kernel launches per train call by difference, as scripts/distinct_timing.py counts them:
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/per_timing.py --launch-probe K [--per]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ma-league_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

from helpers import qmix_args, scheme_for  # noqa: E402


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def learner_on_rollout(device):
    """A QMIX learner on a 32-episode train-mode rollout of the bench's plan, truncated to max_t_filled."""
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.learners import QLearner
    from maleague.steppers import ParallelStepper
    args = qmix_args(batch_size_run=32, seed=1, learner_log_interval=10 ** 12,
                     env_args={"match_build_plan": "medium_1h_4t", "grid_size": 20, "stochastic_spawns": True,
                               "episode_limit": 100})
    stepper = ParallelStepper(args, MainLogger(log_interval=10 ** 12))
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"], info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(info, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    torch.manual_seed(1)
    mac = BasicMAC(proto.scheme, groups, args)
    stepper.initialize(scheme, groups, preprocess, mac)
    learner = QLearner(mac, proto.scheme, MainLogger(log_interval=10 ** 12), args, name="home")
    learner.build_optimizer()
    stepper.t_env = 30000
    batch, _ = stepper.run(test_mode=False)
    stepper.flush()
    T = int(batch.max_t_filled())
    return learner, batch[:, :T], T, args


def timed_call(learner, sample, it):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    learner.train(sample, 30000, it)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def time_learners(reps, warmup, device, default_only):
    legs = {"QLearner.train per=0": learner_on_rollout(device)}
    if not default_only:
        learner, sample, T, args = learner_on_rollout(device)
        g = torch.Generator().manual_seed(2)
        sample.is_weight = (0.1 + 0.9 * torch.rand(sample.batch_size, generator=g)).to(device)
        legs["QLearner.train per=1"] = (learner, sample, T, args)
    times = {k: [] for k in legs}
    for it in range(warmup + reps):
        for name, (learner, sample, T, args) in legs.items():
            ms = timed_call(learner, sample, it)
            if it >= warmup:
                times[name].append(ms)
    out = {}
    for name, (learner, sample, T, args) in legs.items():
        out[name] = dict(summary(times[name]), episodes=sample.batch_size, T=T, agents=args.n_agents)
        if not default_only:
            from maleague import _native
            out[name]["arm"] = _native.qlearner_describe(
                learner._cfg(sample.batch_size, sample.max_seq_length, per=name.endswith("1")))
    return out


def time_replay(reps, warmup, burst, device):
    from maleague import _native
    _native.load(require_gpu=True)
    st = _native.stream_ptr(device)
    slots, B, new = 5000, 32, 4096
    g = torch.Generator().manual_seed(3)
    prio = (0.05 + 3.0 * torch.rand(slots, generator=g)).to(device)
    mx = torch.ones(1, device=device)
    rows = torch.empty(B, dtype=torch.int32, device=device)
    w = torch.empty(B, device=device)
    td = torch.rand(B, generator=g).to(device)
    calls = {
        "mlg_per_sample 5000 slots x 32": lambda k: _native.call(
            "mlg_per_sample", prio.data_ptr(), slots, B, 7, k, 0.4, rows.data_ptr(), w.data_ptr(), None, 0, st),
        "mlg_per_insert 4096 slots": lambda k: _native.call(
            "mlg_per_insert", prio.data_ptr(), slots, (k * new) % slots, new, None, 0.01, 0.6, mx.data_ptr(), st),
        "mlg_per_update 32 rows": lambda k: _native.call(
            "mlg_per_update", prio.data_ptr(), slots, rows.data_ptr(), td.data_ptr(), B, 0.01, 0.6, mx.data_ptr(), st),
    }
    out = {}
    for name, fn in calls.items():
        ms = []
        for it in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(burst):
                fn(it * burst + k)
            b.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms.append(a.elapsed_time(b) / burst)
        out[name] = dict(summary(ms), burst=burst)
    return out


def launch_probe(calls, per, device):
    """Set-up, then `calls` train calls and nothing else: for a kernel trace (see the module docstring)."""
    learner, sample, T, args = learner_on_rollout(device)
    if per:
        sample.is_weight = torch.ones(sample.batch_size, device=device)
    torch.cuda.synchronize()
    for it in range(calls):
        timed_call(learner, sample, it)
    print(json.dumps({"launch_probe": calls, "per": per, "T": T}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burst", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--default-only", action="store_true", help="the unweighted train call alone (runs on the parent)")
    ap.add_argument("--launch-probe", type=int, default=0, metavar="K", help="run K train calls and exit (kernel trace)")
    ap.add_argument("--per", action="store_true", help="the probe's calls carry importance weights")
    a = ap.parse_args()
    device = torch.device("cuda:0")
    if a.launch_probe:
        return launch_probe(a.launch_probe, a.per, device)
    res = {"learner": time_learners(a.reps, a.warmup, device, a.default_only)}
    if not a.default_only:
        res["replay"] = time_replay(a.reps, a.warmup, a.burst, device)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
