#!/usr/bin/env python
"""GPU: the measured figures of profiles/distinct/README.md.

  rollout   HIP-event time of one mlg_rollout_distinct launch (mac: distinct, obs_agent_id off) at 5 agents / H 64 /
            4096 envs (the medium_1h_4t plan, episode limit 100, train mode at t_env 30000), next to mlg_rollout under
            MLG_ROLLOUT_KERNEL=v1 (BasicMAC, obs_agent_id off: the like-for-like generic fp32 kernel) at the same
            shape. The two alternate; median and spread over the repetitions after the warm-up runs.
  learner   one QLearner.train call (qmix) with mac=distinct at 32 episodes x 5 agents on a rollout's own batch, through
            both learner paths in one run -- the fused call (mlg_qlearner_train with cfg.distinct = 1, the default) and
            the unrolled branch (MLG_DISTINCT_LEARNER=unrolled), on learners of their own with equal weights, the calls
            alternating -- next to the shared-agent fused learner's (BasicMAC) on a batch of the same shape: HIP
            events around the call, median and spread.

    python scripts/distinct_timing.py [--envs 4096] [--reps 10] [--warmup 3] [--out FILE.json]

  launches  kernel launches per train call, by difference: the same process run twice under a kernel trace with K = 1
            and K = 3 train calls after the set-up; (count(3) - count(1)) / 2 is one call's launches, whatever the
            set-up and the rollout launched. --plan small is 3 agents, medium_1h_4t is 5.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- \
        python scripts/distinct_timing.py --launch-probe K [--path fused|unrolled] [--plan medium_1h_4t]
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


def build(mac_name, B, device, plan="medium_1h_4t", **kw):
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import REGISTRY
    from maleague.custom_logging import MainLogger
    from maleague.steppers import ParallelStepper
    args = qmix_args(batch_size_run=B, seed=1, obs_agent_id=False, mac=mac_name, learner_log_interval=10 ** 12,
                     env_args={"match_build_plan": plan, "grid_size": 20, "stochastic_spawns": True,
                               "episode_limit": 100}, **kw)
    stepper = ParallelStepper(args, MainLogger(log_interval=10 ** 12))
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"], info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(info, torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    torch.manual_seed(1)
    mac = REGISTRY[mac_name](proto.scheme, groups, args)
    stepper.initialize(scheme, groups, preprocess, mac)
    return stepper, mac, args, proto


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def time_rollouts(envs, reps, warmup, device):
    legs = {}
    for name, mac_name, kernel in (("mlg_rollout_distinct", "distinct", None), ("mlg_rollout.v1", "basic", "v1")):
        stepper, mac, args, _ = build(mac_name, envs, device)
        legs[name] = (stepper, kernel)
    out = {}
    times = {k: [] for k in legs}
    for it in range(warmup + reps):
        for name, (stepper, kernel) in legs.items():
            if kernel:
                os.environ["MLG_ROLLOUT_KERNEL"] = kernel
            else:
                os.environ.pop("MLG_ROLLOUT_KERNEL", None)
            stepper.timing = []
            stepper.t_env = 30000
            stepper.run(test_mode=False)
            stepper.flush()
            torch.cuda.synchronize()
            (a, b), = stepper.timing
            if it >= warmup:
                times[name].append(a.elapsed_time(b))
            out.setdefault(name, {})["arm"] = stepper.describe_rollout()[0]
            out[name]["env_steps"] = int(stepper.last_run["ep_len"].sum())
    os.environ.pop("MLG_ROLLOUT_KERNEL", None)
    for name in legs:
        out[name].update(summary(times[name]))
    return out


def learner_on_rollout(mac_name, device, plan="medium_1h_4t"):
    """A learner on a 32-episode train-mode rollout of its own MAC, truncated to max_t_filled."""
    from maleague.custom_logging import MainLogger
    from maleague.learners import QLearner
    stepper, mac, args, proto = build(mac_name, 32, device, plan=plan)
    learner = QLearner(mac, proto.scheme, MainLogger(log_interval=10 ** 12), args, name="home")
    learner.build_optimizer()
    stepper.t_env = 30000
    batch, _ = stepper.run(test_mode=False)
    stepper.flush()
    T = int(batch.max_t_filled())
    return learner, batch[:, :T], T, args


def timed_call(learner, sample, it, path=None):
    if path == "unrolled":
        os.environ["MLG_DISTINCT_LEARNER"] = "unrolled"
    else:
        os.environ.pop("MLG_DISTINCT_LEARNER", None)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    learner.train(sample, 30000, it)
    b.record()
    torch.cuda.synchronize()
    os.environ.pop("MLG_DISTINCT_LEARNER", None)
    return a.elapsed_time(b)


def time_learners(reps, warmup, device):
    out = {}
    # the two distinct paths: equal weights (the same seed builds both MACs), the same rollout, calls alternating
    legs = {}
    for name, path in (("QLearner.train mac=distinct fused", "fused"), ("QLearner.train mac=distinct unrolled", "unrolled")):
        legs[name] = learner_on_rollout("distinct", device) + (path,)
    times = {k: [] for k in legs}
    for it in range(warmup + reps):
        for name, (learner, sample, T, args, path) in legs.items():
            ms = timed_call(learner, sample, it, path)
            if it >= warmup:
                times[name].append(ms)
    for name, (learner, sample, T, args, path) in legs.items():
        out[name] = dict(summary(times[name]), episodes=32, T=T, agents=args.n_agents)
    learner, sample, T, args = learner_on_rollout("basic", device)
    ms = [timed_call(learner, sample, it) for it in range(warmup + reps)][warmup:]
    out["QLearner.train fused (mac=basic)"] = dict(summary(ms), episodes=32, T=T, agents=args.n_agents)
    return out


def launch_probe(calls, path, plan, device, mac="distinct"):
    """Set-up, then `calls` train calls and nothing else: for a kernel trace (see the module docstring)."""
    learner, sample, T, args = learner_on_rollout(mac, device, plan=plan)
    torch.cuda.synchronize()
    for it in range(calls):
        timed_call(learner, sample, it, path)
    print(json.dumps({"launch_probe": calls, "path": path, "agents": args.n_agents, "T": T}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--learner-only", action="store_true", help="skip the rollout legs")
    ap.add_argument("--launch-probe", type=int, default=0, metavar="K", help="run K train calls and exit (kernel trace)")
    ap.add_argument("--path", choices=("fused", "unrolled"), default="fused")
    ap.add_argument("--plan", default="medium_1h_4t")
    ap.add_argument("--mac", choices=("distinct", "basic"), default="distinct", help="the probe's MAC")
    a = ap.parse_args()
    device = torch.device("cuda:0")
    if a.launch_probe:
        return launch_probe(a.launch_probe, a.path, a.plan, device, a.mac)
    res = {} if a.learner_only else {"rollout": time_rollouts(a.envs, a.reps, a.warmup, device)}
    res["learner"] = time_learners(a.reps, a.warmup, device)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
