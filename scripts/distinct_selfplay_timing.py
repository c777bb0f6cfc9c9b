#!/usr/bin/env python
"""GPU: the measured self-play and cross-play figures of profiles/distinct/README.md.

  rollout    HIP-event time of one mlg_rollout_selfplay_distinct launch (two DistinctMACs, obs_agent_id off) at 5v5 /
             H 64 / 4096 envs (the medium_1h_4t plan, both teams policy-controlled, episode limit 100, train mode at
             t_env 30000), next to mlg_rollout_selfplay (two BasicMACs, obs_agent_id off) at the same shape under
             MLG_ROLLOUT_KERNEL=v1 (the like-for-like generic fp32 kernel) and under the default dispatch, the latter
             also with obs_agent_id on (the configs' default input width, which the static-shape arm serves). The legs
             alternate; median and spread over the repetitions after the warm-up runs.
  crossplay  one DistinctCrossPlayEvaluator.evaluate call (pool pack, mlg_crossplay_rollout_distinct, summary, the one
             device -> host copy) of 3 policies, 9 pairs x 512 greedy games, HIP events around the call, next to the
             summed launch times of nine test-mode mlg_rollout_selfplay_distinct runs of 512 envs.

    python scripts/distinct_selfplay_timing.py [--envs 4096] [--reps 10] [--warmup 3] [--out FILE.json]
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

PLAN, LIMIT, H = "medium_1h_4t", 100, 64


def build(mac_name, B, device, agent_id=False):
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.controllers import REGISTRY
    from maleague.custom_logging import MainLogger
    from maleague.envs.plans import builtin_plan
    from maleague.steppers import SELF_DISTINCT_REGISTRY, SELF_REGISTRY
    args = qmix_args(batch_size_run=B, seed=1, obs_agent_id=agent_id, mac=mac_name, rnn_hidden_dim=H,
                     learner_log_interval=10 ** 12,
                     env_args={"match_build_plan": builtin_plan(PLAN, self_play=True), "grid_size": 20,
                               "stochastic_spawns": True, "episode_limit": LIMIT})
    reg = SELF_DISTINCT_REGISTRY if mac_name == "distinct" else SELF_REGISTRY
    stepper = reg["parallel"](args, MainLogger(log_interval=10 ** 12))
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    scheme, groups, preprocess = scheme_for(dict(info, n_agents=args.n_agents), torch)
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=device)
    torch.manual_seed(1)
    macs = [REGISTRY[mac_name](proto.scheme, groups, args) for _ in range(2)]
    for m in macs:
        m.cuda()
    stepper.initialize(scheme, groups, preprocess, *macs)
    return stepper, macs, args


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def timed_run(stepper, kernel, test_mode=False):
    if kernel:
        os.environ["MLG_ROLLOUT_KERNEL"] = kernel
    else:
        os.environ.pop("MLG_ROLLOUT_KERNEL", None)
    stepper.timing = []
    stepper.t_env = 30000
    stepper.run(test_mode=test_mode)
    stepper.flush()
    torch.cuda.synchronize()
    (a, b), = stepper.timing
    arm = stepper.describe_rollout()[0]
    os.environ.pop("MLG_ROLLOUT_KERNEL", None)
    return a.elapsed_time(b), arm


def time_rollouts(envs, reps, warmup, device):
    legs = {"mlg_rollout_selfplay_distinct": (build("distinct", envs, device)[0], None),
            "mlg_rollout_selfplay.v1": (build("basic", envs, device)[0], "v1"),
            "mlg_rollout_selfplay.default": (build("basic", envs, device)[0], None),
            # the config default input width (agent id on): the static-shape arm serves it
            "mlg_rollout_selfplay.default+agent_id": (build("basic", envs, device, agent_id=True)[0], None)}
    out, times = {}, {k: [] for k in legs}
    for it in range(warmup + reps):
        for name, (stepper, kernel) in legs.items():
            ms, arm = timed_run(stepper, kernel)
            if it >= warmup:
                times[name].append(ms)
            out.setdefault(name, {})["arm"] = arm
            out[name]["env_steps"] = int(stepper.last_run["ep_len"].sum())
    for name in legs:
        out[name].update(summary(times[name]))
    return out


def time_crossplay(reps, warmup, device, P=3, E=512):
    from maleague.envs.teams_env import VecEnvState
    from maleague.league.evaluation import DistinctCrossPlayEvaluator, build_pairs
    from maleague.runs.sp_ma_experiment import load_agent_vector
    stepper, macs, args = build("distinct", E, device)
    stepper.args.reuse_away_batch = False
    nh = macs[0].n_agents
    n_params = sum(p.numel() for p in macs[0].agents[0].parameters())
    g = torch.Generator().manual_seed(7)
    pool = ((torch.rand(P, nh * n_params, generator=g) * 2 - 1) * 0.3).to(device)
    table = build_pairs(range(P), range(P))
    ev = DistinctCrossPlayEvaluator(args, device, episodes_per_launch=E)
    one, nine = [], []
    for it in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ev.evaluate(pool, table, E, episode0=it)
        b.record()
        torch.cuda.synchronize()
        total = 0.0
        for h, aw, _ in table.pairs.tolist():
            load_agent_vector(macs[0], pool[h])
            load_agent_vector(macs[1], pool[aw])
            stepper.envs = VecEnvState(stepper.spec, E, device)
            stepper.envs.episode.fill_(it)
            total += timed_run(stepper, None, test_mode=True)[0]
        if it >= warmup:
            one.append(a.elapsed_time(b))
            nine.append(total)
    return {"DistinctCrossPlayEvaluator.evaluate": dict(summary(one), pairs=P * P, episodes=E),
            "nine mlg_rollout_selfplay_distinct launches": dict(summary(nine), pairs=P * P, envs=E,
                                                                arm=stepper.describe_rollout()[0])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    device = torch.device("cuda:0")
    res = {"rollout": time_rollouts(a.envs, a.reps, a.warmup, device),
           "crossplay": time_crossplay(a.reps, a.warmup, device)}
    print(json.dumps(res, indent=2))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
