"""Time of one feed-forward rollout launch on one GPU, next to the generic DRQN rollout kernel.

    python scripts/dqn_timing.py [--out profiles/dqn] [--commit <hash>] [--repeats 20] [--envs 4096]

Shape: the bench's config 2 (5v5 `medium_1h_4t`, H = 64, episode_limit 100, grid 20, 4096 envs), train mode at a flat
epsilon (t_env past the anneal). HIP events around the single launch of one ParallelStepper.run (stepper.timing):

  mlg_rollout_ff          agent: dqn, the arm mlg_rollout_ff_describe reports
  mlg_rollout (v1)        agent: rnn under MLG_ROLLOUT_KERNEL=v1, the generic fp32 kernel mlg_rollout_ff is built on
  mlg_rollout (default)   agent: rnn, the default arm for the shape, for scale

Warm-up runs, then `repeats` runs of each, alternating; median and spread. The two agents play different policies, so
their episodes differ in length: the mean episode length of the last run is recorded with each figure, and
us_per_env_step divides the launch time by the env steps of that launch. No threshold: a baseline for later tuning.

Needs a GPU; nothing falls back."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ma-league_amd"))


def build(agent, B, dev, episode_limit=100):
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.components.transforms import OneHot
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import ParallelStepper
    from maleague.utils.config import build_config, to_args
    cfg = build_config("qmix", "ma", overrides=[f"batch_size_run={B}", "runner=parallel", "buffer_cpu_only=False",
                                                f"env_args.episode_limit={episode_limit}", "show_exp_parameters=False",
                                                "learner_log_interval=1000000000", "seed=0", f"agent={agent}"])
    args = to_args(cfg)
    stepper = ParallelStepper(args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"], info["n_actions"], info["state_shape"]
    scheme = {"state": {"vshape": info["state_shape"]}, "obs": {"vshape": info["obs_shape"], "group": "agents"},
              "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
              "avail_actions": {"vshape": (info["n_actions"],), "group": "agents", "dtype": torch.int},
              "reward": {"vshape": (1,)}, "terminated": {"vshape": (1,), "dtype": torch.uint8}}
    groups = {"agents": info["n_agents"]}
    preprocess = {"actions": ("actions_onehot", [OneHot(out_dim=info["n_actions"])])}
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=dev)
    torch.manual_seed(0)
    mac = BasicMAC(proto.scheme, groups, args)
    stepper.initialize(scheme, groups, preprocess, mac)
    return stepper


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn"))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--envs", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dqn_timing needs a ROCm GPU")
    dev = torch.device("cuda:0")
    # (label, agent, MLG_ROLLOUT_KERNEL)
    routes = [("mlg_rollout_ff", "dqn", None), ("mlg_rollout.v1", "rnn", "v1"), ("mlg_rollout.default", "rnn", None)]
    steppers = {label: build(agent, a.envs, dev) for label, agent, _ in routes}

    def run(label, kernel):
        if kernel is None:
            os.environ.pop("MLG_ROLLOUT_KERNEL", None)
        else:
            os.environ["MLG_ROLLOUT_KERNEL"] = kernel
        st = steppers[label]
        arm = st.describe_rollout()[0]
        st.run(test_mode=False)
        st.flush()
        os.environ.pop("MLG_ROLLOUT_KERNEL", None)
        return arm

    arms, steps = {}, {label: [] for label, _, _ in routes}
    for label, _, kernel in routes:
        steppers[label].t_env = 100000  # past the anneal: epsilon flat at 0.05
        for _ in range(3):
            arms[label] = run(label, kernel)
        steppers[label].timing = []
    for _ in range(a.repeats):
        for label, _, kernel in routes:
            run(label, kernel)
            steps[label].append(int(steppers[label].last_run["ep_len"].sum()))
    torch.cuda.synchronize()
    out = {}
    for label, _, _ in routes:
        ms = [x.elapsed_time(y) for x, y in steppers[label].timing]
        assert len(ms) == a.repeats, (label, len(ms))
        per = [1e3 * m / s for m, s in zip(ms, steps[label])]
        out[label] = {"arm": arms[label], "ms": ms, "median_ms": statistics.median(ms), "min_ms": min(ms),
                      "max_ms": max(ms), "env_steps": steps[label],
                      "median_us_per_env_step": statistics.median(per),
                      "mean_ep_len": statistics.mean(steps[label]) / a.envs}
    summary = {"commit": a.commit, "device": torch.cuda.get_device_name(0),
               "arch": torch.cuda.get_device_properties(0).gcnArchName, "repeats": a.repeats, "envs": a.envs,
               "rollout": out}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "timing.json"), "w") as f:
        json.dump(summary, f, indent=2)
    print(json.dumps({k: {"arm": v["arm"], "median_ms": round(v["median_ms"], 4), "min_ms": round(v["min_ms"], 4),
                          "max_ms": round(v["max_ms"], 4), "mean_ep_len": round(v["mean_ep_len"], 2),
                          "median_us_per_env_step": round(v["median_us_per_env_step"], 5)} for k, v in out.items()}))


if __name__ == "__main__":
    main()
