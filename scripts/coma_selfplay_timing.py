"""One launch of `mlg_rollout_selfplay_policy` next to one of `mlg_rollout_selfplay` on the generic fp32 arm it is built
from, on one GPU.

    MLG_ROLLOUT_KERNEL=v1 python scripts/coma_selfplay_timing.py [--out profiles/coma_league] [--commit <hash>]
                                                                  [--repeats 10] [--envs 4096]

Shape: the league bench shape, 5v5 `medium_1h_4t` mirrored (both teams policy-controlled), H = 64, 4096 envs,
episode_limit 100, grid 20, train mode, epsilons from the configs' schedules (t_env starts at 50000 and every run adds
4096 x 100 steps, so both are at their floors in the timed runs; epsilon does not change the work). MLG_ROLLOUT_KERNEL=v1
makes mlg_rollout_selfplay launch `v1-global/tpw2` (the script refuses to run otherwise); the policy launch is
`sp-policy-global/tpw2`. HIP events around the run's single launch (stepper.timing). Warm-up runs of both, then
`repeats` runs of each, alternating; median, min, max. Recorded, not gated: the softmax and the draw add work per row,
and the games differ (other policies, other episode lengths), so the mean episode length stands next to each time.

Needs a GPU; nothing falls back."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ma-league_amd"))


def build(alg, B, dev):
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.components.transforms import OneHot
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.envs.plans import mirror_plan
    from maleague.steppers import SELF_POLICY_REGISTRY, SELF_REGISTRY
    from maleague.utils.config import build_config, to_args
    cfg = build_config(alg, "ma", overrides=[f"batch_size_run={B}", "runner=parallel", "buffer_cpu_only=False",
                                             "env_args.episode_limit=100", "show_exp_parameters=False", "seed=0"])
    args = to_args(cfg)
    args.env_args = dict(args.env_args, match_build_plan=mirror_plan(args.env_args["match_build_plan"], ai=False))
    reg = SELF_POLICY_REGISTRY if args.agent_output_type == "pi_logits" else SELF_REGISTRY
    stepper = reg["parallel"](args, MainLogger())
    info = stepper.get_env_info()
    args.n_agents, args.n_actions, args.state_shape = info["n_agents"] // 2, info["n_actions"], info["state_shape"]
    scheme = {"state": {"vshape": info["state_shape"]}, "obs": {"vshape": info["obs_shape"], "group": "agents"},
              "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long},
              "avail_actions": {"vshape": (info["n_actions"],), "group": "agents", "dtype": torch.int},
              "reward": {"vshape": (1,)}, "terminated": {"vshape": (1,), "dtype": torch.uint8}}
    groups = {"agents": args.n_agents}
    preprocess = {"actions": ("actions_onehot", [OneHot(out_dim=info["n_actions"])])}
    proto = EpisodeBatch(scheme, groups, 1, 2, preprocess=preprocess, device=dev)
    torch.manual_seed(0)
    home, away = BasicMAC(proto.scheme, groups, args), BasicMAC(proto.scheme, groups, args)
    stepper.initialize(scheme, groups, preprocess, home, away)
    return stepper


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--envs", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("coma_selfplay_timing: needs a GPU")
    dev = torch.device("cuda:0")
    steppers = {"mlg_rollout_selfplay_policy": build("coma", a.envs, dev),
                "mlg_rollout_selfplay": build("qmix", a.envs, dev)}
    arms = {k: st.describe_rollout()[0] for k, st in steppers.items()}
    if not arms["mlg_rollout_selfplay"].startswith("v1-"):
        sys.exit(f"coma_selfplay_timing: mlg_rollout_selfplay would launch {arms['mlg_rollout_selfplay']}; set "
                 "MLG_ROLLOUT_KERNEL=v1 (the generic fp32 arm the policy kernel is built from)")
    for st in steppers.values():
        st.t_env = 50000
        for _ in range(3):
            st.run(test_mode=False)
        st.flush()
        st.timing = []
    lens = {k: [] for k in steppers}
    for _ in range(a.repeats):
        for k, st in steppers.items():
            st.run(test_mode=False)
            st.flush()
            lens[k].append(float(st.last_run["ep_len"].float().mean()))
    torch.cuda.synchronize()
    res = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "envs": a.envs, "repeats": a.repeats,
           "shape": "5v5 medium_1h_4t mirrored, H 64, episode_limit 100, train mode"}
    for k, st in steppers.items():
        ms = [s.elapsed_time(e) for s, e in st.timing]
        res[k] = {"arm": arms[k], "ms": ms, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
                  "mean_ep_len": statistics.mean(lens[k]), "epsilons": list(st.epsilons)}
    p, q = res["mlg_rollout_selfplay_policy"], res["mlg_rollout_selfplay"]
    res["ratio_policy_over_q"] = p["median_ms"] / q["median_ms"]
    res["ratio_per_env_step"] = (p["median_ms"] / p["mean_ep_len"]) / (q["median_ms"] / q["mean_ep_len"])
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "timing.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
