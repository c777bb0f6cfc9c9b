#!/usr/bin/env python
"""GPU: the time of one mlg_refil_rollout_selfplay launch against mlg_refil_rollout on the same env shape.

4096 envs of refil_8 (k = 3..8), fixed numpy weights (tests/refil_shapes.entity_agent_params, seeds 11 home / 23
away), every launch from the same env state (episode counters reset, so every repetition of an arm does the same work),
train mode at epsilon 0.3 on every side. Arms, alternated inside each repetition:

    selfplay   mlg_refil_rollout_selfplay (sp-ro2/kc2): two policies, two agent phases per step
    ro2        mlg_refil_rollout with MLG_REFIL_ROLLOUT=v1 (ro2/kc2): one policy against the scripted AI
    default    mlg_refil_rollout, default dispatch (ro4-static)

HIP events around each launch (a full-write batch, nothing allocated in the window), warm-up launches first, then the
repetitions; reported: median, min, max in ms, the mean steps per env and the longest episode of each arm (episodes
differ between the arms: the opponents differ; with a short --episode-limit nearly every env of every arm runs to the
limit and the launches do equal numbers of steps) and the ratios of the medians per launch and per env step. Writes one
JSON file.

    python scripts/refil_selfplay_timing.py [--envs 4096] [--episode-limit 100] [--reps 12] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ma-league_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import refil_selfplay_ref as SR  # noqa: E402
import refil_shapes as FS  # noqa: E402
from helpers import entity_scheme_for  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--episode-limit", type=int, default=100)
    ap.add_argument("--eps", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refil_selfplay", "timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from maleague import _native
    from maleague.components.batch_view import mlg_entity_batch
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.envs.entity_env import EntityEnvSpec
    from maleague.envs.teams_env import VecEnvState
    dev, B, T = torch.device("cuda:0"), a.envs, a.episode_limit
    env_args = {"match_build_plan": "refil_8", "episode_limit": T, "seed": 5, "grid_size": 20, "min_agents": 3,
                "max_agents": 8}
    specs = {False: EntityEnvSpec.from_env_args(env_args), True: EntityEnvSpec.from_env_args(env_args, self_play=True)}
    S, A = specs[True].S, specs[True].n_actions
    agents = [SR.sp_agent(dev, FS.entity_agent_params(8 + A, A, seed), S)[0] for seed in (11, 23)]
    scheme, groups, pre = entity_scheme_for(SR.side_info(specs[True]), torch)
    batches = [EpisodeBatch(scheme, groups, B, T + 1, preprocess=pre, device=dev) for _ in range(2)]
    mbs, keep = [], []
    for bt in batches:
        mb, k = mlg_entity_batch(bt)
        mb.full_write = 1
        mbs.append(mb)
        keep.append(k)
    st = {sp: VecEnvState(specs[sp], B, dev) for sp in specs}
    run = torch.zeros(6 * B, dtype=torch.int32, device=dev)
    ri = _native.MlgRunInfo(run[0:B].data_ptr(), run[4 * B:5 * B].data_ptr(), run[B:3 * B].data_ptr(),
                            run[3 * B:4 * B].data_ptr(), None, run[5 * B:6 * B].data_ptr())
    d = agents[0].dims()
    packed = [ag.packed() for ag in agents]
    stream = _native.stream_ptr()

    def launch(arm):
        sp = arm == "selfplay"
        st[sp].episode.zero_()
        if arm == "ro2":
            os.environ["MLG_REFIL_ROLLOUT"] = "v1"
        else:
            os.environ.pop("MLG_REFIL_ROLLOUT", None)
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        if sp:
            _native.call("mlg_refil_rollout_selfplay", _native.byref(specs[True].to_c()), _native.byref(st[True].to_c()),
                         _native.byref(d), _native.ptr(packed[0]), _native.ptr(packed[1]), _native.byref(mbs[0]),
                         _native.byref(mbs[1]), _native.byref(ri), a.eps, a.eps, 0, stream)
        else:
            _native.call("mlg_refil_rollout", _native.byref(specs[False].to_c()), _native.byref(st[False].to_c()),
                         _native.byref(d), _native.ptr(packed[0]), _native.byref(mbs[0]), _native.byref(ri), a.eps, 0,
                         stream)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), (float(run[0:B].float().mean().item()), int(run[0:B].max().item()))

    arms = ("selfplay", "ro2", "default")
    names = {}
    for arm in arms:
        if arm == "ro2":
            os.environ["MLG_REFIL_ROLLOUT"] = "v1"
        else:
            os.environ.pop("MLG_REFIL_ROLLOUT", None)
        names[arm] = (_native.refil_rollout_selfplay_describe(specs[True].to_c(), d) if arm == "selfplay"
                      else _native.refil_rollout_describe(specs[False].to_c(), d))[0]
    for _ in range(a.warmup):
        for arm in arms:
            launch(arm)
    ms = {arm: [] for arm in arms}
    steps = {}
    for _ in range(a.reps):
        for arm in arms:
            t, steps[arm] = launch(arm)
            ms[arm].append(t)
    out = {"envs": B, "episode_limit": T, "eps": a.eps, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "arms": {}}
    for arm in arms:
        v = np.array(ms[arm])
        out["arms"][arm] = {"kernel": names[arm], "median_ms": float(np.median(v)), "min_ms": float(v.min()),
                            "max_ms": float(v.max()), "mean_steps_per_env": steps[arm][0],
                            "longest_episode": steps[arm][1],
                            "us_per_env_step": float(np.median(v)) * 1e3 / (B * steps[arm][0])}
    for arm in ("ro2", "default"):
        out[f"selfplay_over_{arm}_per_env_step"] = (out["arms"]["selfplay"]["us_per_env_step"]
                                                    / out["arms"][arm]["us_per_env_step"])
        out[f"selfplay_over_{arm}_launch"] = out["arms"]["selfplay"]["median_ms"] / out["arms"][arm]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
