"""QLearner.train / REFILLearner.train (MODE=refil) microbenchmark on the bench's shapes: 5v5 medium_1h_4t (refil:
refil_8, 3-8 agents) rollouts (ENVS envs, episode_limit 100) fill a device replay ring, then REPS train() calls on
batch_size 32 samples read in place (the bench's path). MODE=iql / vdn select those algorithms, MODE=attn_qmix /
attn_vdn the REFIL learner's attention baselines (plain entity agent, FlexQMixer / VDNMixer); extra key=value
arguments are config overrides (e.g. hypernet_layers=1 mixing_embed_dim=64), so any mixer shape is timed the same way.
EP_STEP=N advances episode_num by N per call (0: the target network is never updated).
Prints mean ms per train() (HIP events on the learner's stream), the loss of the last call and a SHA-256 of the
flat parameters after the last call (same seeds -> same bytes, whichever library computed them), so variant libraries
(MLG_LIB=...) can be A/B-compared; run under rocprofv3 --kernel-trace --stats for the per-kernel split."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ma-league_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

from maleague.custom_logging import MainLogger
from maleague.runs import MultiAgentExperiment
from maleague.utils.config import build_config, to_args

ENVS = int(os.environ.get("ENVS", "512"))
REPS = int(os.environ.get("REPS", "50"))
overrides = [f"batch_size_run={ENVS}", "runner=parallel", "buffer_cpu_only=False",
             "env_args.match_build_plan=medium_1h_4t", "env_args.episode_limit=100", "seed=0",
             "learner_log_interval=1000000000", "log_interval=1000000000", "runner_log_interval=1000000000",
             "test_interval=1000000000000", "t_max=1000000000000", "show_exp_parameters=False"]
MODE = os.environ.get("MODE", "qmix")
# episodes gathered between two train() calls: the episode_num of call r is (r + 1) * EP_STEP, so a value >=
# target_update_interval (bench.py's runs: batch_size_run = 4096 >= 200) has every call end with a target update
EP_STEP = int(os.environ.get("EP_STEP", "0"))
if MODE in ("refil", "attn_qmix", "attn_vdn"):
    overrides = [o.replace("medium_1h_4t", "refil_8") for o in overrides]
    cfg = build_config(MODE, "ma_entity", overrides=overrides + sys.argv[1:], device_index=0)
else:
    if MODE not in ("qmix", "iql", "vdn"):
        raise SystemExit(f"MODE={MODE!r}: qmix, iql, vdn, refil, attn_qmix or attn_vdn")
    cfg = build_config(MODE, "ma", overrides=overrides + sys.argv[1:], device_index=0)
np.random.seed(0)
torch.manual_seed(0)
args = to_args(cfg)
exp = MultiAgentExperiment(args, MainLogger(log_interval=10 ** 12))
exp._init_stepper()
exp.stepper.t_env = 10 ** 6
for i in range(2):  # fill the ring (and warm the learner)
    exp._train_episode(i * ENVS)
torch.cuda.synchronize()
buf, lrn = exp.home_buffer, exp.home_learner
samples = [buf.sample(args.batch_size, view=True) for _ in range(REPS)]
lrn.train(samples[0], 10 ** 6, 0)
torch.cuda.synchronize()
ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
for r in range(REPS):
    ev[r][0].record()
    lrn.train(samples[r], 10 ** 6, (r + 1) * EP_STEP)
    ev[r][1].record()
torch.cuda.synchronize()
ms = [a.elapsed_time(b) for a, b in ev]
sha = hashlib.sha256(lrn._flat.flat.detach().cpu().numpy().tobytes()).hexdigest()
print(json.dumps({"mode": MODE, "train_ms": sum(ms) / len(ms), "min_ms": min(ms), "median_ms": float(np.median(ms)),
                  "loss": lrn.last_stats["loss"], "param_sha256": sha,
                  "grad_norm": lrn.last_stats["grad_norm"], "T": samples[0].max_seq_length,
                  "t_filled_mean": float(np.mean([int(s_.max_t_filled()) for s_ in samples[:10]]))}))
