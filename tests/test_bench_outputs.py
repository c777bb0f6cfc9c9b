"""bench.py --dump-outputs and the plain / --full split.

CPU: dump_outputs on a hand-built experiment whose last rollout sits in replay-ring slots that wrap around the ring's
end -- the sampled episodes must be read from the right slots, every file float32 / float64, the whole dump under the
64 MB limit. GPU: one tiny plain run of the bench itself (what the test is about): exactly --steps timed steps, the
headline leg only, ms_per_step in the line, the dump written."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_reads_wrapped_ring_slots(tmp_path):
    from maleague.components.replay_buffer import ReplayBuffer, RingEpisodeBatch
    bench = _bench_module()
    scheme = {"obs": {"vshape": 3, "group": "agents"}, "reward": {"vshape": (1,)},
              "actions": {"vshape": (1,), "group": "agents", "dtype": torch.long}}
    size, B, T = 100, 80, 4
    ring = ReplayBuffer(scheme, {"agents": 2}, size, T, device="cpu")
    g = torch.Generator().manual_seed(3)
    for k, v in ring.data.transition_data.items():
        v.copy_(torch.randint(0, 50, v.shape, generator=g).to(v.dtype))
    slot0 = 70  # episodes 0..29 in slots 70..99, episodes 30..79 in slots 0..49
    batch = RingEpisodeBatch(ring, slot0, B)
    params = torch.arange(10, dtype=torch.float32)
    learner = SimpleNamespace(_flat=SimpleNamespace(flat=params), _tflat=SimpleNamespace(flat=params + 1),
                              _sq=params * 2, last_stats={"loss": 0.5, "grad_norm": 2.0})
    last = {"ep_len": torch.arange(B, dtype=torch.int32), "returns": torch.arange(B, dtype=torch.float32) / 4}
    exp = SimpleNamespace(stepper=SimpleNamespace(last_run=last, home_batch=batch), home_learner=learner)
    bench.dump_outputs(str(tmp_path), exp)

    got = {f[:-4]: np.load(tmp_path / f, allow_pickle=False) for f in os.listdir(tmp_path)}
    assert set(got) == {"params", "target_params", "square_avg", "train_stats", "rollout_ep_len", "rollout_returns",
                        "rollout_envs", "rollout_obs", "rollout_reward", "rollout_actions", "rollout_filled"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 * 2 ** 20
    assert np.array_equal(got["params"], params.numpy()) and np.array_equal(got["square_avg"], 2 * params.numpy())
    assert np.array_equal(got["train_stats"], [0.5, 2.0]) and got["train_stats"].dtype == np.float64
    assert np.array_equal(got["rollout_ep_len"], np.arange(B))
    envs = got["rollout_envs"].astype(np.int64)
    assert len(envs) == min(B, bench.DUMP_ENVS) and len(set(envs)) == len(envs) and (np.diff(envs) > 0).all()
    assert envs.min() < size - slot0 <= envs.max(), "the sample should straddle the wrap for this test to bite"
    for k in ("obs", "reward", "actions", "filled"):
        want = ring.data.transition_data[k][(envs + slot0) % size].float().numpy()
        assert np.array_equal(got["rollout_" + k], want), k
    # the same arguments give the same sample
    bench.dump_outputs(str(tmp_path / "again"), exp)
    assert np.array_equal(np.load(tmp_path / "again" / "rollout_envs.npy"), got["rollout_envs"])


@pytest.mark.gpu
def test_plain_bench_run_times_the_headline_leg_and_dumps(device, tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--envs", "128", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "env-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    # value = env steps of the 3 timed iterations / their time
    assert out["value"] == pytest.approx(out["env_steps"] / (3 * out["ms_per_step"] * 1e-3), rel=1e-6)
    assert 3 * 128 <= out["env_steps"] <= 3 * 128 * 100
    # a plain run: no league / REFIL leg, no CPU baseline
    assert "league" not in out and "refil" not in out and out["cpu_baseline"] is None
    got = {f[:-4]: np.load(tmp_path / f, allow_pickle=False) for f in os.listdir(tmp_path)}
    assert {"params", "target_params", "square_avg", "train_stats", "rollout_ep_len", "rollout_returns",
            "rollout_envs", "rollout_obs", "rollout_state", "rollout_actions", "rollout_reward"} <= set(got)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 * 2 ** 20
    assert got["rollout_ep_len"].shape == (128,) and got["rollout_obs"].shape[:2] == (64, 101)
    assert got["params"].size > 0 and np.abs(got["square_avg"]).sum() > 0  # the learner trained
    # the sampled episodes are the last rollout's: rewards past an episode's end are zero, its return is their sum
    envs = got["rollout_envs"].astype(np.int64)
    L = got["rollout_ep_len"][envs].astype(np.int64)
    rew = got["rollout_reward"][..., 0]
    for i, n in enumerate(L):
        assert not rew[i, n:].any()
    assert np.allclose(rew.sum(1), got["rollout_returns"][envs], rtol=1e-5, atol=1e-5)
