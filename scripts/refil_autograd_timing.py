"""Forward + backward time of the reference-style REFIL loop (EntityMAC unroll with the imagine copies, gather,
FlexQMixer plain and with groups, the lambda-mixed TD loss, loss.backward()) through the differentiable native ops,
next to the same loss in plain PyTorch on the same card (the oracle's functions, oracle/refil_ref.py, moved to the
device) and to one REFILLearner.train call (mlg_refil_train: the same loss fused, plus clipping and RMSprop).

    python scripts/refil_autograd_timing.py [--out profiles/refil_autograd/timing.json] [--B 32] [--T 101]
                                            [--iters 10] [--repeats 5]

Config 5's learner shape: batch_size 32 episodes of episode_limit 100 (T = 101 stored steps), refil_8 dims (8 agents,
16 entities, 21 actions), on a seeded random batch whose episodes are all filled (the longest case). Per side:
warm-up, then `repeats` windows of `iters` passes between two HIP events; the figure is the median window over
`iters`. The three sides alternate in one process. The loss and batch builders are those of
tests/test_gpu_refil_autograd.py. Needs a GPU; nothing falls back.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ma-league_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_gpu_refil_autograd as T  # noqa: E402


def window_ms(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=101)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("refil_autograd_timing.py needs a GPU")
    from maleague.controllers import EntityMAC
    from maleague.learners import REFILLearner
    dev = torch.device("cuda:0")
    args, b, eb, p, mp, groupA, mac, target_mac, mx, target_mx = T._loop_setup(dev, seed=3, B=a.B, T=a.T)
    for k in ("terminated", "filled"):  # every episode runs to the end: the longest case
        eb.data.transition_data[k].fill_(0 if k == "terminated" else 1)
        b[k].fill_(0 if k == "terminated" else 1)
    params = list(mac.parameters()) + list(mx.parameters())

    def native():
        loss = T._gpu_loss(args, eb, groupA, mac, target_mac, mx, target_mx)
        torch.autograd.backward([loss], inputs=params)
        return loss

    pp = {k: v.to(dev).requires_grad_(True) for k, v in p.items()}
    mpp = {k: v.to(dev).requires_grad_(True) for k, v in mp.items()}
    bb = {k: v.to(dev) for k, v in b.items()}
    gA = groupA.to(dev)

    def plain():
        loss = T._ref_loss_fn(args, bb, pp, mpp, gA)
        torch.autograd.backward([loss], inputs=list(pp.values()) + list(mpp.values()))
        return loss

    mac2 = EntityMAC(eb.scheme, eb.groups, args)
    mac2.agent.load_state_dict(mac.agent.state_dict())
    learner = REFILLearner(mac2, eb.scheme, T._Log(), args, name="home")
    learner.mixer.load_state_dict(mx.state_dict())
    learner.target_mixer.load_state_dict(mx.state_dict())
    learner.target_mac.load_state(mac2)
    learner.build_optimizer()
    args.lr = 0.0  # informational: the fused call's optimizer step leaves the weights where they are

    def fused():
        learner.train(eb, 0, 0, groupA=gA)

    l_native, l_plain = float(native().detach()), float(plain().detach())
    sides = {"native": native, "plain_torch": plain, "fused_train": fused}
    for f in sides.values():
        f(), f()
    torch.cuda.synchronize()
    win = {k: [] for k in sides}
    for _ in range(a.repeats):  # alternating windows
        for k, f in sides.items():
            win[k].append(window_ms(f, a.iters))
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": a.B, "T": a.T, "iters": a.iters,
           "repeats": a.repeats, "loss_native": l_native, "loss_plain_torch": l_plain,
           "ms": {k: statistics.median(v) for k, v in win.items()}, "windows_ms": win}
    print(" ".join(f"{k} {v:.3f} ms" for k, v in res["ms"].items()), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
