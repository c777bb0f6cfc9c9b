"""Forward + backward time of the differentiable agent and mixer ops next to the same computation in plain
PyTorch on the same card (the oracle's functions, oracle/learner_ref.py, moved to the device).

    python scripts/autograd_timing.py [--out profiles/autograd/timing.json] [--iters 500] [--repeats 5]

Per case: warm-up, then `repeats` windows of `iters` forward + backward passes each between two HIP events; the
figure is the median window over `iters`. Both sides are timed in the same process, alternating, on the same seeded
inputs. The loss is sum(q gq) + sum(h' gh) for the agent (5v5 dims: d_obs 80, A 15, N 5, H 64) at R = 160 and
R = 20480, and sum(q_tot g) for the two-layer mixer (S 60, E 32, HE 64) at R = 3200; the forward alone (no_grad) is
timed the same way, to split the figure. Needs a GPU; nothing falls back.
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ma-league_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import learner_ref as LR  # noqa: E402
from maleague.modules.agents.drqn_agent import DRQNAgentNetwork  # noqa: E402
from maleague.modules.mixers import QMixer  # noqa: E402

N, A, H, D_OBS, S, E, HE = 5, 15, 64, 80, 60, 32, 64


def window_ms(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def time_pair(native, plain, iters, repeats, warmup=20):
    for _ in range(warmup):
        native(), plain()
    torch.cuda.synchronize()
    tn, tp = [], []
    for _ in range(repeats):  # alternating windows
        tn.append(window_ms(native, iters))
        tp.append(window_ms(plain, iters))
    return {"native_ms": statistics.median(tn), "torch_ms": statistics.median(tp), "native_windows_ms": tn,
            "torch_windows_ms": tp}


def no_grad(fn):
    def run():
        with torch.no_grad():
            fn()
    return run


def agent_case(R, dev):
    args = SimpleNamespace(n_agents=N, n_actions=A, rnn_hidden_dim=H, obs_last_action=True, obs_agent_id=True,
                           device=dev)
    torch.manual_seed(0)
    ag = DRQNAgentNetwork(D_OBS + A + N, args).enable_autograd()
    ref = {k: v.detach().clone().requires_grad_(True) for k, v in ag.state_dict().items()}
    x, h = torch.randn(R, D_OBS + A + N, device=dev), torch.randn(R, H, device=dev) * 0.5
    gq, gh = torch.randn(R, A, device=dev), torch.randn(R, H, device=dev)
    params = list(ag.parameters())

    def native():
        q, hn = ag(x, h)
        torch.autograd.backward([q, hn], [gq, gh], inputs=params)

    def plain():
        q, hn = LR.drqn_forward(ref, x, h)
        torch.autograd.backward([q, hn], [gq, gh], inputs=list(ref.values()))

    return native, plain, no_grad(lambda: ag(x, h)), no_grad(lambda: LR.drqn_forward(ref, x, h))


def mixer_case(R, dev):
    args = SimpleNamespace(n_agents=N, state_shape=S, mixing_embed_dim=E, hypernet_layers=2, hypernet_embed=HE,
                           device=dev)
    torch.manual_seed(0)
    mx = QMixer(args).enable_autograd()
    ref = {k: v.detach().clone().requires_grad_(True) for k, v in mx.state_dict().items()}
    qs = (torch.randn(R, 1, N, device=dev) * 1.5).requires_grad_(True)
    st, g = torch.randn(R, 1, S, device=dev), torch.randn(R, 1, 1, device=dev)
    params = list(mx.parameters()) + [qs]

    def native():
        torch.autograd.backward([mx(qs, st)], [g], inputs=params)

    def plain():
        torch.autograd.backward([LR.qmix_forward(ref, qs, st, N, E, 2)], [g], inputs=list(ref.values()) + [qs])

    return native, plain, no_grad(lambda: mx(qs, st)), no_grad(lambda: LR.qmix_forward(ref, qs, st, N, E, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("autograd_timing.py needs a GPU")
    dev = "cuda"
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters,
           "repeats": a.repeats, "cases": {}}
    for name, make in (("agent_R160", lambda: agent_case(160, dev)), ("agent_R20480", lambda: agent_case(20480, dev)),
                       ("mixer_R3200", lambda: mixer_case(3200, dev))):
        native, plain, native_fwd, plain_fwd = make()
        c = res["cases"][name] = time_pair(native, plain, a.iters, a.repeats)
        c["forward_only"] = time_pair(native_fwd, plain_fwd, a.iters, a.repeats)  # the same modules under no_grad
        print(f"{name}: forward+backward native {c['native_ms']:.4f} ms, plain PyTorch {c['torch_ms']:.4f} ms; "
              f"forward only {c['forward_only']['native_ms']:.4f} / {c['forward_only']['torch_ms']:.4f} ms", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
