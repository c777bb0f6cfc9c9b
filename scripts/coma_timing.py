"""Times of the COMA path on one GPU.

    python scripts/coma_timing.py [--out profiles/coma] [--commit <hash>] [--repeats 10]

Shape: 5v5 `medium_1h_4t`, H = 64, episode_limit 100, grid 20, the values of algs/coma.yaml.

  rollout   HIP events around the single launch of one ParallelStepper.run (stepper.timing): `mlg_rollout_policy`
            (pi_logits MAC, multinomial draw, train mode) next to `mlg_rollout` (Q MAC, epsilon-greedy, default kernel
            for the shape) at B = 8 and B = 4096. Warm-up runs, then `repeats` runs of each, alternating; median.
  learner   one COMALearner.train on a B = 8 rollout batch truncated to its longest episode, next to an eager fp32
            torch restatement of the same step on the same GPU (nn.Linear critic, GRUCell agent, autograd,
            torch.optim.RMSprop; one optimizer step per timestep, as the algorithm prescribes). HIP events around
            the whole call, ending in a synchronise, host work included; warm-up, then `repeats` alternating windows;
            median. Both start every window from the same parameters.

Needs a GPU; nothing falls back."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ma-league_amd"))


def build(alg, B, dev, episode_limit=100):
    from maleague.components.episode_batch import EpisodeBatch
    from maleague.components.transforms import OneHot
    from maleague.controllers import BasicMAC
    from maleague.custom_logging import MainLogger
    from maleague.steppers import ParallelStepper
    from maleague.utils.config import build_config, to_args
    cfg = build_config(alg, "ma", overrides=[f"batch_size_run={B}", "runner=parallel", "buffer_cpu_only=False",
                                             f"env_args.episode_limit={episode_limit}", "show_exp_parameters=False",
                                             "learner_log_interval=1000000000", "seed=0"])
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
    return stepper, mac, args, proto.scheme


def time_rollouts(dev, repeats):
    out = {}
    for B in (8, 4096):
        steppers = {alg: build(alg, B, dev)[0] for alg in ("coma", "qmix")}
        for st in steppers.values():
            st.t_env = 50000
            for _ in range(3):
                st.run(test_mode=False)
            st.flush()
            st.timing = []
        for _ in range(repeats):
            for st in steppers.values():
                st.run(test_mode=False)
                st.flush()
        torch.cuda.synchronize()
        for alg, st in steppers.items():
            ms = [a.elapsed_time(b) for a, b in st.timing]
            out[f"{'mlg_rollout_policy' if alg == 'coma' else 'mlg_rollout'}.B{B}"] = {
                "ms": ms, "median_ms": statistics.median(ms), "mean_ep_len": float(st.last_run["ep_len"].float().mean())}
    return out


class EagerComa:
    """The COMA train step in eager fp32 torch ops (the algorithm of the COMA paper as the reference arranges it)."""

    def __init__(self, agent_sd, critic_sd, args, D):
        dev, H, A = args.device, args.rnn_hidden_dim, args.n_actions
        self.a = args
        self.fc1 = torch.nn.Linear(agent_sd["fc1.weight"].shape[1], H, device=dev)
        self.gru = torch.nn.GRUCell(H, H, device=dev)
        self.fc2 = torch.nn.Linear(H, A, device=dev)
        self.agent = torch.nn.ModuleDict({"fc1": self.fc1, "gru": self.gru, "fc2": self.fc2})
        self.agent.load_state_dict(agent_sd)
        self.critic = torch.nn.Sequential(torch.nn.Linear(D, 128), torch.nn.ReLU(), torch.nn.Linear(128, 128),
                                          torch.nn.ReLU(), torch.nn.Linear(128, A)).to(dev)
        for (k, v), p in zip(critic_sd.items(), self.critic.parameters()):
            p.data.copy_(v)
        self.target = copy.deepcopy(self.critic)
        kw = dict(alpha=args.optim_alpha, eps=args.optim_eps)
        self.a_opt = torch.optim.RMSprop(self.agent.parameters(), lr=args.lr, **kw)
        self.c_opt = torch.optim.RMSprop(self.critic.parameters(), lr=args.critic_lr, **kw)

    def critic_in(self, b, t):
        oh = b["actions_onehot"]
        B, _, N, A = oh.shape
        ts = slice(None) if t is None else slice(t, t + 1)
        T = oh[:, ts].shape[1]
        joint = oh[:, ts].reshape(B, T, 1, N * A).expand(-1, -1, N, -1)
        keep = (1 - torch.eye(N, device=oh.device)).repeat_interleave(A, dim=1)
        prev = torch.cat([torch.zeros_like(oh[:, :1]), oh[:, :-1]], dim=1)[:, ts].reshape(B, T, 1, N * A)
        eye = torch.eye(N, device=oh.device).expand(B, T, N, N)
        return torch.cat([b["state"][:, ts].unsqueeze(2).expand(-1, -1, N, -1), b["obs"][:, ts], joint * keep,
                          prev.expand(-1, -1, N, -1), eye], dim=-1)

    def train(self, b, eps, mask_before_softmax):
        a = self.a
        B, T, N, A = b["actions_onehot"].shape
        term = b["terminated"][:, :-1].float()
        mask = b["filled"][:, :-1].float()
        mask[:, 1:] = mask[:, 1:] * (1 - term[:, :-1])
        acts = b["actions"]
        with torch.no_grad():
            tq = self.target(self.critic_in(b, None)).gather(3, acts).squeeze(3)
            ret = torch.zeros_like(tq)
            ret[:, -1] = tq[:, -1] * (1 - term.sum(1))
            for t in reversed(range(T - 1)):
                ret[:, t] = a.td_lambda * a.gamma * ret[:, t + 1] + mask[:, t] * (
                    b["reward"][:, t] + (1 - a.td_lambda) * a.gamma * tq[:, t + 1] * (1 - term[:, t]))
        q_vals = torch.zeros(B, T - 1, N, A, device=tq.device)
        for t in reversed(range(T - 1)):
            mt = mask[:, t].expand(-1, N)
            if mt.sum() == 0:
                continue
            q = self.critic(self.critic_in(b, t)).squeeze(1)
            q_vals[:, t] = q.detach()
            td = (q.gather(2, acts[:, t]).squeeze(2) - ret[:, t]) * mt
            self.c_opt.zero_grad()
            ((td ** 2).sum() / mt.sum()).backward()
            torch.nn.utils.clip_grad_norm_(self.critic.parameters(), a.grad_norm_clip)
            self.c_opt.step()
        h = torch.zeros(B * N, a.rnn_hidden_dim, device=tq.device)
        eye = torch.eye(N, device=tq.device).expand(B, N, N)
        pis = []
        for t in range(T - 1):
            last = torch.zeros_like(b["actions_onehot"][:, 0]) if t == 0 else b["actions_onehot"][:, t - 1]
            x = torch.cat([b["obs"][:, t], last, eye], dim=-1).reshape(B * N, -1)
            h = self.gru(F.relu(self.fc1(x)), h)
            logits = self.fc2(h).view(B, N, A)
            av = b["avail_actions"][:, t]
            if mask_before_softmax:
                logits = logits.masked_fill(av == 0, -1e10)
            p = torch.softmax(logits, dim=-1)
            K = av.sum(-1, keepdim=True).float() if mask_before_softmax else float(A)
            p = (1 - eps) * p + eps / K
            pis.append(p.masked_fill(av == 0, 0.0) if mask_before_softmax else p)
        pi = torch.stack(pis, dim=1).masked_fill(b["avail_actions"][:, :-1] == 0, 0.0)
        pi = (pi / pi.sum(-1, keepdim=True)).masked_fill(b["avail_actions"][:, :-1] == 0, 0.0)
        m = mask.expand(-1, -1, N)
        base = (pi * q_vals).sum(-1).detach()
        adv = (q_vals.gather(3, acts[:, :-1]).squeeze(3) - base).detach()
        pt = torch.where(m == 0, torch.ones_like(m), pi.gather(3, acts[:, :-1]).squeeze(3))
        loss = -(torch.log(pt) * adv * m).sum() / m.sum()
        self.a_opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.agent.parameters(), a.grad_norm_clip)
        self.a_opt.step()
        return loss.detach()


def time_learner(dev, repeats):
    from maleague.custom_logging import MainLogger
    from maleague.learners import COMALearner
    stepper, mac, args, scheme = build("coma", 8, dev)
    batch, _ = stepper.run(test_mode=False)
    stepper.flush()
    T = int(batch.max_t_filled())
    sample = batch[:, :T]
    learner = COMALearner(mac, scheme, MainLogger(), args, name="home")
    learner.build_optimizer()
    agent0 = {k: v.clone() for k, v in mac.agent.state_dict().items()}
    critic0 = {k: v.clone() for k, v in learner.critic.state_dict().items()}
    eager = EagerComa(agent0, critic0, args, learner.critic.input_shape)
    eager0 = (copy.deepcopy(eager.agent.state_dict()), copy.deepcopy(eager.critic.state_dict()))
    data = {k: v for k, v in sample.data.transition_data.items()}
    eps = float(mac.action_selector.epsilon)

    def reset():
        mac.agent.load_state_dict(agent0)
        learner.critic.load_state_dict(critic0)
        learner.target_critic.load_state_dict(critic0)
        learner._sq.zero_()
        eager.agent.load_state_dict(eager0[0])
        eager.critic.load_state_dict(eager0[1])
        eager.target.load_state_dict(eager0[1])

    routes = {"COMALearner.train": lambda: learner.train(sample, 0, 0),
              "eager_torch_fp32": lambda: eager.train(data, eps, bool(args.mask_before_softmax))}
    res = {k: [] for k in routes}
    for it in range(2 + repeats):
        for k, fn in routes.items():
            reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= 2:
                res[k].append(a.elapsed_time(b))
    out = {k: {"ms": v, "median_ms": statistics.median(v)} for k, v in res.items()}
    out["timesteps"] = T
    out["critic_steps_taken"] = float(learner._cstats[5])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coma"))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("coma_timing needs a ROCm GPU")
    dev = torch.device("cuda:0")
    summary = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
               "rollout": time_rollouts(dev, a.repeats), "learner": time_learner(dev, a.repeats)}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "timing.json"), "w") as f:
        json.dump(summary, f, indent=2)
    brief = {k: round(v["median_ms"], 4) for k, v in summary["rollout"].items()}
    brief.update({k: round(v["median_ms"], 3) for k, v in summary["learner"].items() if isinstance(v, dict) and "median_ms" in v})
    brief.update(timesteps=summary["learner"]["timesteps"], critic_steps=summary["learner"]["critic_steps_taken"])
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
