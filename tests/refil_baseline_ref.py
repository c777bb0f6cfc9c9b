"""CPU restatement (PyTorch fp32, autograd) of the REFIL learner's two attention baselines, on top of
oracle/refil_ref.py: REFILLearner.train (marl/learners/refil_learner.py:67-202) with the plain entity agent
(:107-110) and FlexQMixer (:152-155, attention-QMIX) or VDNMixer (vdn.py:9, attention-VDN).

TEST INFRASTRUCTURE ONLY: the checker of tests/test_gpu_refil_baselines.py; pinned against
tests/golden/refil_attn_qmix.npz / refil_attn_vdn.npz (generated from the reference itself by
tests/golden/make_refil_baseline_golden.py) in tests/test_refil_baseline_ref.py.
"""
from __future__ import annotations

import torch

import refil_ref as RR


class REFILBaselineRef(RR.REFILLearnerRef):
    """The non-imagine branch: one online MAC unroll, no groups, loss = the masked TD loss (no lambda); RMSprop
    and the target update as REFILLearnerRef, with its ``dtype``, ``last_grads`` and entity_last_action handling.
    args.mixer in {"flex_qmix", "vdn"}; vdn: mixer_p empty."""

    def __init__(self, agent_p, mixer_p, args, dtype=torch.float32):
        if args.mixer not in ("flex_qmix", "vdn"):
            raise ValueError(f"mixer {args.mixer!r}")
        super().__init__(agent_p, {} if args.mixer == "vdn" else mixer_p, args, dtype=dtype)

    def mix(self, p, qs, ins):
        if self.args.mixer == "vdn":
            return qs.sum(dim=2, keepdim=True)
        return RR.flex_qmix(p, qs, *ins, self.args)

    def train(self, batch, episode_num):
        a = self.args
        batch = self.cast(batch)
        rewards = batch["reward"][:, :-1]
        actions = batch["actions"][:, :-1]
        terminated = batch["terminated"][:, :-1].to(self.dtype)
        mask = batch["filled"][:, :-1].to(self.dtype)
        mask[:, 1:] = mask[:, 1:] * (1 - terminated[:, :-1])
        avail = batch["avail_actions"]
        mac_out, _ = RR.mac_forward(self.agent, batch, a, groupA=None)
        chosen = torch.gather(mac_out[:, :-1], dim=3, index=actions).squeeze(3)
        with torch.no_grad():
            tq, _ = RR.mac_forward(self.t_agent, batch, a, groupA=None)
        tq = tq[:, 1:].clone()
        tq[avail[:, 1:] == 0] = -9999999
        if a.double_q:
            mo = mac_out.clone().detach()
            mo[avail == 0] = -9999999
            cur = mo[:, 1:].max(dim=3, keepdim=True)[1]
            tmax = torch.gather(tq, 3, cur).squeeze(3)
        else:
            tmax = tq.max(dim=3)[0]
        mix_ins, targ_ins = self.mixer_ins(batch)
        chosen = self.mix(self.mixer, chosen, mix_ins)
        with torch.no_grad():
            tmax = self.mix(self.t_mixer, tmax, targ_ins)
        targets = rewards + a.gamma * (1 - terminated) * tmax
        td = chosen - targets.detach()
        mask = mask.expand_as(td)
        mtd = td * mask
        loss = (mtd ** 2).sum() / mask.sum()
        self.opt.zero_grad()
        loss.backward()
        self.keep_grads()
        gn = torch.nn.utils.clip_grad_norm_(self.params, a.grad_norm_clip)
        self.opt.step()
        if (episode_num - self.last_target_update_episode) / a.target_update_interval >= 1.0:
            self.t_agent = {k: v.detach().clone() for k, v in self.agent.items()}
            self.t_mixer = {k: v.detach().clone() for k, v in self.mixer.items()}
            self.last_target_update_episode = episode_num
        me = mask.sum().item()
        return {"loss": loss.item(), "grad_norm": float(gn), "td_error_abs": mtd.abs().sum().item() / me,
                "q_taken_mean": (chosen * mask).sum().item() / (me * a.n_agents),
                "target_mean": (targets * mask).sum().item() / (me * a.n_agents)}
