"""Oracle of prioritized episode replay: a numpy float64 restatement of mlg_per_sample / mlg_per_insert
/ mlg_per_update and of their counter RNG stream, and PERLearnerRef, oracle/learner_ref.py's QLearnerRef with the
importance-weighted loss and the per-episode errors. tests/test_per.py pins the selection rule and the weight formula
to the reference's own BinarySumTree / Memory through tests/golden/per.npz.
"""
import numpy as np
import torch

import learner_ref as LR

PER_PURPOSE = 6
E, A, BETA, BETA_INCREMENT = 0.01, 0.6, 0.4, 0.001  # the reference's defaults (Memory)
_M64 = (1 << 64) - 1


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def rng(key, ctr):
    return splitmix64((key & _M64) ^ splitmix64(ctr))


def ctr(episode, t, purpose, idx):
    return ((episode & 0xFFFFFFFF) << 32) | ((t & 0xFFFF) << 16) | ((purpose & 0xF) << 12) | (idx & 0xFFF)


def u01(r):
    return float(np.float32(r >> 40) * np.float32(1.0 / 16777216.0))


def uniforms(seed, draw, B):
    """u_i of draw `draw`: mlg_u01(mlg_rng(seed, mlg_ctr(draw, 0, PER_PURPOSE, i)))."""
    return np.asarray([u01(rng(seed, ctr(draw, 0, PER_PURPOSE, i))) for i in range(B)], dtype=np.float64)


def select(cum, s):
    """The first slot, in slot order, whose inclusive cumulative priority is >= s (BinarySumTree._retrieve: s <= left
    goes left); the last slot if none is."""
    return np.minimum(np.searchsorted(cum, s, side="left"), len(cum) - 1).astype(np.int64)


def weights(n_live, p, total, beta):
    """Memory.sample's importance weights: (n p / total)^-beta over their maximum."""
    w = np.power(n_live * (np.asarray(p, dtype=np.float64) / total), -beta)
    return w / w.max()


def strata(total, u, B):
    return (np.arange(B, dtype=np.float64) + u) * total / float(B)


def sample(prio, n_live, B, seed, draw, beta):
    """-> rows [B] int64, is_weight [B] float64, margin: the smallest distance of a draw to a cumulative boundary
    relative to the total (a draw closer than ~1e-9 is a near tie: an fp64 scan in another order may pick the
    neighbour)."""
    p = np.asarray(prio[:n_live], dtype=np.float64)
    cum = np.cumsum(p)
    total = cum[-1]
    s = strata(total, uniforms(seed, draw, B), B)
    rows = select(cum, s)
    margin = float(np.min(np.abs(cum[None, :] - s[:, None]))) / total if n_live * B <= 1 << 24 else \
        neighbour_margin(cum, s, rows) / total
    return rows, weights(n_live, p[rows], total, beta), margin


def neighbour_margin(cum, s, rows):
    """min over the draws of the distance to the nearest cumulative boundary, from each draw's two neighbouring
    boundaries only: cum is non-decreasing and cum[r - 1] < s <= cum[r] for the selected slot r, so no other boundary
    is nearer (a draw past the last boundary has that one alone). The value of the full O(B n) minimum in O(B)."""
    up = np.abs(cum[rows] - s)
    down = np.where(rows > 0, np.abs(s - cum[np.maximum(rows - 1, 0)]), np.inf)
    return float(np.min(np.minimum(up, down)))


def priority(err, e=E, a=A):
    return np.power(np.abs(np.asarray(err, dtype=np.float64)) + e, a)


def insert(prio, max_p, slot0, count, errors=None, e=E, a=A):
    """In place on the float64 vector `prio`; -> the new maximum."""
    idx = (slot0 + np.arange(count)) % len(prio)
    if errors is None:
        prio[idx] = max_p
        return max_p
    p = priority(errors, e, a).astype(np.float32).astype(np.float64)
    prio[idx] = p
    return max(max_p, float(p.max()))


def update(prio, max_p, rows, td_abs, e=E, a=A):
    p = priority(td_abs, e, a).astype(np.float32).astype(np.float64)
    prio[np.asarray(rows, dtype=np.int64)] = p
    return max(max_p, float(p.max()))


class PERLearnerRef(LR.QLearnerRef):
    """QLearnerRef with loss = sum_b w_b sum_t (mask td)^2 / sum(mask) and td_abs[b] = sum |mask td| / sum mask of the
    episode (0 where it has no masked step; for IQL both sums run over the agents as well). The statistics stay
    unweighted. `is_weight` [B] (None = ones) is read per call; `last_td_abs` [B] is set by it. _train restates
    QLearnerRef._train line for line up to the loss."""
    is_weight = None
    last_td_abs = None

    def _train(self, batch, t_env, episode_num):
        a = self.args
        N = a.n_agents
        rewards = batch["reward"][:, :-1]
        actions = batch["actions"][:, :-1]
        terminated = batch["terminated"][:, :-1].float()
        mask = batch["filled"][:, :-1].float()
        mask[:, 1:] = mask[:, 1:] * (1 - terminated[:, :-1])
        avail = batch["avail_actions"]
        T = batch["obs"].shape[1]
        mac_out, _ = LR.mac_unroll(self.p, batch, N, T, last_action=a.obs_last_action, agent_id=a.obs_agent_id)
        chosen = torch.gather(mac_out[:, :-1], dim=3, index=actions).squeeze(3)
        with torch.no_grad():
            tmac, _ = LR.mac_unroll(self.tp, batch, N, T, last_action=a.obs_last_action, agent_id=a.obs_agent_id)
        tmac = tmac[:, 1:].clone()
        tmac[avail[:, 1:] == 0] = -9999999
        if a.double_q:
            md = mac_out.clone().detach()
            md[avail == 0] = -9999999
            cur_max = md[:, 1:].max(dim=3, keepdim=True)[1]
            target_max = torch.gather(tmac, 3, cur_max).squeeze(3)
        else:
            target_max = tmac.max(dim=3)[0]
        if self.mixer in ("qmix", "vdn"):
            chosen = self._mix(self.mp, chosen, batch["state"][:, :-1])
            with torch.no_grad():
                target_max = self._mix(self.tmp, target_max, batch["state"][:, 1:])
        targets = rewards + a.gamma * (1 - terminated) * target_max
        td = chosen - targets.detach()
        mask = mask.expand_as(td)
        mtd = td * mask
        B = mtd.shape[0]
        w = torch.ones(B, dtype=mtd.dtype) if self.is_weight is None else \
            torch.as_tensor(np.asarray(self.is_weight), dtype=mtd.dtype)
        loss = (w.view(B, 1, 1) * mtd ** 2).sum() / mask.sum()
        with torch.no_grad():
            ms = mask.sum(dim=(1, 2))
            self.last_td_abs = torch.where(ms > 0, mtd.abs().sum(dim=(1, 2)) / ms.clamp(min=1), torch.zeros_like(ms))
        self.opt.zero_grad()
        loss.backward()
        self.last_grads = [p.grad.detach().clone() for p in self.params]
        grad_norm = torch.nn.utils.clip_grad_norm_(self.params, a.grad_norm_clip)
        self.opt.step()
        if (episode_num - self.last_target_update_episode) / a.target_update_interval >= 1.0:
            self.update_targets()
            self.last_target_update_episode = episode_num
        self.trained_steps += int(torch.count_nonzero(mask))
        me = mask.sum().item()
        return {"loss": loss.item(), "grad_norm": float(grad_norm), "td_error_abs": mtd.abs().sum().item() / me,
                "q_taken_mean": (chosen * mask).sum().item() / (me * N),
                "target_mean": (targets * mask).sum().item() / (me * N)}


def per_ref_class(base):
    """`base` (QLearnerRef or a subclass that swaps the MAC unroll around super()._train, as dqn_ref.DQNLearnerRef and
    distinct_ref.DistinctLearnerRef do) with the weighted _train next in its method resolution order."""
    if base is LR.QLearnerRef:
        return PERLearnerRef
    return type("PER" + base.__name__, (base, PERLearnerRef), {})
