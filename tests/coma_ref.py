"""A float64 restatement of COMA, written for the tests: the critic's input rows, the critic MLP with its hand-written
backward, TD(lambda) targets, the sequential critic steps (clip_grad_norm_ + RMSprop), the policy softmax with the
epsilon floor, the actor loss, and (in fp32, as the kernels) the multinomial draw on the oracle's counter RNG.
tests/test_coma_ref.py pins it to the golden fixtures (tests/golden/coma_*.npz) on the CPU."""
import numpy as np

CRITIC_KEYS = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias"]
PURPOSE_POLICY = 5


def f64(d, dtype=np.float64):
    return {k: np.asarray(v, dtype=dtype) for k, v in d.items()}


def critic_inputs(batch, t, dtype=np.float64):
    """[B, N, D] rows of timestep t: [state | obs_n | joint one-hot actions at t, agent n's block zeroed | joint one-hot
    actions at t - 1 (zeros at t = 0) | eye row n]."""
    oh = np.asarray(batch["actions_onehot"], dtype=dtype)
    B, _, N, A = oh.shape
    state = np.repeat(np.asarray(batch["state"], dtype=dtype)[:, t][:, None, :], N, axis=1)
    obs = np.asarray(batch["obs"], dtype=dtype)[:, t]
    joint = np.repeat(oh[:, t].reshape(B, 1, N * A), N, axis=1)
    keep = np.repeat(1.0 - np.eye(N, dtype=dtype), A, axis=1)  # [N, N * A]
    last = np.zeros((B, N, N * A), dtype) if t == 0 else np.repeat(oh[:, t - 1].reshape(B, 1, N * A), N, axis=1)
    eye = np.repeat(np.eye(N, dtype=dtype)[None], B, axis=0)
    return np.concatenate([state, obs, joint * keep[None], last, eye], axis=-1)


DENSE_KB = 32  # coma.hip's dense16 adds its inputs in chains of this length and then the chains, in ascending order


def mm_ascending(a, b, bias=None, fused=False, block=None):
    """a [..., K] @ b [K, O] (+ bias) with the products added one k at a time in ascending order, in a's dtype: the
    order of the kernels' sums (a dot product over the inputs, a weight gradient over the rows). fused: each step is one
    fused multiply-add (the product is exact in float64; rounded once, to a's dtype), as the matrix instructions of
    the kernels' dense layers; else the product is rounded before the add, as their gradient sums. block: the terms
    go ``block`` at a time into a chain that starts at zero and is then added to the total (dense16's blocked sum)."""
    if block is not None:
        acc = np.zeros(a.shape[:-1] + (b.shape[1],), a.dtype) + (0 if bias is None else bias)
        for k0 in range(0, a.shape[-1], block):
            acc = acc + mm_ascending(a[..., k0:k0 + block], b[k0:k0 + block], None, fused)
        return acc
    acc = np.zeros(a.shape[:-1] + (b.shape[1],), a.dtype) + (0 if bias is None else bias)
    for k in range(a.shape[-1]):
        if fused:
            acc = (acc.astype(np.float64) + a[..., k:k + 1].astype(np.float64) * b[k].astype(np.float64)).astype(a.dtype)
        else:
            acc = acc + a[..., k:k + 1] * b[k]
    return acc


def critic_forward(p, x, ascending=False):
    if ascending:
        h1 = np.maximum(mm_ascending(x, p["fc1.weight"].T, p["fc1.bias"], True, DENSE_KB), 0)
        h2 = np.maximum(mm_ascending(h1, p["fc2.weight"].T, p["fc2.bias"], True, DENSE_KB), 0)
        return h1, h2, mm_ascending(h2, p["fc3.weight"].T, p["fc3.bias"], True, DENSE_KB)
    h1 = np.maximum(x @ p["fc1.weight"].T + p["fc1.bias"], 0.0)
    h2 = np.maximum(h1 @ p["fc2.weight"].T + p["fc2.bias"], 0.0)
    return h1, h2, h2 @ p["fc3.weight"].T + p["fc3.bias"]


def masks(batch, dtype=np.float64):
    """mask [B, T-1] = filled, times 1 - terminated of the step before (coma_learner.py:53-55)."""
    term = np.asarray(batch["terminated"], dtype=dtype)[:, :-1, 0]
    m = np.asarray(batch["filled"], dtype=dtype)[:, :-1, 0].copy()
    m[:, 1:] *= 1.0 - term[:, :-1]
    return m, term


def td_lambda_targets(rewards, terminated, mask, target_qs, gamma, td_lambda):
    """build_td_lambda_targets (coma_learner.py:10-21): target_qs [B, T, N], the rest [B, T-1] -> [B, T-1, N]."""
    ret = np.zeros_like(target_qs)
    ret[:, -1] = target_qs[:, -1] * (1.0 - terminated.sum(axis=1))[:, None]
    for t in reversed(range(ret.shape[1] - 1)):
        ret[:, t] = td_lambda * gamma * ret[:, t + 1] + mask[:, t, None] * (
            rewards[:, t, None] + (1.0 - td_lambda) * gamma * target_qs[:, t + 1] * (1.0 - terminated[:, t, None]))
    return ret[:, :-1]


class CriticRef:
    """COMALearner._train_critic (coma_learner.py:121-169) in float64, parameters as dicts of arrays. ``dtype``:
    np.float32 restates it in the kernels' precision (numpy's summation order), to measure the fp32 noise floor.
    ``norms``: the gradient norms before the clip of the latest train(), in the order the steps were taken.
    ``defect``: None, or one of DEFECTS -- the restatement of a kernel that forgot the second pass of a 256-wide stride
    loop, for the tests that show a comparison would notice it (tests/test_coma_shapes.py). ``ascending``: every
    matrix product adds its terms one at a time in ascending order (mm_ascending: fused in the layers, product rounded
    first in the gradient sums), as the kernels do, where numpy's products add them in blocks."""
    DEFECTS = ("stats_rows_256", "norm_blocks_256", "target_rows_256", "masks_256", "masksum_256")

    def __init__(self, params, target=None, gamma=0.99, td_lambda=0.8, lr=0.0005, alpha=0.99, eps=1e-5, clip=10.0,
                 dtype=np.float64, defect=None, ascending=False):
        self.ascending = ascending
        assert defect is None or defect in self.DEFECTS
        self.dtype, self.defect = dtype, defect
        self.norms = []
        self.p = f64(params, dtype)
        self.tp = f64(params if target is None else target, dtype)
        self.sq = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.gamma, self.td_lambda, self.lr, self.alpha, self.eps, self.clip = gamma, td_lambda, lr, alpha, eps, clip
        self.steps = 0
        self.last_update = 0

    def train(self, batch):
        """-> q_vals [B, T-1, N, A], targets [B, T-1, N], the five stat sums over the taken steps and their count."""
        acts = np.asarray(batch["actions"])[..., 0]
        B, T, N = acts.shape
        dt = self.dtype
        self.norms = []
        mask, term = masks(batch, dt)
        if self.defect == "masks_256":
            mask.reshape(-1)[256:] = 0
        if self.defect == "masksum_256":
            mask[:, 256:] = 0
        asc = self.ascending
        mm = mm_ascending if asc else (lambda a, b: a @ b)
        tq = np.stack([np.take_along_axis(critic_forward(self.tp, critic_inputs(batch, t, dt), asc)[2], acts[:, t, :, None],
                                          axis=2)[..., 0] for t in range(T)], axis=1)
        rewards = np.asarray(batch["reward"], dtype=dt)[:, :-1, 0]
        targets = td_lambda_targets(rewards, term, mask, tq, self.gamma, self.td_lambda)
        if self.defect == "target_rows_256":
            targets = np.where((np.arange(B * N).reshape(B, 1, N) >= 256), 0, targets).astype(dt)
        A = self.p["fc3.weight"].shape[0]
        q_vals = np.zeros((B, T - 1, N, A), dt)
        sums = np.zeros(5, dt)
        taken = 0
        for t in reversed(range(T - 1)):
            mt = np.repeat(mask[:, t, None], N, axis=1)
            den = mt.sum()
            if den == 0:
                continue
            x = critic_inputs(batch, t, dt)
            h1, h2, q = critic_forward(self.p, x, asc)
            q_vals[:, t] = q
            qt = np.take_along_axis(q, acts[:, t, :, None], axis=2)[..., 0]
            mtd = (qt - targets[:, t]) * mt
            loss = (mtd ** 2).sum() / den
            dq = np.zeros_like(q)
            np.put_along_axis(dq, acts[:, t, :, None], (2.0 * mtd * mt / den)[..., None], axis=2)
            d2 = (dq @ self.p["fc3.weight"]) * (h2 > 0)  # one term per row: no order
            d1 = (mm_ascending(d2, self.p["fc2.weight"], None, True, DENSE_KB) if asc else d2 @ self.p["fc2.weight"]) * (h1 > 0)
            flat2 = lambda a: a.reshape(B * N, -1)  # noqa: E731
            rowsum = (lambda a: mm(a.T, np.ones((B * N, 1), dt))[:, 0]) if asc else (lambda a: a.sum(0))
            g = {"fc3.weight": mm(flat2(dq).T, flat2(h2)), "fc3.bias": rowsum(flat2(dq)),
                 "fc2.weight": mm(flat2(d2).T, flat2(h1)), "fc2.bias": rowsum(flat2(d2)),
                 "fc1.weight": mm(flat2(d1).T, flat2(x)), "fc1.bias": rowsum(flat2(d1))}
            norm = np.sqrt(sum((v ** 2).sum() for v in g.values()))
            if self.defect == "norm_blocks_256":
                norm = np.sqrt((np.concatenate([g[k].reshape(-1) for k in CRITIC_KEYS])[:256 * 256] ** 2).sum())
            coef = min(self.clip / (norm + 1e-6), 1.0)
            self.norms.append(float(norm))
            for k in CRITIC_KEYS:
                gk = g[k] * coef
                self.sq[k] = self.alpha * self.sq[k] + (1.0 - self.alpha) * gk * gk
                self.p[k] = self.p[k] - self.lr * gk / (np.sqrt(self.sq[k]) + self.eps)
            self.steps += 1
            taken += 1
            if self.defect == "stats_rows_256":
                keep = (np.arange(B * N) < 256).reshape(B, N)
                loss, mtd, qt, mt = ((mtd * keep) ** 2).sum() / den, mtd * keep, qt * keep, mt * keep
            sums += np.array([loss, norm, np.abs(mtd).sum() / den, (qt * mt).sum() / den, (targets[:, t] * mt).sum() / den], dt)
        return q_vals, targets, sums, taken

    def maybe_update_target(self, interval):
        if (self.steps - self.last_update) / interval >= 1.0:
            self.tp = {k: v.copy() for k, v in self.p.items()}
            self.last_update = self.steps


def softmax_policy(logits, avail, eps, mask_before_softmax, test_mode):
    """MultiAgentController._softmax (multi_agent_controller.py:78-99) in float64 over [..., A]."""
    x = np.asarray(logits, dtype=np.float64).copy()
    av = np.asarray(avail) != 0
    if mask_before_softmax:
        x[~av] = -1e10
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    if not test_mode:
        K = av.sum(axis=-1, keepdims=True).astype(np.float64) if mask_before_softmax else float(x.shape[-1])
        with np.errstate(divide="ignore", invalid="ignore"):
            p = (1.0 - eps) * p + eps / K
        if mask_before_softmax:
            p[~av] = 0.0
    return p


def softmax_policy_grad(logits, avail, eps, mask_before_softmax, test_mode, g):
    """d sum(g * softmax_policy) / d logits in float64 (the masked assignments pass nothing)."""
    x = np.asarray(logits, dtype=np.float64).copy()
    av = np.asarray(avail) != 0
    off = ~av if mask_before_softmax else np.zeros_like(av)
    x[off] = -1e10
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    y = e / e.sum(axis=-1, keepdims=True)
    dy = np.asarray(g, dtype=np.float64) * (1.0 if test_mode else 1.0 - eps)
    if not test_mode:
        dy = np.where(off, 0.0, dy)
    dx = y * (dy - (dy * y).sum(axis=-1, keepdims=True))
    return np.where(off, 0.0, dx)


def actor_loss_torch(pi, avail, actions, q_vals, mask):
    """coma_learner.py:75-96 on torch tensors (any dtype; differentiable in pi): -> loss, advantage_mean, pi_max mean,
    the sum of the expanded mask. pi / avail / q_vals [B, T-1, N, A], actions [B, T-1, N, 1], mask [B, T-1, 1]."""
    import torch
    N, A = pi.shape[2], pi.shape[3]
    m = mask.repeat(1, 1, N).view(-1)
    mac_out = pi.clone()
    mac_out[avail == 0] = 0
    mac_out = mac_out / mac_out.sum(dim=-1, keepdim=True)
    mac_out[avail == 0] = 0
    q = q_vals.reshape(-1, A)
    p = mac_out.view(-1, A)
    baseline = (p * q).sum(dim=-1).detach()
    q_taken = torch.gather(q, dim=1, index=actions.reshape(-1, 1)).squeeze(1)
    pi_taken = torch.gather(p, dim=1, index=actions.reshape(-1, 1)).squeeze(1)
    pi_taken[m == 0] = 1.0
    adv = (q_taken - baseline).detach()
    loss = -((torch.log(pi_taken) * adv) * m).sum() / m.sum()
    return loss, (adv * m).sum() / m.sum(), (p.max(dim=1)[0] * m).sum() / m.sum(), m.sum()


def select_multinomial(probs, avail, key, episode, t, agent, greedy=False):
    """The draw rule of mlg_select_multinomial in fp32 on the oracle's counter RNG: the first available k whose running
    fp32 sum of m_k exceeds u * total, else the last available k; greedy: the first available k of the largest m_k."""
    import envref
    p = np.asarray(probs, dtype=np.float32)
    on = np.asarray(avail) != 0
    idx = np.nonzero(on)[0]
    if len(idx) == 0:
        return 0
    if greedy:
        return int(idx[np.argmax(p[idx])])
    total = np.float32(0.0)
    for k in idx:
        total = np.float32(total + p[k])
    u = np.float32(envref.u01(envref.rng(key, envref.ctr(episode, t, PURPOSE_POLICY, agent))))
    thr = np.float32(u * total)
    run = np.float32(0.0)
    for k in idx:
        run = np.float32(run + p[k])
        if run > thr:
            return int(k)
    return int(idx[-1])


def policy_u(key, episode, t, agent):
    import envref
    return np.float32(envref.u01(envref.rng(key, envref.ctr(episode, t, PURPOSE_POLICY, agent))))


def softmax_policy_torch(logits, avail, eps, mask_before_softmax, test_mode=False):
    """softmax_policy on torch tensors (differentiable in the logits, as the reference's in-place form)."""
    import torch
    x = logits.clone()
    off = avail == 0
    if mask_before_softmax:
        x[off] = -1e10
    p = torch.softmax(x, dim=-1)
    if not test_mode:
        K = (~off).sum(dim=-1, keepdim=True).to(p.dtype) if mask_before_softmax else float(x.shape[-1])
        p = (1 - eps) * p + eps / K
        if mask_before_softmax:
            p = p.masked_fill(off, 0.0)
    return p


class LearnerRef:
    """COMALearner.train (coma_learner.py:49-119) in float64: CriticRef, then the MAC unroll (oracle/learner_ref.py),
    the policy softmax, the actor loss, clip_grad_norm_ and RMSprop of the agent, and the target-critic update."""

    def __init__(self, agent_params, critic_params, n_agents, epsilon, mask_before_softmax, lr=0.0005, critic_lr=0.0005,
                 alpha=0.99, opt_eps=1e-5, clip=10.0, gamma=0.99, td_lambda=0.8, target_update_interval=200,
                 dtype=np.float64):
        import torch
        self.critic = CriticRef(critic_params, gamma=gamma, td_lambda=td_lambda, lr=critic_lr, alpha=alpha, eps=opt_eps,
                                clip=clip, dtype=dtype)
        self.dtype = dtype
        self.tdtype = torch.float64 if dtype == np.float64 else torch.float32
        self.agent = {k: torch.tensor(np.asarray(v), dtype=self.tdtype, requires_grad=True)
                      for k, v in agent_params.items()}
        self.sq = {k: torch.zeros_like(v) for k, v in self.agent.items()}
        self.N, self.epsilon, self.mask = n_agents, epsilon, mask_before_softmax
        self.lr, self.alpha, self.opt_eps, self.clip, self.interval = lr, alpha, opt_eps, clip, target_update_interval

    def train(self, batch):
        """-> dict of the nine stats, q_vals, targets."""
        import torch
        import learner_ref as LR
        q_vals, targets, sums, taken = self.critic.train(batch)
        B, T = batch["obs"].shape[:2]
        tb = {"obs": torch.tensor(batch["obs"], dtype=self.tdtype),
              "actions_onehot": torch.tensor(batch["actions_onehot"], dtype=self.tdtype)}
        H = self.agent["gru.weight_hh"].shape[1]
        h0 = torch.zeros(B * self.N, H, dtype=self.tdtype)
        for v in self.agent.values():
            v.grad = None
        logits, _ = LR.mac_unroll({k: v for k, v in self.agent.items()}, tb, self.N, T=T - 1, h0=h0)
        avail = torch.tensor(batch["avail_actions"][:, :-1])
        pi = softmax_policy_torch(logits, avail, self.epsilon, self.mask)
        m, _ = masks(batch, self.dtype)
        loss, adv, pimax, _ = actor_loss_torch(pi, avail, torch.tensor(batch["actions"][:, :-1]),
                                               torch.tensor(q_vals), torch.tensor(m)[..., None])
        loss.backward()
        norm = torch.sqrt(sum((v.grad ** 2).sum() for v in self.agent.values()))
        coef = min(self.clip / (float(norm) + 1e-6), 1.0)
        with torch.no_grad():
            for k, v in self.agent.items():
                g = v.grad * coef
                self.sq[k] = self.alpha * self.sq[k] + (1 - self.alpha) * g * g
                v -= self.lr * g / (self.sq[k].sqrt() + self.opt_eps)
        self.critic.maybe_update_target(self.interval)
        stats = {k: sums[i] / taken for i, k in enumerate(["critic_loss", "critic_grad_norm", "td_error_abs",
                                                            "q_taken_mean", "target_mean"])} if taken else {}
        stats.update(advantage_mean=float(adv.detach()), coma_loss=float(loss.detach()),
                     agent_grad_norm=float(norm.detach()), pi_max=float(pimax.detach()))
        return stats, q_vals, targets
