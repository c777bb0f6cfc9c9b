"""Generate the COMA golden vectors from the reference (PMatthaei/ma-league).

TEST INFRASTRUCTURE ONLY, as make_golden.py: runs where the reference is mounted read-only, imports its Python modules
and records their inputs / outputs as .npz fixtures (data only, no reference source text).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_coma_golden.py

Fixtures:
  coma_policy.npz          MultiAgentController._softmax       src/marl/controllers/multi_agent_controller.py:78-99
                           (both mask_before_softmax settings x train / test mode) and the values of
                           src/config/algs/coma.yaml (key "coma_yaml", a JSON string)
  coma_learner_mask.npz    COMALearner.train, 3 consecutive calls, mask_before_softmax True / False
  coma_learner_nomask.npz  src/marl/learners/coma_learner.py:49-169, src/marl/modules/critics/coma.py:22-73
      b.*                  the batch (make_golden.make_batch: B=4, T=7, N=5, d_obs=80, A=15, S=60, lengths [6,3,4,2])
      p0.agent.* p0.critic.*   initial parameters
      stat{i}.*            the nine stats of call i (critic stats: means over the taken steps)
      q_vals{i} targets{i} _train_critic's q_vals [B,T-1,N,A] and build_td_lambda_targets' output [B,T-1,N]
      sub{i}.agent / .critic / .target_critic   every 16th element of the flat parameters after call i
                           (target_update_interval = 10 and 6 critic steps per call: the one target update fires at
                           the end of call 2, so sub1.target_critic = sub1.critic = sub2.target_critic)
      p3.agent.* p3.critic.*   the parameters after call 3
      steps{i} last_update{i}  critic_training_steps / last_target_update_step after call i
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as MG  # noqa: E402  (puts the reference on sys.path)

import torch as th  # noqa: E402
import yaml  # noqa: E402

from marl.controllers.basic_controller import BasicMAC  # noqa: E402
import marl.learners.coma_learner as ref_coma  # noqa: E402

OUT = HERE
STATS = ["critic_loss", "critic_grad_norm", "td_error_abs", "q_taken_mean", "target_mean", "advantage_mean", "coma_loss",
         "agent_grad_norm", "pi_max"]
SUB = 16


def coma_yaml():
    with open(os.path.join(MG.REF_SRC, "config", "algs", "coma.yaml")) as f:
        return yaml.safe_load(f)


def coma_args(**kw):
    cfg = coma_yaml()
    cfg.pop("env_args", None)
    a = dict(agent_output_type="pi_logits", action_selector="multinomial", critic_lr=0.0005, td_lambda=0.8,
             target_update_interval=10, test_greedy=True)
    for k in ("epsilon_start", "epsilon_finish", "epsilon_anneal_time", "lr", "critic_lr", "td_lambda", "q_nstep",
              "critic_train_mode"):
        a[k] = cfg[k]
    a.update(kw)
    return MG.base_args(**a)


def flat(module):
    return th.cat([p.detach().reshape(-1) for p in module.parameters()]).numpy().copy()


def learner_fixture(tag, mask_before_softmax):
    th.manual_seed(7)
    args = coma_args(mask_before_softmax=mask_before_softmax)
    B, T, N, d_obs, A, S = 4, 7, 5, 80, 15, 60
    batch, scheme, groups, preprocess = MG.make_batch(B, T, N, d_obs, A, S, [6, 3, 4, 2], seed=8)
    mac = BasicMAC(batch.scheme, groups, args)
    logger = MG.StatLogger()
    learner = ref_coma.COMALearner(mac, batch.scheme, logger, args, name="home")
    out = {"epsilon": np.array(mac.action_selector.epsilon, dtype=np.float64),
           "mask_before_softmax": np.array(int(mask_before_softmax))}
    out.update(MG.sd_to_np("p0.agent.", mac.agent.state_dict()))
    out.update(MG.sd_to_np("p0.critic.", learner.critic.state_dict()))
    out.update(MG.batch_to_np("b.", batch))
    captured = {}
    orig_td, orig_tc = ref_coma.build_td_lambda_targets, learner._train_critic

    def td(*a, **k):
        captured["targets"] = orig_td(*a, **k)
        return captured["targets"]

    def tc(*a, **k):
        q, log = orig_tc(*a, **k)
        captured["q_vals"] = q.detach().clone()
        return q, log

    ref_coma.build_td_lambda_targets = td
    learner._train_critic = tc
    calls = [(100, 0), (200, 4), (300, 8)]
    out["calls"] = np.array(calls, dtype=np.int64)
    for i, (t_env, ep) in enumerate(calls):
        logger.stats.clear()
        learner.train(batch, t_env, ep)
        stats = {k.replace("home_comalearner_", ""): v for k, v, _ in logger.stats}
        for k in STATS:
            out[f"stat{i}.{k}"] = np.array(stats[k], dtype=np.float64)
        out[f"q_vals{i}"] = captured["q_vals"].numpy().copy()
        out[f"targets{i}"] = captured["targets"].detach().numpy().copy()
        out[f"sub{i}.agent"] = flat(mac.agent)[::SUB]
        out[f"sub{i}.critic"] = flat(learner.critic)[::SUB]
        out[f"sub{i}.target_critic"] = flat(learner.target_critic)[::SUB]
        out[f"steps{i}"] = np.array(learner.critic_training_steps, dtype=np.int64)
        out[f"last_update{i}"] = np.array(learner.last_target_update_step, dtype=np.int64)
        if i == 1:
            assert np.array_equal(flat(learner.critic), flat(learner.target_critic)), "the update fires after call 2"
    assert np.array_equal(out["sub1.target_critic"], out["sub2.target_critic"])
    ref_coma.build_td_lambda_targets = orig_td
    out.update(MG.sd_to_np("p3.agent.", mac.agent.state_dict()))
    out.update(MG.sd_to_np("p3.critic.", learner.critic.state_dict()))
    assert all(np.isfinite(v).all() for k, v in out.items() if v.dtype.kind == "f"), "NaN in the reference run"
    np.savez_compressed(os.path.join(OUT, f"coma_learner_{tag}.npz"), **out)


def policy_fixture():
    """_softmax on random logits: A in {11, 15, 55}, rows with one and with no available action."""
    out = {"coma_yaml": np.array(json.dumps(coma_yaml(), sort_keys=True))}
    rng = np.random.RandomState(21)
    for A in (11, 15, 55):
        Bn, N = 6, 5
        logits = (rng.randn(Bn, N, A) * 2).astype(np.float32)
        avail = (rng.rand(Bn, N, A) < 0.6).astype(np.int32)
        avail[..., 0] = np.maximum(avail[..., 0], (avail.sum(-1) == 0))
        avail[0, 0, :] = 0
        avail[0, 0, A // 2] = 1   # one available action
        avail[0, 1, :] = 0        # none
        avail[1, 0, :] = 1        # all
        out[f"A{A}.logits"], out[f"A{A}.avail"] = logits, avail
        for mask in (True, False):
            args = coma_args(mask_before_softmax=mask, n_actions=A)
            scheme, groups, preprocess = MG.scheme_for(8 * (A - 5), A, 6 * (A - 5))
            groups = {"agents": N}
            batch = MG.EpisodeBatch(scheme, groups, Bn, 2, preprocess=preprocess, device="cpu")
            batch.update({"avail_actions": th.tensor(avail)}, ts=0)
            mac = BasicMAC(batch.scheme, groups, args)
            mac.action_selector.epsilon = 0.3
            for test_mode in (False, True):
                p = mac._softmax(th.tensor(logits).reshape(Bn * N, A).clone(), batch, 0, test_mode)
                out[f"A{A}.probs.mask{int(mask)}.test{int(test_mode)}"] = p.reshape(Bn, N, A).numpy().copy()
    out["epsilon"] = np.array(0.3)
    np.savez_compressed(os.path.join(OUT, "coma_policy.npz"), **out)


if __name__ == "__main__":
    policy_fixture()
    learner_fixture("mask", True)
    learner_fixture("nomask", False)
    print("COMA golden fixtures written to", OUT)
