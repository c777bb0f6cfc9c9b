"""Golden vectors of the reference QLearner for the mixer shapes beyond the default one (run where the reference
checkout that make_golden.py names is present):

  qlearner_qmix_h1.npz         hypernet_layers 1 (the reference QMixer's fallback, qmix.py:17), mixing_embed_dim 32
  qlearner_qmix_e64_he128.npz  hypernet_layers 2, mixing_embed_dim 64, hypernet_embed 128

Both reuse make_golden.qlearner_fixture unchanged (same batch, agent seed and three calls as qlearner_qmix_dq.npz),
in its non-"full" form: initial parameters, the statistics of every call, the parameters after the last call.

  qlearner_qmix_9v9_h128.npz        off the default agent shape: N = 9, A = 23, S = 108, d_obs = 144 (the 9v9 plan's
  qlearner_qmix_9v9_h128_after.npz  dims), rnn_hidden_dim 128, default mixer widths; B = 4, T = 7, three calls

qlearner_fixture fixes the agent dims, so these come from its sibling below, dims_fixture: the same recipe (seeds,
episode lengths, calls, non-"full" form) at other dims. The H = 128 agent alone is 0.5 MB, so the fixture is two
files under the 1 MiB limit for a committed file: the first holds the initial parameters, the batch, the calls and
every call's statistics, the `_after` file the online agent and mixer after the last call and `target_is_online`:
whether the reference's target agent then equalled its online agent bit for bit (the third call ends with the target
update), in place of a third copy of the agent.

There is no IQL golden: with `mixer: None` the reference's QLearner.parameters() returns [] (the precedence slip at
q_learner.py:30-32) and torch.optim.RMSprop refuses an empty parameter list, so the reference cannot train IQL at
all. IQL is checked against oracle/learner_ref.py only (tests/test_gpu_learner_shapes.py).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as G  # noqa: E402


def dims_fixture(tag, N, A, S, d_obs, **kw):
    """make_golden.qlearner_fixture's recipe at other agent dims, written as qlearner_<tag>.npz and
    qlearner_<tag>_after.npz (see the module docstring)."""
    th = G.th
    th.manual_seed(7)
    args = G.base_args(n_agents=N, n_actions=A, state_shape=S, **kw)
    B, T = 4, 7
    batch, scheme, groups, preprocess = G.make_batch(B, T, N, d_obs, A, S, [6, 3, 4, 2], seed=8)
    mac = G.BasicMAC(batch.scheme, groups, args)
    logger = G.StatLogger()
    learner = G.QLearner(mac, batch.scheme, logger, args, name="home")
    learner.build_optimizer()
    out = {}
    out.update(G.sd_to_np("p0.agent.", mac.agent.state_dict()))
    out.update(G.sd_to_np("p0.mixer.", learner.mixer.state_dict()))
    out.update(G.batch_to_np("b.", batch))
    calls = [(100, 0), (200, 32), (300, 232)]  # (t_env, episode_num): 3rd call crosses target_update_interval
    out["calls"] = np.array(calls, dtype=np.int64)
    for i, (t_env, ep) in enumerate(calls):
        logger.stats.clear()
        learner.train(batch, t_env, ep)
        stats = {k.replace("home_qlearner_", ""): v for k, v, _ in logger.stats}
        for k in ["loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean"]:
            out[f"stat{i}.{k}"] = np.array(stats[k], dtype=np.float64)
    out["trained_steps"] = np.array(mac.agent.trained_steps, dtype=np.int64)
    last = len(calls)
    after = {}
    after.update(G.sd_to_np(f"p{last}.agent.", mac.agent.state_dict()))
    after.update(G.sd_to_np(f"p{last}.mixer.", learner.mixer.state_dict()))
    tsd = learner.target_mac.agent.state_dict()
    after["target_is_online"] = np.array(all(th.equal(v, tsd[k]) for k, v in mac.agent.state_dict().items()))
    for name, data in ((f"qlearner_{tag}.npz", out), (f"qlearner_{tag}_after.npz", after)):
        path = os.path.join(G.OUT, name)
        np.savez_compressed(path, **data)
        assert os.path.getsize(path) <= 1 << 20, (name, os.path.getsize(path))


if __name__ == "__main__":
    G.qlearner_fixture("qmix_h1", False, hypernet_layers=1)
    G.qlearner_fixture("qmix_e64_he128", False, mixing_embed_dim=64, hypernet_embed=128)
    dims_fixture("qmix_9v9_h128", N=9, A=23, S=108, d_obs=144, rnn_hidden_dim=128)
    print("golden fixtures written to", G.OUT)
