"""Generate the distinct-controller golden vectors from the reference (mac: distinct).

TEST INFRASTRUCTURE ONLY, run where make_golden.py runs: it imports the reference's own Python modules through
make_golden.py and records their inputs / outputs as one small fixture (data only, no reference source text).

The reference's DistinctMAC cannot be constructed as it stands: MultiAgentController.__init__ sets
``self.agent.trained_steps = 0`` on what DistinctMAC._build_agent returns, a plain list. This script
patches _build_agent in the running process only, to return the same networks in a list subclass that takes
attributes, and changes nothing else. forward is recorded at batch_size 1, the one batch size at which the reference's
agent-major concatenation equals its [B, N, A] view.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_distinct_golden.py

Fixture distinct.npz (N = 3, H = 32, d_obs = 48, A = 11, T = 4, B = 1, obs_last_action on, obs_agent_id off):
  p<i>.*      state_dict of network i           src/marl/controllers/distinct_agents_controller.py:79-80
  b.*         the batch
  q           DistinctMAC.forward over t = 0..3, [T, B, N, A]      :32-38 with basic_controller.py:38-50
  h           the hidden states after the last step, [N, B, H]
  ckpt_names  the file names DistinctMAC.save_models wrote                                   :67-71
  ckpt_keys   the keys of each file's state dict, in order; the tensors read back from file i are checked here to equal
              p<i>.* bit for bit and are not stored twice
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402  (puts the reference on sys.path)

import torch as th  # noqa: E402
from marl.controllers.distinct_agents_controller import DistinctMAC  # noqa: E402

OUT = MG.OUT


class _Agents(list):
    """A list that takes attributes (MultiAgentController.__init__ sets trained_steps on it)."""


_build = DistinctMAC._build_agent
DistinctMAC._build_agent = lambda self, input_shape: _Agents(_build(self, input_shape))  # the fix, this process only


def fixture():
    th.manual_seed(4)
    B, T, N, d_obs, A, S = 1, 4, 3, 48, 11, 36
    args = MG.base_args(n_agents=N, n_actions=A, state_shape=S, rnn_hidden_dim=32, obs_agent_id=False)
    batch, scheme, groups, preprocess = MG.make_batch(B, T, N, d_obs, A, S, [3], seed=6)
    mac = DistinctMAC(batch.scheme, groups, args)
    with th.no_grad():  # default initialisations are near-uniform in Q: spread the networks apart
        for i, agent in enumerate(mac.agents):
            agent.fc2.weight.mul_(1.0 + i)
    mac.init_hidden(B)
    qs = []
    with th.no_grad():
        for t in range(T):
            q = mac.forward(batch, t)
            assert tuple(q.shape) == (B, N, A)
            qs.append(q.numpy().copy())
    out = {}
    for i, agent in enumerate(mac.agents):
        out.update(MG.sd_to_np(f"p{i}.", agent.state_dict()))
    out.update(MG.batch_to_np("b.", batch))
    out["q"] = np.stack(qs)
    out["h"] = np.stack([h.detach().reshape(B, -1).numpy().copy() for h in mac.hidden_states])
    with tempfile.TemporaryDirectory() as d:
        mac.save_models(d, "home_")
        names = sorted(os.listdir(d))
        for i in range(N):
            sd = th.load(os.path.join(d, f"home_agent_{i}.th"), map_location="cpu")
            keys = list(sd)
            assert keys == list(mac.agents[i].state_dict())
            assert all(np.array_equal(v.numpy(), out[f"p{i}.{k}"]) for k, v in sd.items())
    out["ckpt_names"] = np.array(names)
    out["ckpt_keys"] = np.array(keys)
    np.savez_compressed(os.path.join(OUT, "distinct.npz"), **out)


if __name__ == "__main__":
    fixture()
