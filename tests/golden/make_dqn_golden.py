"""Generate the feed-forward agent's golden vectors from the reference (agent: dqn).

TEST INFRASTRUCTURE ONLY, run where make_golden.py runs: it imports the reference's own Python modules through
make_golden.py and records their inputs / outputs as small fixtures (data only, no reference source text).

The reference's DQNAgentNetwork.init_hidden returns zeros(batch_size, 1, 1), which BasicMAC.init_hidden cannot expand
(DESIGN.md §7), so ``agent: dqn`` never ran under BasicMAC there. This script patches init_hidden in the running
process only, with the shape this project uses (a zero [1, 1] tensor), and changes nothing else.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dqn_golden.py

Fixtures:
  dqn_forward.npz       DQNAgentNetwork.forward  src/marl/modules/agents/dqn_agent.py:34-37
                        p.* state_dict, inputs [40, 100], q [40, 15]
  dqn_mac_forward.npz   BasicMAC._build_inputs + forward over t = 0..3 with agent="dqn"
                        src/marl/controllers/basic_controller.py:38-50,80-92: p.* state_dict, b.* batch, q [T, B, N, A]
  ckpt_dqn/100/home_agent.th  written by the reference's BasicMAC.save_models (tests load it with weights_only=True)
  qlearner_dqn_qmix.npz, qlearner_dqn_vdn.npz   make_golden.qlearner_fixture's recipe (B = 4, T = 7, three
                        QLearner.train calls: initial parameters, per-call statistics, final parameters) with agent="dqn"
                        src/marl/learners/q_learner.py:34-131
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402  (puts the reference on sys.path)

import torch as th  # noqa: E402
from marl.controllers.basic_controller import BasicMAC  # noqa: E402
from marl.modules.agents.dqn_agent import DQNAgentNetwork  # noqa: E402

OUT = MG.OUT

# the fix, in this process only
DQNAgentNetwork.init_hidden = lambda self: th.zeros(1, 1, device=self.args.device)


def forward_fixture():
    th.manual_seed(0)
    args = MG.base_args(agent="dqn")
    agent = DQNAgentNetwork(100, args)
    g = th.Generator().manual_seed(1)
    inputs = th.randn(40, 100, generator=g)
    with th.no_grad():
        q, h = agent(inputs, th.zeros(40, 1))
    assert h.shape == (40, 1) and not h.any()
    out = MG.sd_to_np("p.", agent.state_dict())
    out.update(inputs=inputs.numpy(), q=q.numpy())
    np.savez_compressed(os.path.join(OUT, "dqn_forward.npz"), **out)


def mac_fixture():
    th.manual_seed(2)
    args = MG.base_args(agent="dqn")
    B, T, N, d_obs, A, S = 3, 4, 5, 80, 15, 60
    batch, scheme, groups, preprocess = MG.make_batch(B, T, N, d_obs, A, S, [3, 2, 3], seed=3)
    mac = BasicMAC(batch.scheme, groups, args)
    mac.init_hidden(B)
    assert tuple(mac.hidden_states.shape) == (B, N, 1)
    qs = []
    with th.no_grad():
        for t in range(T):
            qs.append(mac.forward(batch, t).numpy().copy())
    out = MG.sd_to_np("p.", mac.agent.state_dict())
    out.update(MG.batch_to_np("b.", batch))
    out["q"] = np.stack(qs)
    np.savez_compressed(os.path.join(OUT, "dqn_mac_forward.npz"), **out)
    ck = os.path.join(OUT, "ckpt_dqn", "100")
    os.makedirs(ck, exist_ok=True)
    mac.save_models(ck, "home_")


if __name__ == "__main__":
    forward_fixture()
    mac_fixture()
    MG.qlearner_fixture("dqn_qmix", False, agent="dqn")
    MG.qlearner_fixture("dqn_vdn", False, agent="dqn", mixer="vdn")
