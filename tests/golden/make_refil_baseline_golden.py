"""Generate the golden vectors of the REFIL learner's two attention baselines from the reference.

TEST INFRASTRUCTURE ONLY; runs in the build container with the reference mounted read-only at
/root/reference and records inputs/outputs of the reference's own modules as .npz data.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_refil_baseline_golden.py

Two consecutive REFILLearner.train calls (src/marl/learners/refil_learner.py:67-202, the non-imagine branch
:107-110 / :152-155) on the B = 4, T = 7 batch of make_refil_golden.py's learner_fixture (lengths 6, 4, 6, 3; one
episode not terminated), read back from refil_learner.npz:

refil_attn_qmix.npz   agent entity_attend_rnn, mixer flex_qmix (attention-QMIX)
refil_attn_vdn.npz    agent entity_attend_rnn, mixer vdn       (attention-VDN; mixer.state_dict() is empty)

Each holds the batch (b.*), and per call c the logged stats (c{c}.stat.*; no im_loss: the reference logs it only
for imagine agents) and the agent / mixer parameters after the call (c{c}.agent.*, c{c}.mixer.*). The initial
parameters are those of refil_learner.npz (its p0.agent.* / p0.mixer.*): the imagine fixture and the baselines
start from the same networks. refil_attn_vdn.npz repeats them (p0.agent.*); refil_attn_qmix.npz does not -- three
copies of the 130645 parameters do not fit a committed file, two do -- and its readers take p0.* from
refil_learner.npz.

As in make_refil_golden.py the reference's EntityMAC cannot serve forward(batch, t=None); the fixture uses the
intended semantics (t=None = the whole episode) with the reference's own _build_inputs and agent networks, and the
torch 1.9 masked_fill semantics for uint8 masks.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

REF_SRC = "/root/reference/src"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF_SRC)
sys.dont_write_bytecode = True

import torch as th  # noqa: E402

th.set_num_threads(1)

# The reference targets torch 1.9, where masked_fill accepted uint8 masks (read as bool); torch 2.x refuses them.
_masked_fill = th.Tensor.masked_fill


def _masked_fill_u8(self, mask, value):
    return _masked_fill(self, mask.bool() if mask.dtype == th.uint8 else mask, value)


th.Tensor.masked_fill = _masked_fill_u8

from marl.components.episode_batch import EpisodeBatch  # noqa: E402
from marl.components.transforms import OneHot  # noqa: E402
from marl.controllers.entity_controller import EntityMAC  # noqa: E402
from marl.learners.refil_learner import REFILLearner  # noqa: E402
from marl.modules.agents import REGISTRY as agent_REGISTRY  # noqa: E402
from marl.modules.agents.entity_rnn_agent import EntityAttentionRNNAgent  # noqa: E402

NA, NE, ED, A = 8, 16, 8, 21  # agents, entities, entity features, actions


def baseline_args(**kw):
    a = dict(n_agents=NA, n_entities=NE, n_actions=A, entity_shape=ED, entity_last_action=True,
             attn_embed_dim=64, attn_n_heads=4, rnn_hidden_dim=64, hypernet_embed=64, mixing_embed_dim=32,
             pooling_type=None, softmax_mixing_weights=False, mixer="flex_qmix", entity_scheme=True,
             agent="entity_attend_rnn", agent_output_type="q", action_selector="epsilon_greedy",
             epsilon_start=1.0, epsilon_finish=0.05, epsilon_anneal_time=50000, double_q=True, gamma=0.99,
             lr=5e-4, optim_alpha=0.99, optim_eps=1e-5, weight_decay=0, grad_norm_clip=10,
             target_update_interval=200, learner_log_interval=0, lmbda=0.5, train_gt_factors=False,
             train_rand_gt_factors=False, test_gt_factors=False, gt_mask_avail=False, device="cpu",
             obs_last_action=False, obs_agent_id=False, freeze_native=False)
    a.update(kw)
    return SimpleNamespace(**a)


def sd(prefix, module):
    return {f"{prefix}{k}": v.detach().numpy().copy() for k, v in module.state_dict().items()}


class _Log:
    def __init__(self):
        self.stats = {}
        self.console_logger = SimpleNamespace(info=lambda *a, **k: None)

    def log_stat(self, k, v, t):
        self.stats[k] = float(v)


class _IntendedEntityMAC(EntityMAC):
    """EntityMAC with the intended forward(batch, t=None): t=None -> the whole episode; inputs from the
    reference's own EntityMAC._build_inputs."""

    def train(self):  # the learner forwards train() / eval() to the agent (refil_learner.py:82-85)
        self.agent.train()

    def eval(self):
        self.agent.eval()

    def forward(self, ep_batch, t=None, test_mode=False, **kw):
        if t is None:
            t = slice(0, ep_batch["avail_actions"].shape[1])
        inputs = self._build_inputs(ep_batch, t)
        q, self.hidden_states = self.agent(inputs, self.hidden_states)
        return q


def fixture_batch(src):
    """The learner_fixture batch, from the arrays refil_learner.npz recorded of it."""
    arrs = {k[2:]: src[k] for k in src.files if k.startswith("b.")}
    B, T = arrs["entities"].shape[:2]
    scheme = {"entities": {"vshape": ED, "group": "entities"},
              "obs_mask": {"vshape": (NE,), "group": "entities", "dtype": th.uint8},
              "entity_mask": {"vshape": (NE,), "dtype": th.uint8},
              "actions": {"vshape": (1,), "group": "agents", "dtype": th.long},
              "avail_actions": {"vshape": (A,), "group": "agents", "dtype": th.int},
              "reward": {"vshape": (1,)}, "terminated": {"vshape": (1,), "dtype": th.uint8}}
    groups = {"agents": NA, "entities": NE}
    batch = EpisodeBatch(scheme, groups, B, T, preprocess={"actions": ("actions_onehot", [OneHot(out_dim=A)])})
    for k, v in arrs.items():
        batch.data.transition_data[k].copy_(th.from_numpy(v))
    return batch, groups, arrs


def record(mixer, name, with_p0):
    src = np.load(os.path.join(OUT, "refil_learner.npz"), allow_pickle=False)
    batch, groups, arrs = fixture_batch(src)
    agent_REGISTRY["entity_attend_rnn"] = EntityAttentionRNNAgent
    args = baseline_args(mixer=mixer)
    mac = _IntendedEntityMAC(batch.scheme, groups, args)
    learner = REFILLearner(mac, batch.scheme, _Log(), args)
    p0a = {k[len("p0.agent."):]: th.from_numpy(src[k]) for k in src.files if k.startswith("p0.agent.")}
    mac.agent.load_state_dict(p0a)
    learner.target_mac.agent.load_state_dict(p0a)
    if mixer == "flex_qmix":
        p0m = {k[len("p0.mixer."):]: th.from_numpy(src[k]) for k in src.files if k.startswith("p0.mixer.")}
        learner.mixer.load_state_dict(p0m)
        learner.target_mixer.load_state_dict(p0m)
    out = {f"b.{k}": v for k, v in arrs.items()}
    if with_p0:
        out.update(sd("p0.agent.", mac.agent))
        out.update(sd("p0.mixer.", learner.mixer))
    for call in range(2):
        th.manual_seed(100 + call)
        learner.logger = _Log()
        learner.train(batch, t_env=1000 * (call + 1), episode_num=call)
        for k, v in learner.logger.stats.items():
            out[f"c{call}.stat.{k}"] = np.array(v)
        out.update(sd(f"c{call}.agent.", mac.agent))
        out.update(sd(f"c{call}.mixer.", learner.mixer))
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path), "bytes; stats", sorted(learner.logger.stats))


def main():
    record("flex_qmix", "refil_attn_qmix.npz", with_p0=False)
    record("vdn", "refil_attn_vdn.npz", with_p0=True)


if __name__ == "__main__":
    main()
