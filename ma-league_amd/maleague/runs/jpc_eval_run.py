"""Joint-policy-correlation evaluation run (API of src/runs/evaluation/jpc_eval_run.py:12-89).

``instances_num`` independent self-play instances are trained, then the home policy of every instance plays the away
policy of every instance; ``jpc_matrix[i, j]`` is the sum of the two sides' mean episode returns, and the average
proportional loss (eval/methods.py:8-18) says how much a policy loses when it meets a partner it was not trained with.

The reference trains and evaluates in a process ``Pool`` and runs one ``evaluate_mean_returns`` per pair. Here the
instances train one after another on this GPU, their policies stay on the device as rows of one pool tensor, and ONE
``CrossPlayEvaluator.evaluate`` call (``PolicyCrossPlayEvaluator`` for ``pi_logits`` policies) plays all instances_num^2
pairs in one launch (league.evaluation).
"""
from __future__ import annotations

import copy
from typing import List

import torch

from ..envs.plans import mirror_plan
from ..league.evaluation import CrossPlayResult, avg_proportional_loss, build_pairs, evaluator_for
from .sp_ma_experiment import SelfPlayMultiAgentExperiment, agent_vector


class JointPolicyCorrelationEvaluationRun:
    def __init__(self, args, logger, instances_num: int = 2, eval_episodes=100):
        self.args = args
        self.args.t_max = 200
        self.logger = logger
        self.instances_num = instances_num
        self.eval_episodes = eval_episodes
        self.policies: List[tuple] = [tuple()] * self.instances_num  # (home, away) parameter vectors per instance
        self.jpc_matrix: torch.Tensor = torch.zeros([self.instances_num, self.instances_num], dtype=torch.float32)
        self.result: CrossPlayResult = None  # the full tables of the evaluation (win rates, episode lengths, ...)

    def start(self) -> None:
        """Train the instances, evaluate every (home of i, away of j) pair, fill the JPC matrix."""
        pool = self.train_instances()
        self.result = self.evaluate_instances(pool)
        self.jpc_matrix = self.result.jpc_matrix.to(torch.float32).clone()
        self.logger.info("Finished JPC Evaluation")
        self.logger.info("Avg. Proportional Loss: {}".format(avg_proportional_loss(self.jpc_matrix)))

    def _instance_args(self, instance: int):
        args = copy.deepcopy(self.args)
        args.seed = int(getattr(self.args, "seed", 0) or 0) + instance  # independent instances
        args.env_args = dict(self.args.env_args)
        # self-play: both plan teams policy-controlled (the config's policy team, mirrored)
        args.env_args["match_build_plan"] = mirror_plan(self.args.env_args["match_build_plan"], ai=False,
                                                        config_dir=getattr(self.args, "config_dir", None))
        return args

    def train_instances(self) -> torch.Tensor:
        """Trains every instance in turn; returns the pool [2 * instances_num, n_params]: rows 0..n-1 the home
        policies, rows n..2n-1 the away policies."""
        self.logger.info("Train {} instances.".format(self.instances_num))
        for instance in range(self.instances_num):
            self.policies[instance] = self.train_instance_pair(instance)
        return torch.stack([p[0] for p in self.policies] + [p[1] for p in self.policies])

    def train_instance_pair(self, instance: int):
        """One self-play training run (t_max env steps); returns copies of its (home, away) parameter vectors."""
        play = SelfPlayMultiAgentExperiment(args=self._instance_args(instance), logger=self.logger)
        play.start()
        return agent_vector(play.home_mac).clone(), agent_vector(play.away_mac).clone()

    def evaluate_instances(self, pool: torch.Tensor) -> CrossPlayResult:
        """Every instance's home policy against every instance's away policy, eval_episodes greedy games each."""
        n = self.instances_num
        self.logger.info("Evaluate {} pairings for {} episodes.".format(n * n, self.eval_episodes))
        pairs = build_pairs(range(n), range(n, 2 * n))
        # CrossPlayEvaluator, PolicyCrossPlayEvaluator for pi_logits policies (COMA), or DistinctCrossPlayEvaluator for
        # mac: distinct (a pool row is then a policy's N networks back to back)
        return evaluator_for(self._instance_args(0), pool.device).evaluate(pool, pairs, self.eval_episodes)
