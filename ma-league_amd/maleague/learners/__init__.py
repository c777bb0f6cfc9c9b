"""Learner registry (reference: src/marl/learners/__init__.py:5-9; SFS is out of scope; "refil" =
REFILLearner, unregistered in the reference; "q_learner" is the key the reference's own algs/iql.yaml
names, which its registry lacks: an alias of "q")."""
from .coma_learner import COMALearner
from .q_learner import Learner, QLearner
from .refil_learner import REFILLearner

REGISTRY = {"q": QLearner, "q_learner": QLearner, "refil": REFILLearner, "coma": COMALearner}

__all__ = ["COMALearner", "Learner", "QLearner", "REFILLearner", "REGISTRY"]
