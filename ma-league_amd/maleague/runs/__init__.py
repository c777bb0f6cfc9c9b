from .ma_experiment import MultiAgentExperiment
from .sp_ma_experiment import LeagueExperiment, SelfPlayMultiAgentExperiment
from .jpc_eval_run import JointPolicyCorrelationEvaluationRun

REGISTRY = {"normal": MultiAgentExperiment, "self": SelfPlayMultiAgentExperiment, "league": LeagueExperiment}

# evaluation runs by the reference's config key (``eval: jpc``, src/main.py:93-101)
EVAL_REGISTRY = {"jpc": JointPolicyCorrelationEvaluationRun}

__all__ = ["MultiAgentExperiment", "SelfPlayMultiAgentExperiment", "LeagueExperiment", "REGISTRY",
           "JointPolicyCorrelationEvaluationRun", "EVAL_REGISTRY"]
