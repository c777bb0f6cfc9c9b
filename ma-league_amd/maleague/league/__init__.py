from .distributed import DistributedLeague
from .evaluation import (CrossPlayEvaluator, CrossPlayResult, DistinctCrossPlayEvaluator, PolicyCrossPlayEvaluator,
                         aggregate, avg_proportional_loss, build_pairs, evaluator_for)
from .instance import DistinctLeagueInstance, LeagueInstance, league_instance_for, league_roles_for
from .matchmaking import REGISTRY as MATCHMAKING_REGISTRY
from .payoff import (REGISTRY, FSPSampling, PayoffEntry, PayoffWrapper, PFSPSampling, SPSampling,
                     episode_result)
from .roles import (ROLES, LeagueExploiter, LeagueView, MainExploiter, MainPlayer, SimplePlayer, alphastar_roles,
                    remove_monotonic_suffix)

__all__ = ["DistributedLeague", "LeagueInstance", "DistinctLeagueInstance", "league_instance_for", "league_roles_for", "MATCHMAKING_REGISTRY", "PayoffEntry",
           "PayoffWrapper", "PFSPSampling", "FSPSampling", "SPSampling", "REGISTRY", "episode_result", "ROLES",
           "LeagueView", "MainPlayer", "MainExploiter", "LeagueExploiter", "SimplePlayer", "alphastar_roles",
           "remove_monotonic_suffix", "CrossPlayEvaluator", "PolicyCrossPlayEvaluator",
           "DistinctCrossPlayEvaluator", "evaluator_for",
           "CrossPlayResult", "aggregate", "avg_proportional_loss", "build_pairs"]
