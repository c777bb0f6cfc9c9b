"""Stepper registries (reference: src/steppers/__init__.py:6-12). With ``entity_scheme`` (REFIL, config 5) the
same keys resolve to the entity-env steppers (see build_stepper)."""
from .entity_stepper import EntityEpisodeStepper, EntityParallelStepper
from .parallel_stepper import EnvStepper, EpisodeStepper, ParallelStepper
from .self_play_stepper import (OpponentMix, SelfPlayDistinctParallelStepper, SelfPlayDistinctStepper,
                                SelfPlayEntityParallelStepper, SelfPlayEntityStepper, SelfPlayFFParallelStepper, SelfPlayFFStepper, SelfPlayParallelStepper,
                                SelfPlayPolicyParallelStepper, SelfPlayPolicyStepper, SelfPlayStepper)

REGISTRY = {"episode": EpisodeStepper, "parallel": ParallelStepper}
SELF_REGISTRY = {"episode": SelfPlayStepper, "parallel": SelfPlayParallelStepper}
# two pi_logits MACs (COMA in self-play and the league): the policy softmax and the multinomial draw on both sides
SELF_POLICY_REGISTRY = {"episode": SelfPlayPolicyStepper, "parallel": SelfPlayPolicyParallelStepper}
# two DistinctMACs (mac: distinct in self-play and the league): one network per agent slot on both sides
SELF_DISTINCT_REGISTRY = {"episode": SelfPlayDistinctStepper, "parallel": SelfPlayDistinctParallelStepper}
# two feed-forward MACs (agent: dqn in self-play and the league): no hidden state on either side
SELF_FF_REGISTRY = {"episode": SelfPlayFFStepper, "parallel": SelfPlayFFParallelStepper}
ENTITY_REGISTRY = {"episode": EntityEpisodeStepper, "parallel": EntityParallelStepper}
# two EntityMACs (REFIL, attn_qmix, attn_vdn in self-play): the two-policy entity env, away side in the canonical view
SELF_ENTITY_REGISTRY = {"episode": SelfPlayEntityStepper, "parallel": SelfPlayEntityParallelStepper}


def build_stepper(args, logger, log_start_t=0):
    reg = ENTITY_REGISTRY if getattr(args, "entity_scheme", False) else REGISTRY
    return reg[args.runner](args=args, logger=logger, log_start_t=log_start_t)


__all__ = ["EnvStepper", "OpponentMix", "EpisodeStepper", "ParallelStepper", "SelfPlayParallelStepper", "SelfPlayStepper",
           "SelfPlayPolicyParallelStepper", "SelfPlayPolicyStepper", "SelfPlayDistinctParallelStepper",
           "SelfPlayDistinctStepper", "SelfPlayFFParallelStepper", "SelfPlayFFStepper", "EntityParallelStepper",
           "EntityEpisodeStepper", "SelfPlayEntityParallelStepper", "SelfPlayEntityStepper", "REGISTRY", "SELF_REGISTRY", "SELF_POLICY_REGISTRY", "SELF_DISTINCT_REGISTRY",
           "SELF_FF_REGISTRY", "ENTITY_REGISTRY", "SELF_ENTITY_REGISTRY", "build_stepper"]
