"""Exception types of the reference's hot-path boundary (src/exceptions/*.py)."""


class HiddenStateNotInitialized(Exception):
    def __init__(self):
        super().__init__("Please run init_hidden() to initialize the hidden state before running forward pass.)")


class MultiAgentControllerNotInitialized(Exception):
    def __init__(self):
        super().__init__("Multi-Agent Controller not initialized."
                         "Please run initialize() with it`s corresponding arguments to prepare the runner.")


class NoLearnersProvided(Exception):
    def __init__(self):
        super().__init__("The provided list of learners is empty. Make sure to register learners before calling a save.")


ENTITY_LEAGUE_ERROR = ("{who}: entity_scheme agents (REFIL, attn_qmix, attn_vdn) are not supported here: the league "
                       "instance, cross-play evaluation and opponent mixtures need per-team rosters in the entity env "
                       "spec (out of scope). Two EntityMACs play each other through SelfPlayEntityParallelStepper / "
                       "SelfPlayEntityStepper (steppers.SELF_ENTITY_REGISTRY) under SelfPlayMultiAgentExperiment")


def refuse_entity_league(args, who: str):
    """The league layers refuse entity-scheme configs by name."""
    if getattr(args, "entity_scheme", False):
        raise NotImplementedError(ENTITY_LEAGUE_ERROR.format(who=who))
