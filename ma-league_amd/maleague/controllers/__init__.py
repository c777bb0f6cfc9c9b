"""MAC registry (reference: src/marl/controllers/__init__.py:6-11; "entity" = EntityMAC, unregistered in the
reference; "ensemble" and "gpe" are research stubs there and stay out)."""
from .basic_controller import BasicMAC, MultiAgentController
from .distinct_controller import DistinctMAC
from .entity_controller import EntityMAC

REGISTRY = {"basic": BasicMAC, "distinct": DistinctMAC, "entity": EntityMAC}

__all__ = ["BasicMAC", "DistinctMAC", "EntityMAC", "MultiAgentController", "REGISTRY"]
