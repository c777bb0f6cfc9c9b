"""Critic registry (reference: src/marl/modules/critics/__init__.py)."""
from .coma import COMACritic

REGISTRY = {"coma": COMACritic}

__all__ = ["COMACritic", "REGISTRY"]
