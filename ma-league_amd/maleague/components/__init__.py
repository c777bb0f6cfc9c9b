from .episode_batch import EpisodeBatch
from .replay_buffer import PrioritizedReplayBuffer, ReplayBuffer
from .transforms import OneHot, Transform
from .epsilon_schedules import DecayThenFlatSchedule

__all__ = ["EpisodeBatch", "ReplayBuffer", "PrioritizedReplayBuffer", "OneHot", "Transform", "DecayThenFlatSchedule"]
