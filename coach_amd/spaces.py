"""The space descriptions a network is constructed from — the fields of rl_coach/spaces.py that the
device networks read (observation shape, number of discrete actions / action dimension and bounds)."""
from enum import Enum

import numpy as np


class Space(object):
    def __init__(self, shape, low=-np.inf, high=np.inf):
        self.shape = np.array([shape]) if np.isscalar(shape) else np.array(shape)
        self.low, self.high = low, high

    @property
    def num_dimensions(self):
        return len(self.shape)


class ObservationSpace(Space):
    """VectorObservationSpace: shape (D,); image observations: (H, W, stack) uint8."""


class DiscreteActionSpace(Space):
    def __init__(self, num_actions, descriptions=None):
        super().__init__(1, 0, num_actions - 1)
        self.actions = list(range(num_actions))
        self.descriptions = descriptions


class BoxActionSpace(Space):
    def __init__(self, shape, low=-1.0, high=1.0):
        super().__init__(shape, low, high)


class StateSpace(object):
    def __init__(self, sub_spaces):
        self.sub_spaces = dict(sub_spaces)

    def __getitem__(self, item):
        return self.sub_spaces[item]


class SpacesDefinition(object):
    def __init__(self, state, goal, action, reward=None):
        self.state, self.goal, self.action, self.reward = state, goal, action, reward


# ---- goals (spaces.py:508-638): parameter holders with the reference's constructor signatures.  The arithmetic they
# stand for — the distance between a goal and the `goal_name` part of a state, turned into (reward, game_over) — runs on
# the device (csrc/her.hip) for ReachingGoal under the Euclidean and Manhattan metrics.
class GoalToRewardConversion(object):
    def __init__(self, goal_reaching_reward=0):
        self.goal_reaching_reward = goal_reaching_reward


class ReachingGoal(GoalToRewardConversion):
    """goal_reaching_reward once the distance is at or below the threshold (and the episode is over), else
    default_reward (spaces.py:522-542)."""
    def __init__(self, distance_from_goal_threshold, goal_reaching_reward=0, default_reward=-1):
        super().__init__(goal_reaching_reward)
        self.distance_from_goal_threshold = distance_from_goal_threshold
        self.default_reward = default_reward


class InverseDistanceFromGoal(GoalToRewardConversion):
    """min(max_reward, 1 / distance) (spaces.py:545-560): held for presets that name it; no device implementation."""
    def __init__(self, distance_from_goal_threshold, max_reward=1):
        super().__init__(goal_reaching_reward=max_reward)
        self.distance_from_goal_threshold = distance_from_goal_threshold
        self.max_reward = max_reward


class GoalsSpace(object):
    """spaces.py:563-638: which observation is the achieved goal (`goal_name`), how a distance becomes a reward
    (`reward_type`) and which distance (`distance_metric`: a DistanceMetric member or a callable).  A parameter holder:
    the shape and bounds the reference copies from its target space are the environment's slice table's here."""
    class DistanceMetric(Enum):
        Euclidean = 0
        Cosine = 1
        Manhattan = 2

    def __init__(self, goal_name, reward_type, distance_metric):
        self.goal_name = goal_name
        self.distance_metric = distance_metric
        self.reward_type = reward_type
        self.target_space = None
        self.max_abs_range = None
