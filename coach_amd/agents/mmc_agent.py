"""Mixed Monte Carlo (MMC) on one MI355X — host-side mirror of rl_coach/agents/mmc_agent.py (parameter classes :26-45,
MixedMonteCarloAgent.learn_from_batch :57-83).

A DQN-family agent whose TD target is (1 - monte_carlo_mixing_rate) times the Double-DQN target plus
monte_carlo_mixing_rate times the transition's Monte Carlo return (the episodic replay's n_step_discounted_rewards
column, n_step = -1: the discounted return to the episode's end).
Per step: DQN's acting (online Q values, epsilon-greedy).
Per update: online(s') (the selector), target(s'), online(s) -> rlx_mixed_target_head_loss without the target's values
on s (targets, loss, dQ: csrc/pal.hip) -> backward -> TF1 Adam.
"""
from ..memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters
from .dqn_agent import DQNAgentParameters, DQNAlgorithmParameters
from .pal_agent import MixedTargetDQNAgent


class MixedMonteCarloAlgorithmParameters(DQNAlgorithmParameters):       # mmc_agent.py:26-34
    def __init__(self):
        super().__init__()
        self.monte_carlo_mixing_rate = 0.1


class MixedMonteCarloAgentParameters(DQNAgentParameters):               # mmc_agent.py:37-45
    def __init__(self):
        super().__init__()
        self.algorithm = MixedMonteCarloAlgorithmParameters()
        self.memory = EpisodicExperienceReplayParameters()

    @property
    def path(self):
        return 'coach_amd.agents.mmc_agent:MixedMonteCarloAgent'


class MixedMonteCarloAgent(MixedTargetDQNAgent):
    MODE = "mmc"

    def _target_parameters(self):
        return 0.0, False, self.ap.algorithm.monte_carlo_mixing_rate
