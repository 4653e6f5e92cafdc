"""MuJoCo Wolpertinger for the device engine.

The experiment of rl_coach/presets/Mujoco_Wolpertinger.py, field by field (tests/golden/wolpertinger_preset.json): the
agent's defaults (DDPG's networks and cadence, absolute Gaussian noise of 0.1 on the proto-action, episodic replay, one
neighbour, an embedding of width one) with Dense(400) embedders and Dense(300) middlewares in both networks, an empty
action embedder in the critic, the box discretised into 10^6 actions, 3000 heat-up steps and an evaluation episode every
20 episodes; any level of the MuJoCo v2 family (selected with `make(level=...)` or `env_params.level.select(...)`).
MuJoCo itself is not part of this engine: the level's spaces are served by the synthetic vector environment
(coach_amd/environments/gym_environment.py), the way Mujoco_NAF runs here.
"""
from collections import OrderedDict

from coach_amd.agents.wolpertinger_agent import WolpertingerAgentParameters
from coach_amd.architectures.layers import Dense
from coach_amd.base_parameters import EmbedderScheme, PresetValidationParameters, VisualizationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps
from coach_amd.environments.environment import SingleLevelSelection
from coach_amd.environments.gym_environment import GymVectorEnvironment, mujoco_v2
from coach_amd.filters.action import BoxDiscretization
from coach_amd.filters.filter import OutputFilter
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters


def make(level=None, num_envs=None, agent_seed=0, num_bins=int(1e6), k=None):
    schedule = ScheduleParameters()
    schedule.improve_steps = EnvironmentSteps(2000000)
    schedule.steps_between_evaluation_periods = EnvironmentEpisodes(20)
    schedule.evaluation_steps = EnvironmentEpisodes(1)
    schedule.heatup_steps = EnvironmentSteps(3000)

    agent = WolpertingerAgentParameters()
    agent.seed = agent_seed
    agent.network_wrappers['actor'].input_embedders_parameters['observation'].scheme = [Dense(400)]
    agent.network_wrappers['actor'].middleware_parameters.scheme = [Dense(300)]
    agent.network_wrappers['critic'].input_embedders_parameters['observation'].scheme = [Dense(400)]
    agent.network_wrappers['critic'].middleware_parameters.scheme = [Dense(300)]
    agent.network_wrappers['critic'].input_embedders_parameters['action'].scheme = EmbedderScheme.Empty
    agent.output_filter = OutputFilter(
        action_filters=OrderedDict([('discretization', BoxDiscretization(num_bins_per_dimension=num_bins))]),
        is_a_reference_filter=False)
    if k is not None:
        agent.algorithm.k = k

    env = GymVectorEnvironment(level=SingleLevelSelection(mujoco_v2))
    if level is not None:
        env.level.select(level)
    if num_envs is not None:
        env.num_envs = num_envs
    validation = PresetValidationParameters()
    validation.test = True
    validation.min_reward_threshold = 500
    validation.max_episodes_to_achieve_reward = 1000
    validation.reward_test_level = 'inverted_pendulum'
    validation.trace_test_levels = ['inverted_pendulum']
    return BasicRLGraphManager(agent_params=agent, env_params=env, schedule_params=schedule,
                               vis_params=VisualizationParameters(), preset_validation_params=validation)


graph_manager = make()
