"""Behavioral Cloning on the device CartPole from a logged dataset.

This preset is the project's own: the reference's BC presets (Doom_Basic_BC, MontezumaRevenge_BC) need simulators and
pickled replay buffers that are not served.  It keeps their shape — no heat-up, num_consecutive_playing_steps =
EnvironmentSteps(0), improve_steps and steps_between_evaluation_periods in TrainingSteps, an evaluation_epsilon of 0 —
on CartPole-v0 (coach_amd/environments/cartpole_vector_environment.py) and a CSV file of logged transitions
(core_types.CsvDataset) that the agent's EpisodicExperienceReplay starts as.  There is no module-level graph_manager:
the dataset's path is an argument.
"""
from coach_amd.agents.bc_agent import BCAgentParameters
from coach_amd.base_parameters import VisualizationParameters
from coach_amd.core_types import CsvDataset, EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager
from coach_amd.graph_managers.graph_manager import ScheduleParameters
from coach_amd.memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters


def make(dataset, seed=1234, agent_seed=0, improve_steps=2000, steps_between_evaluation_periods=500,
         evaluation_episodes=5, batch_size=32, learning_rate=0.00025):
    """dataset: the path of a CSV file of logged transitions; seed: the environment's reset-state streams;
    agent_seed: the agent's host generators and initial weights"""
    if not dataset:
        raise ValueError("CartPole_BC trains from a logged dataset: make(dataset=path of a CSV file)")
    sched = ScheduleParameters()
    sched.improve_steps = TrainingSteps(improve_steps)
    sched.steps_between_evaluation_periods = TrainingSteps(steps_between_evaluation_periods)
    sched.evaluation_steps = EnvironmentEpisodes(evaluation_episodes)
    sched.heatup_steps = EnvironmentSteps(0)

    agent = BCAgentParameters()
    agent.seed = agent_seed
    agent.algorithm.num_consecutive_playing_steps = EnvironmentSteps(0)
    agent.algorithm.num_consecutive_training_steps = 1
    agent.network_wrappers['main'].batch_size = batch_size
    agent.network_wrappers['main'].learning_rate = learning_rate
    agent.exploration.evaluation_epsilon = 0
    agent.memory = EpisodicExperienceReplayParameters()
    agent.memory.load_memory_from_file_path = CsvDataset(dataset)

    env = CartPoleVectorEnvironmentParameters(1, "CartPole-v0", seed=seed)
    return BasicRLGraphManager(agent_params=agent, env_params=env, schedule_params=sched,
                               vis_params=VisualizationParameters())
