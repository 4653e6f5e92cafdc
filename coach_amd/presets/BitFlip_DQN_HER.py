"""BitFlip DQN with Hindsight Experience Replay, 20 bits, for the device engine — the hyper-parameters and the golden
test of rl_coach/presets/BitFlip_DQN_HER.py: the agent of BitFlip_DQN with the episodic hindsight replay (`Final` goal
selection, one hindsight copy per transition, goal = the 'state' observation, reward 0 at distance 0 and -1 otherwise,
Euclidean); an averaged evaluation reward of -15 within 10 000 episodes.  20 bits are not learnable from the sparse
reward alone; relabelling every episode with the goal it did reach is what makes them so.  The copies are written on
the device (coach_amd/memories/episodic/episodic_hindsight_experience_replay.py)."""
from coach_amd.base_parameters import PresetValidationParameters, VisualizationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters
from coach_amd.memories.episodic.episodic_hindsight_experience_replay import (
    EpisodicHindsightExperienceReplayParameters, HindsightGoalSelectionMethod)
from coach_amd.presets.BitFlip_DQN import agent_parameters, environment_parameters
from coach_amd.spaces import GoalsSpace, ReachingGoal

BIT_LENGTH = 20


def make(num_envs=1, seed=1234, agent_seed=0, bit_length=BIT_LENGTH):
    """seed: the environments' reset streams; agent_seed: the agent's host generators and initial weights."""
    sched = ScheduleParameters()
    sched.improve_steps = EnvironmentEpisodes(16 * 50 * 200)                   # 200 epochs
    sched.steps_between_evaluation_periods = EnvironmentEpisodes(16 * 50)      # 50 cycles
    sched.evaluation_steps = EnvironmentEpisodes(10)
    sched.heatup_steps = EnvironmentSteps(0)
    agent = agent_parameters(agent_seed)
    agent.memory = EpisodicHindsightExperienceReplayParameters()
    agent.memory.hindsight_goal_selection_method = HindsightGoalSelectionMethod.Final
    agent.memory.hindsight_transitions_per_regular_transition = 1
    agent.memory.goals_space = GoalsSpace(goal_name='state',
                                          reward_type=ReachingGoal(distance_from_goal_threshold=0, goal_reaching_reward=0,
                                                                   default_reward=-1),
                                          distance_metric=GoalsSpace.DistanceMetric.Euclidean)
    validation = PresetValidationParameters()
    validation.test = True
    validation.min_reward_threshold = -15
    validation.max_episodes_to_achieve_reward = 10000
    return BasicRLGraphManager(agent_params=agent, env_params=environment_parameters(bit_length, num_envs, seed),
                               schedule_params=sched, vis_params=VisualizationParameters(),
                               preset_validation_params=validation)


graph_manager = make()
