"""BitFlip DQN, 8 bits, for the device engine — the hyper-parameters and the golden test of
rl_coach/presets/BitFlip_DQN.py: one [Dense(256)] middleware over the two Empty embedders 'desired_goal' and 'state'
(the environment's [desired_goal | state] vector), discount 0.98, 40 updates of batch 128 after every 16 finished
episodes, a soft target update (rate 0.05) every 40 updates, constant epsilon 0.2 (0 when evaluating), a 1 M-transition
uniform replay; an averaged evaluation reward of -7.9 within 10 000 episodes.  8 bits are learnable without hindsight;
BitFlip_DQN_HER is the 20-bit problem that is not.  The level is BitFlip on the device
(coach_amd/environments/bit_flip_vector_environment.py).  `make(num_envs=...)` runs more envs per GPU."""
from coach_amd.agents.dqn_agent import DQNAgentParameters
from coach_amd.architectures.embedder_parameters import InputEmbedderParameters
from coach_amd.architectures.layers import Dense
from coach_amd.base_parameters import EmbedderScheme, PresetValidationParameters, VisualizationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.gym_environment import GymVectorEnvironment
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters
from coach_amd.memories.memory import MemoryGranularity
from coach_amd.schedules import ConstantSchedule

BIT_LENGTH = 8


def agent_parameters(agent_seed=0):
    """the agent both BitFlip presets share (BitFlip_DQN.py:27-42)"""
    agent = DQNAgentParameters()
    agent.seed = agent_seed
    net = agent.network_wrappers['main']
    net.learning_rate = 0.001
    net.batch_size = 128
    net.middleware_parameters.scheme = [Dense(256)]
    net.input_embedders_parameters = {'state': InputEmbedderParameters(scheme=EmbedderScheme.Empty),
                                      'desired_goal': InputEmbedderParameters(scheme=EmbedderScheme.Empty)}
    alg = agent.algorithm
    alg.discount = 0.98
    alg.num_consecutive_playing_steps = EnvironmentEpisodes(16)
    alg.num_consecutive_training_steps = 40
    alg.num_steps_between_copying_online_weights_to_target = TrainingSteps(40)
    alg.rate_for_copying_weights_to_target = 0.05
    agent.memory.max_size = (MemoryGranularity.Transitions, 10**6)
    agent.exploration.epsilon_schedule = ConstantSchedule(0.2)
    agent.exploration.evaluation_epsilon = 0
    return agent


def environment_parameters(bit_length, num_envs=1, seed=1234):
    env = GymVectorEnvironment(level='rl_coach.environments.toy_problems.bit_flip:BitFlip')
    env.additional_simulator_parameters = {'bit_length': bit_length, 'mean_zero': True}
    env.custom_reward_threshold = -bit_length + 1
    env.num_envs, env.seed = num_envs, seed
    return env


def make(num_envs=1, seed=1234, agent_seed=0, bit_length=BIT_LENGTH):
    """seed: the environments' reset streams; agent_seed: the agent's host generators and initial weights."""
    sched = ScheduleParameters()
    sched.improve_steps = TrainingSteps(400000)
    sched.steps_between_evaluation_periods = EnvironmentEpisodes(16 * 50)      # 50 cycles
    sched.evaluation_steps = EnvironmentEpisodes(10)
    sched.heatup_steps = EnvironmentSteps(0)
    validation = PresetValidationParameters()
    validation.test = True
    validation.min_reward_threshold = -7.9
    validation.max_episodes_to_achieve_reward = 10000
    return BasicRLGraphManager(agent_params=agent_parameters(agent_seed),
                               env_params=environment_parameters(bit_length, num_envs, seed), schedule_params=sched,
                               vis_params=VisualizationParameters(), preset_validation_params=validation)


graph_manager = make()
