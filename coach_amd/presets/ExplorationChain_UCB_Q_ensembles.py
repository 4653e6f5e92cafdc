"""ExplorationChain with UCB over a Q ensemble, for the device engine — the experiment of
rl_coach/presets/ExplorationChain_UCB_Q_ensembles.py, field by field (tests/golden/ucb_chain_presets.json):
the chain of N = 20 states with a 27-step limit (`max_steps = N + 7`), Therm observations, start state 1,
reward 0.001 at the left end and 1 at the right end; a Bootstrapped DQN agent with 20 heads (the heads'
gradient into the torso scaled by 1 / 20, data-sharing probability 1) explored by UCB with lamb = 10 and a constant
epsilon of 0, lr 2.5e-4, discount .99, one update per 4 env-steps, a 1 M-transition uniform replay, no input and no
output filter; 20 heat-up steps, 2 000 training episodes, one evaluation episode every 10.  The level is ExplorationChain
on the device (coach_amd/environments/exploration_chain_vector_environment.py).  The reference sets no bar; from start
state 1 the best return is 10.0 (the right end reached at step 18, reward 1 on steps 18 .. 27) and never leaving the left
end gives at most 27 * 0.001.  `make(num_envs=...)` runs more envs per GPU."""
from coach_amd.agents.bootstrapped_dqn_agent import BootstrappedDQNAgentParameters
from coach_amd.base_parameters import VisualizationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps
from coach_amd.environments.gym_environment import GymVectorEnvironment
from coach_amd.exploration_policies.ucb import UCBParameters
from coach_amd.filters.filter import NoInputFilter, NoOutputFilter
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters
from coach_amd.memories.memory import MemoryGranularity
from coach_amd.schedules import ConstantSchedule

N = 20
HEADS = 20


def schedule_parameters():
    """the schedule the three ExplorationChain presets share"""
    sched = ScheduleParameters()
    sched.improve_steps = EnvironmentEpisodes(2000)
    sched.steps_between_evaluation_periods = EnvironmentEpisodes(10)
    sched.evaluation_steps = EnvironmentEpisodes(1)
    sched.heatup_steps = EnvironmentSteps(N)
    return sched


def environment_parameters(cls=GymVectorEnvironment, num_envs=1):
    env = cls(level='rl_coach.environments.toy_problems.exploration_chain:ExplorationChain')
    env.additional_simulator_parameters = {'chain_length': N, 'max_steps': N + 7}
    env.num_envs = num_envs
    return env


def ensemble_agent_parameters(agent_seed=0):
    """the 20-head agent ExplorationChain_Bootstrapped_DQN and this preset share, with the agent's own exploration"""
    agent = BootstrappedDQNAgentParameters()
    agent.seed = agent_seed
    net = agent.network_wrappers['main']
    net.learning_rate = 0.00025
    net.heads_parameters[0].num_output_head_copies = HEADS
    net.heads_parameters[0].rescale_gradient_from_head_by_factor = 1.0 / HEADS
    agent.memory.max_size = (MemoryGranularity.Transitions, 1000000)
    agent.algorithm.discount = 0.99
    agent.algorithm.num_consecutive_playing_steps = EnvironmentSteps(4)
    agent.input_filter = NoInputFilter()
    agent.output_filter = NoOutputFilter()
    return agent


def make(num_envs=1, agent_seed=0):
    agent = ensemble_agent_parameters(agent_seed)
    agent.exploration = UCBParameters()
    agent.exploration.bootstrapped_data_sharing_probability = 1.0
    agent.exploration.architecture_num_q_heads = HEADS
    agent.exploration.epsilon_schedule = ConstantSchedule(0)
    agent.exploration.lamb = 10
    return BasicRLGraphManager(agent_params=agent, env_params=environment_parameters(num_envs=num_envs),
                               schedule_params=schedule_parameters(), vis_params=VisualizationParameters())


graph_manager = make()
