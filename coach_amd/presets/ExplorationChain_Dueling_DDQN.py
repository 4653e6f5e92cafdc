"""ExplorationChain with Dueling Double DQN, for the device engine — the experiment of
rl_coach/presets/ExplorationChain_Dueling_DDQN.py, field by field (tests/golden/ucb_chain_presets.json): the baseline
the two ensemble presets are compared with.  ExplorationChain_UCB_Q_ensembles' chain and schedule (the level given as
plain GymEnvironmentParameters, as the reference does), a DDQN agent with the dueling head, lr 2.5e-4, discount .99, one
update per 4 env-steps, a 1 M-transition uniform replay, epsilon 1 -> 0.1 over 27 * 2 000 steps, no filters."""
from coach_amd.agents.ddqn_agent import DDQNAgentParameters
from coach_amd.architectures.head_parameters import DuelingQHeadParameters
from coach_amd.base_parameters import VisualizationParameters
from coach_amd.core_types import EnvironmentSteps
from coach_amd.environments.gym_environment import GymEnvironmentParameters
from coach_amd.filters.filter import NoInputFilter, NoOutputFilter
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager
from coach_amd.memories.memory import MemoryGranularity
from coach_amd.presets.ExplorationChain_UCB_Q_ensembles import N, environment_parameters, schedule_parameters
from coach_amd.schedules import LinearSchedule


def make(num_envs=1, agent_seed=0):
    agent = DDQNAgentParameters()
    agent.seed = agent_seed
    agent.network_wrappers['main'].learning_rate = 0.00025
    agent.network_wrappers['main'].heads_parameters = [DuelingQHeadParameters()]
    agent.memory.max_size = (MemoryGranularity.Transitions, 1000000)
    agent.algorithm.discount = 0.99
    agent.algorithm.num_consecutive_playing_steps = EnvironmentSteps(4)
    agent.exploration.epsilon_schedule = LinearSchedule(1, 0.1, (N + 7) * 2000)
    agent.input_filter = NoInputFilter()
    agent.output_filter = NoOutputFilter()
    return BasicRLGraphManager(agent_params=agent,
                               env_params=environment_parameters(GymEnvironmentParameters, num_envs=num_envs),
                               schedule_params=schedule_parameters(), vis_params=VisualizationParameters())


graph_manager = make()
