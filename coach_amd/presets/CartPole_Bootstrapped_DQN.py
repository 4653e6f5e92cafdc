"""CartPole Bootstrapped DQN for the device engine — a preset of this package, not one of the reference's (it ships
Bootstrapped DQN for Atari and for its ExplorationChain environment only).

CartPole_DQN's experiment — discount .99, a target copy every 100 env-steps, one update per env-step, lr 2.5e-4, MSE
loss, a 40 k-transition uniform replay, epsilon 1 -> 0.01 over 10 k steps, 1 000 heat-up steps, one evaluation episode
every 10 episodes — with the Bootstrapped defaults: 10 heads, data-sharing probability 1, the heads' gradient into the
torso scaled by 1 / 10.  Its bar is the one the reference sets for its CartPole DQN-family presets: an averaged
evaluation reward of 150 within 250 episodes.  Evaluation acts by the heads' majority vote.
"""
from coach_amd.agents.bootstrapped_dqn_agent import BootstrappedDQNAgentParameters
from coach_amd.base_parameters import PresetValidationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters
from coach_amd.memories.memory import MemoryGranularity
from coach_amd.presets.CartPole_DQN import HYPER as DQN_HYPER
from coach_amd.schedules import LinearSchedule

HYPER = dict(DQN_HYPER, heads=10, data_sharing_probability=1.0)


def make(num_envs=1, seed=1234, agent_seed=0, **overrides):
    """seed: the environments' reset-state streams; agent_seed: the agent's host generators and initial weights."""
    h = dict(HYPER, **overrides)
    agent = BootstrappedDQNAgentParameters()
    agent.seed = agent_seed
    alg, net = agent.algorithm, agent.network_wrappers['main']
    alg.discount = h["discount"]
    alg.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(h["target_copy_every"])
    alg.num_consecutive_playing_steps = EnvironmentSteps(h["env_steps_per_update"])
    net.learning_rate = h["learning_rate"]
    net.replace_mse_with_huber_loss = False
    head = net.heads_parameters[0]
    head.num_output_head_copies = h["heads"]
    head.rescale_gradient_from_head_by_factor = 1.0 / h["heads"]
    agent.exploration.architecture_num_q_heads = h["heads"]
    agent.exploration.bootstrapped_data_sharing_probability = h["data_sharing_probability"]
    agent.memory.max_size = (MemoryGranularity.Transitions, h["replay_transitions"])
    agent.exploration.epsilon_schedule = LinearSchedule(*h["epsilon"])
    sched = ScheduleParameters()
    sched.heatup_steps = EnvironmentSteps(h["heatup_steps"])
    sched.evaluation_steps = EnvironmentEpisodes(1)
    sched.improve_steps = TrainingSteps(10000000000)
    sched.steps_between_evaluation_periods = EnvironmentEpisodes(h["episodes_between_evaluations"])
    env = CartPoleVectorEnvironmentParameters(num_envs, "CartPole-v0", seed=seed)
    validation = PresetValidationParameters(test=True, min_reward_threshold=150, max_episodes_to_achieve_reward=250)
    return BasicRLGraphManager(agent_params=agent, env_params=env, schedule_params=sched,
                               preset_validation_params=validation)


graph_manager = make()
