"""CartPole Quantile-Regression DQN for the device engine.

The experiment of rl_coach/presets/CartPole_QR_DQN.py: 50 atoms per action, discount .99, a target copy every 100
env-steps, one update per env-step, lr 5e-4 (the other network settings are QR-DQN's defaults: Adam epsilon 0.01 / 32,
kappa 1), a 40 k-transition uniform replay, epsilon 1 -> 0.01 over 10 k steps, 1 000 heat-up steps and one evaluation
episode every 10 episodes.  Its golden test is the reference's: an averaged evaluation reward of 150 within 250
episodes.  The level is CartPole-v0 on the device (coach_amd/environments/cartpole_vector_environment.py).
"""
from coach_amd.agents.qr_dqn_agent import QuantileRegressionDQNAgentParameters
from coach_amd.base_parameters import PresetValidationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters
from coach_amd.memories.memory import MemoryGranularity
from coach_amd.schedules import LinearSchedule

HYPER = dict(discount=0.99, target_copy_every=100, env_steps_per_update=1, atoms=50, learning_rate=5e-4,
             replay_transitions=40000, epsilon=(1.0, 0.01, 10000), heatup_steps=1000, episodes_between_evaluations=10)


def make(num_envs=1, seed=1234, agent_seed=0, **overrides):
    """seed: the environments' reset-state streams; agent_seed: the agent's host generators and initial weights."""
    h = dict(HYPER, **overrides)
    agent = QuantileRegressionDQNAgentParameters()
    agent.seed = agent_seed
    alg, net = agent.algorithm, agent.network_wrappers['main']
    alg.discount = h["discount"]
    alg.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(h["target_copy_every"])
    alg.num_consecutive_playing_steps = EnvironmentSteps(h["env_steps_per_update"])
    alg.atoms = h["atoms"]
    net.learning_rate = h["learning_rate"]
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
