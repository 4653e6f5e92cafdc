"""CartPole Direct Future Prediction for the device engine — rl_coach/presets/CartPole_DFP.py: learning rate 1e-4, the
three input embedders Medium (Dense 256, leaky_relu), epsilon 0.5 -> 0.01 over 3000 steps (0.01 when evaluating),
discount 1, the accumulated reward as THE measurement with goal [1], one update per env-step, targets past an episode's
end taken from its last step, 100 heat-up steps, one evaluation episode every 10 episodes; the bar is an averaged
evaluation reward of 120 within 250 episodes.  The level is CartPole-v0 on the device
(coach_amd/environments/cartpole_vector_environment.py).
"""
from coach_amd.agents.dfp_agent import DFPAgentParameters, HandlingTargetsAfterEpisodeEnd
from coach_amd.base_parameters import EmbedderScheme, PresetValidationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters
from coach_amd.schedules import LinearSchedule

HYPER = dict(learning_rate=0.0001, epsilon=(0.5, 0.01, 3000), evaluation_epsilon=0.01, discount=1.0,
             env_steps_per_update=1, goal_vector=[1], heatup_steps=100, episodes_between_evaluations=10)


def make(num_envs=1, seed=1234, agent_seed=0, **overrides):
    """seed: the environments' reset-state streams; agent_seed: the agent's host generators and initial weights."""
    h = dict(HYPER, **overrides)
    agent = DFPAgentParameters()
    agent.seed = agent_seed
    alg, net = agent.algorithm, agent.network_wrappers['main']
    net.learning_rate = h["learning_rate"]
    for name in ('observation', 'goal', 'measurements'):
        net.input_embedders_parameters[name].scheme = EmbedderScheme.Medium
    agent.exploration.epsilon_schedule = LinearSchedule(*h["epsilon"])
    agent.exploration.evaluation_epsilon = h["evaluation_epsilon"]
    alg.discount = h["discount"]
    alg.use_accumulated_reward_as_measurement = True
    alg.num_consecutive_playing_steps = EnvironmentSteps(h["env_steps_per_update"])
    alg.goal_vector = list(h["goal_vector"])           # accumulated_reward
    alg.handling_targets_after_episode_end = HandlingTargetsAfterEpisodeEnd.LastStep
    sched = ScheduleParameters()
    sched.heatup_steps = EnvironmentSteps(h["heatup_steps"])
    sched.evaluation_steps = EnvironmentEpisodes(1)
    sched.improve_steps = TrainingSteps(10000000000)
    sched.steps_between_evaluation_periods = EnvironmentEpisodes(h["episodes_between_evaluations"])
    env = CartPoleVectorEnvironmentParameters(num_envs, "CartPole-v0", seed=seed)
    validation = PresetValidationParameters(test=True, min_reward_threshold=120, max_episodes_to_achieve_reward=250)
    return BasicRLGraphManager(agent_params=agent, env_params=env, schedule_params=sched,
                               preset_validation_params=validation)


graph_manager = make()
