"""CartPole vanilla Policy Gradients for the device engine, with the hyper-parameters of rl_coach/presets/CartPole_PG.py:
discount .99, returns baselined per timestep (the agent's default rescaler), one update window per episode, the
accumulated gradients applied every 5 episodes, Adam with lr 5e-4, rewards rescaled by 1/200, no heat-up, one evaluation
episode every 20 episodes — and its golden test: an averaged evaluation reward of 130 within 550 episodes
(presets/CartPole_PG.py:42-45).  The level is CartPole-v0 on the device
(coach_amd/environments/cartpole_vector_environment.py: gym 0.12.5's physics)."""
from coach_amd.agents.policy_gradients_agent import PolicyGradientsAgentParameters
from coach_amd.base_parameters import PresetValidationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
from coach_amd.filters.filter import InputFilter
from coach_amd.filters.reward import RewardRescaleFilter
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters


def make(num_envs=1, seed=1234, agent_seed=0):
    """seed: the environments' reset-state streams; agent_seed: the agent's host generators and initial weights
    (the reference's `--seed`, rl_coach/tests/test_golden.py:122 runs its golden tests with 0)."""
    agent = PolicyGradientsAgentParameters()
    agent.seed = agent_seed
    alg, net = agent.algorithm, agent.network_wrappers['main']
    alg.discount = 0.99
    alg.apply_gradients_every_x_episodes = 5
    alg.num_steps_between_gradient_updates = 20000
    net.optimizer_type = 'Adam'
    net.learning_rate = 0.0005
    agent.input_filter = InputFilter()
    agent.input_filter.add_reward_filter('rescale', RewardRescaleFilter(1 / 200.))
    env = CartPoleVectorEnvironmentParameters(num_envs, "CartPole-v0", seed=seed)
    sched = ScheduleParameters()
    sched.improve_steps = TrainingSteps(10000000000)
    sched.steps_between_evaluation_periods = EnvironmentEpisodes(20)
    sched.evaluation_steps = EnvironmentEpisodes(1)
    sched.heatup_steps = EnvironmentSteps(0)
    validation = PresetValidationParameters(test=True, min_reward_threshold=130, max_episodes_to_achieve_reward=550)
    return BasicRLGraphManager(agent_params=agent, env_params=env, schedule_params=sched,
                               preset_validation_params=validation)


graph_manager = make()
