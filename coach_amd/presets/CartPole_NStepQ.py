"""CartPole N-step Q for the device engine, with the hyper-parameters of rl_coach/presets/CartPole_NStepQ.py: 'N-Step'
targets, discount .99, update windows of 5 steps (t_max) and the accumulated gradients applied every episode (the
agent's defaults), Adam with lr 1e-4, the online weights copied to the target network every 100 environment steps,
rewards rescaled by 1/200, no heat-up, one evaluation episode every 10 episodes — and its golden test: an averaged
evaluation reward of 150 within 200 episodes, run by the reference with 8 asynchronous workers
(presets/CartPole_NStepQ.py:38-42); here `num_envs` lockstep envs feed one network, and the worker count is kept as
data.  The level is CartPole-v0 on the device (coach_amd/environments/cartpole_vector_environment.py: gym 0.12.5's
physics)."""
from coach_amd.agents.n_step_q_agent import NStepQAgentParameters
from coach_amd.base_parameters import PresetValidationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
from coach_amd.filters.filter import InputFilter
from coach_amd.filters.reward import RewardRescaleFilter
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters


def make(num_envs=1, seed=1234, agent_seed=0):
    """seed: the environments' reset-state streams; agent_seed: the agent's host generators and initial weights
    (the reference's `--seed`, rl_coach/tests/test_golden.py:122 runs its golden tests with 0)."""
    agent = NStepQAgentParameters()
    agent.seed = agent_seed
    alg, net = agent.algorithm, agent.network_wrappers['main']
    alg.discount = 0.99
    net.learning_rate = 0.0001
    alg.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(100)
    agent.input_filter = InputFilter()
    agent.input_filter.add_reward_filter('rescale', RewardRescaleFilter(1 / 200.))
    env = CartPoleVectorEnvironmentParameters(num_envs, "CartPole-v0", seed=seed)
    sched = ScheduleParameters()
    sched.improve_steps = TrainingSteps(10000000000)
    sched.steps_between_evaluation_periods = EnvironmentEpisodes(10)
    sched.evaluation_steps = EnvironmentEpisodes(1)
    sched.heatup_steps = EnvironmentSteps(0)
    validation = PresetValidationParameters(test=True, min_reward_threshold=150, max_episodes_to_achieve_reward=200,
                                            num_workers=8)
    return BasicRLGraphManager(agent_params=agent, env_params=env, schedule_params=sched,
                               preset_validation_params=validation)


graph_manager = make()
