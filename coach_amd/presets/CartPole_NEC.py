"""CartPole NEC for the device engine.

The experiment of rl_coach/presets/CartPole_NEC.py, field by field: lr 2.5e-4, epsilon 0.5 -> 0.1 over 1 000 steps,
evaluation epsilon 0, discount .99, an episodic replay of 200 episodes, rewards rescaled by 1 / 200, 1 300 heat-up steps,
one evaluation episode every 10 episodes, and the agent's defaults (dnd_size 500 000, 50 neighbours, n_step 100, one
update per 4 env-steps); its golden bar is an averaged evaluation reward of 150 within 300 episodes
(presets/CartPole_NEC.py:41-46).  The level is CartPole-v0 on the device.  `dnd_size` is an override here because the
default tables take 2 x 500 000 x 512 floats = 2 GB of keys.
"""
from coach_amd.agents.nec_agent import NECAgentParameters
from coach_amd.base_parameters import PresetValidationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters
from coach_amd.memories.memory import MemoryGranularity
from coach_amd.schedules import LinearSchedule

HYPER = dict(discount=0.99, learning_rate=0.00025, epsilon=(0.5, 0.1, 1000), evaluation_epsilon=0,
             replay_episodes=200, reward_rescale=1 / 200., heatup_steps=1300, episodes_between_evaluations=10,
             dnd_size=500000)


def make(num_envs=1, seed=1234, agent_seed=0, **overrides):
    h = dict(HYPER, **overrides)
    agent = NECAgentParameters()
    agent.seed = agent_seed
    agent.network_wrappers['main'].learning_rate = h["learning_rate"]
    agent.exploration.epsilon_schedule = LinearSchedule(*h["epsilon"])
    agent.exploration.evaluation_epsilon = h["evaluation_epsilon"]
    agent.algorithm.discount = h["discount"]
    agent.algorithm.dnd_size = h["dnd_size"]
    agent.algorithm.reward_rescale = h["reward_rescale"]
    agent.memory.max_size = (MemoryGranularity.Episodes, h["replay_episodes"])
    sched = ScheduleParameters()
    sched.improve_steps = TrainingSteps(10000000000)
    sched.steps_between_evaluation_periods = EnvironmentEpisodes(h["episodes_between_evaluations"])
    sched.evaluation_steps = EnvironmentEpisodes(1)
    sched.heatup_steps = EnvironmentSteps(h["heatup_steps"])
    env = CartPoleVectorEnvironmentParameters(num_envs, "CartPole-v0", seed=seed)
    validation = PresetValidationParameters(test=True, min_reward_threshold=150, max_episodes_to_achieve_reward=300)
    return BasicRLGraphManager(agent_params=agent, env_params=env, schedule_params=sched,
                               preset_validation_params=validation)


graph_manager = make()
