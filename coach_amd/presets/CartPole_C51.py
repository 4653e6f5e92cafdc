"""CartPole Categorical DQN (C51) for the device engine.

The reference has no CartPole preset for this agent.  Schedule, replay size, target-copy period, update period and
validation bar are those of rl_coach/presets/CartPole_QR_DQN.py (discount .99, a target copy every 100 env-steps, one
update per env-step, a 40 k-transition uniform replay, 1 000 heat-up steps, one evaluation episode every 10 episodes, an
averaged evaluation reward of 150 within 250 episodes).  The support, learning rate and epsilon schedule were chosen on
the device: 51 atoms on [0, 100] — the discounted return of a 200-step episode at .99 is 86.6, so no target
reaches v_max, where the reference's projection drops the mass of clipped atoms.  The level is CartPole-v0 on the device
(coach_amd/environments/cartpole_vector_environment.py).
"""
from coach_amd.agents.categorical_dqn_agent import CategoricalDQNAgentParameters
from coach_amd.base_parameters import PresetValidationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters
from coach_amd.memories.memory import MemoryGranularity
from coach_amd.schedules import LinearSchedule

HYPER = dict(discount=0.99, target_copy_every=100, env_steps_per_update=1, v_min=0.0, v_max=100.0, atoms=51,
             learning_rate=5e-4, replay_transitions=40000, epsilon=(1.0, 0.01, 10000), heatup_steps=1000,
             episodes_between_evaluations=10)


def make(num_envs=1, seed=1234, agent_seed=0, **overrides):
    """seed: the environments' reset-state streams; agent_seed: the agent's host generators and initial weights."""
    h = dict(HYPER, **overrides)
    agent = CategoricalDQNAgentParameters()
    agent.seed = agent_seed
    alg, net = agent.algorithm, agent.network_wrappers['main']
    alg.discount = h["discount"]
    alg.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(h["target_copy_every"])
    alg.num_consecutive_playing_steps = EnvironmentSteps(h["env_steps_per_update"])
    alg.v_min, alg.v_max, alg.atoms = h["v_min"], h["v_max"], h["atoms"]
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
