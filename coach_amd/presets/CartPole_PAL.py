"""CartPole PAL (Persistent Advantage Learning) for the device engine.

The experiment of rl_coach/presets/CartPole_PAL.py, field by field (tests/golden/pal_preset.json): CartPole_DQN's
hyper-parameters — discount .99, a target copy every 100 env-steps, one update per env-step, lr 2.5e-4, MSE loss,
epsilon 1 -> 0.01 over 10 k steps, 1 000 heat-up steps, one evaluation episode every 10 episodes — with the PAL agent's
defaults (alpha 0.9, the non-persistent form, Monte Carlo mixing rate 0.1) and a 40 k-transition EPISODIC replay, and
its golden test: an averaged evaluation reward of 150 within 250 episodes (presets/CartPole_PAL.py:47-51).  The level is
CartPole-v0 on the device (coach_amd/environments/cartpole_vector_environment.py).
"""
from coach_amd.agents.pal_agent import PALAgentParameters
from coach_amd.base_parameters import PresetValidationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters
from coach_amd.memories.memory import MemoryGranularity
from coach_amd.presets.CartPole_DQN import HYPER
from coach_amd.schedules import LinearSchedule


def make(num_envs=1, seed=1234, agent_seed=0, agent_parameters=PALAgentParameters, **overrides):
    """seed: the environments' reset-state streams; agent_seed: the agent's host generators and initial weights;
    agent_parameters: the parameter class of the agent that runs the experiment (CartPole_MMC passes its own)."""
    h = dict(HYPER, **overrides)
    agent = agent_parameters()
    agent.seed = agent_seed
    alg, net = agent.algorithm, agent.network_wrappers['main']
    alg.discount = h["discount"]
    alg.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(h["target_copy_every"])
    alg.num_consecutive_playing_steps = EnvironmentSteps(h["env_steps_per_update"])
    net.learning_rate = h["learning_rate"]
    net.replace_mse_with_huber_loss = False
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
