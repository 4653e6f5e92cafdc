"""CartPole DQN with the Boltzmann exploration policy: the CartPole_DQN preset of this package with its epsilon-greedy
policy swapped for rl_coach/exploration_policies/boltzmann.py — the agent samples its action from softmax(Q / T), with
the temperature T falling linearly from 1.0 to 0.01 over 10 000 acting steps (TEMPERATURE).  Same hyper-parameters and
the same golden bar as CartPole_DQN.
"""
from coach_amd.exploration_policies.boltzmann import BoltzmannParameters
from coach_amd.presets import CartPole_DQN
from coach_amd.schedules import LinearSchedule

TEMPERATURE = (1.0, 0.01, 10000)


def make(num_envs=1, seed=1234, agent_seed=0, temperature=TEMPERATURE, **overrides):
    gm = CartPole_DQN.make(num_envs=num_envs, seed=seed, agent_seed=agent_seed, **overrides)
    gm.agent_params.exploration = BoltzmannParameters()
    gm.agent_params.exploration.temperature_schedule = LinearSchedule(*temperature)
    return gm


graph_manager = make()
