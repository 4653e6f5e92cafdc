"""CartPole DQN with the ParameterNoise exploration policy: the CartPole_DQN preset of this package with its
epsilon-greedy policy swapped for rl_coach/exploration_policies/parameter_noise.py — every dense layer of the Q network
is a factorised NoisyNet layer and the agent acts by plain argmax.  Same hyper-parameters, and the golden bar the
reference sets for its CartPole DQN-family presets, the noisy-net CartPole_Rainbow included
(presets/CartPole_Rainbow.py:48-51): an evaluation reward of 150 within 250 episodes.
"""
from coach_amd.exploration_policies.parameter_noise import ParameterNoiseParameters
from coach_amd.presets import CartPole_DQN


def make(num_envs=1, seed=1234, agent_seed=0, **overrides):
    gm = CartPole_DQN.make(num_envs=num_envs, seed=seed, agent_seed=agent_seed, **overrides)
    gm.agent_params.exploration = ParameterNoiseParameters(gm.agent_params)
    return gm


graph_manager = make()
