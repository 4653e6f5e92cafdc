"""CartPole DQN with the dense layers' products on the bf16 matrix pipe: the CartPole_DQN preset of this package with
`network_wrappers['main'].precision = "bf16"` (a device-engine addition, base_parameters.NetworkParameters) — weights,
activations, gradients and the Adam state stay fp32; every product rounds its operands to bf16 and sums in fp32.  Same
hyper-parameters and the same golden bar as CartPole_DQN.
"""
from coach_amd.presets import CartPole_DQN


def make(num_envs=1, seed=1234, agent_seed=0, **overrides):
    gm = CartPole_DQN.make(num_envs=num_envs, seed=seed, agent_seed=agent_seed, **overrides)
    gm.agent_params.network_wrappers['main'].precision = "bf16"
    return gm


graph_manager = make()
