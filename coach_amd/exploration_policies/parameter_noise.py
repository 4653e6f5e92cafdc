"""ParameterNoise for N lockstep envs — mirror of rl_coach/exploration_policies/parameter_noise.py
(ParameterNoiseParameters :29-41, ParameterNoise :44-90).

The policy explores through the network, not through the action: every dense layer of the agent's networks (input
embedders, middleware, heads — `_replace_network_dense_layers`, :79-90) becomes a factorised NoisyNet layer
(architectures.layers.NoisyNetDense -> nn.graph.NoisyDense, csrc/noisy_dense.hip) that samples new noise for every
forward pass, and the action is np.argmax of the action values (:62-68): the FIRST maximum, no epsilon, no random
tie-break, no host draw.  The agent's acting kernel does that reduction on the device (rlx_argmax_rows on fp32 Q values,
rlx_quantile_argmax / rlx_categorical_argmax on the distributional agents' fp64 action values).  Evaluation phases keep
sampling noise, as the reference does.  Continuous action spaces (:69-72) are not served.
"""
from ..architectures.layers import NoisyNetDense
from ..core_types import RunPhase


def _components(network_wrapper_params):
    return list(network_wrapper_params.input_embedders_parameters.values()) + \
        [network_wrapper_params.middleware_parameters] + list(network_wrapper_params.heads_parameters)


def replace_network_dense_layers(network_params):
    """parameter_noise.py:79-90: dense_layer = NoisyNetDense on every component of every network wrapper."""
    for network_wrapper_params in network_params.values():
        for component_params in _components(network_wrapper_params):
            component_params.dense_layer = NoisyNetDense


def network_is_noisy(network_wrapper_params):
    """has ParameterNoise marked this network wrapper?  (all of its components, or none)"""
    marks = [getattr(c, "dense_layer", None) is NoisyNetDense for c in _components(network_wrapper_params)]
    if any(marks) and not all(marks):
        raise ValueError("a network with noisy dense layers in some components only is not supported")
    return all(marks)


class ParameterNoiseParameters(object):                  # parameter_noise.py:29-41
    """Constructing it MARKS agent_params.network_wrappers (dense_layer = NoisyNetDense on every component).  The marks
    stay: assigning another exploration policy to the same agent parameters afterwards leaves noisy networks under a
    policy that is not ParameterNoise, which the agents refuse with a ValueError ("... come together") — build fresh
    agent parameters instead."""

    def __init__(self, agent_params):
        if not getattr(agent_params.algorithm, "supports_parameter_noise", False):
            raise ValueError("Currently only DQN variants are supported for using an exploration type of "
                             "ParameterNoise.")
        self.network_params = agent_params.network_wrappers
        # (the reference marks the networks when the policy object is built, which is before its networks are; here
        # the agent builds its network first, so the parameters object marks them)
        replace_network_dense_layers(self.network_params)

    @property
    def path(self):
        return 'coach_amd.exploration_policies.parameter_noise:ParameterNoise'


class ParameterNoise(object):
    def __init__(self, num_actions, n_env, device, params):
        self.A, self.n_env, self.device = num_actions, n_env, device
        self.network_params = params.network_params
        replace_network_dense_layers(self.network_params)
        self.phase = RunPhase.HEATUP

    def get_control_param(self):                         # :76-77
        return 0

    def epsilon(self):
        return 0.0
