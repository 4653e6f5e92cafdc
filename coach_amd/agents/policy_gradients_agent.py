"""Vanilla Policy Gradients on one MI355X — host-side mirror of rl_coach/agents/policy_gradients_agent.py (parameter
classes :35-84, PolicyGradientsAgent :87-133) over the on-policy base (agents/policy_optimization_agent.py).

Per vector step: states -> the policy network's logits -> softmax + categorical draw (host uniforms, reference order) ->
the 'Entropy' sample -> env.step -> reward filter -> the env's episode row.
Per update window (by default a whole episode: num_steps_between_gradient_updates = 20000): ONE launch,
rlx_pg_episode_window, restates the returns of the episode (n_step -1), update_episode_statistics, the rescaling loop
with its quirks and the 'Returns Mean' / 'Returns Variance' samples, and leaves the fp32 advantages column; forward on the
window's states; ONE launch, rlx_pg_head_loss, gives -mean(log pi(a) * advantage) - beta * mean entropy and dlogits;
backward; accumulated += gradients.  Every apply_gradients_every_x_episodes episodes: one TF1 Adam step.
Discrete action spaces only: the continuous PolicyHead (and with it AdditiveNoise exploration) is not served.
"""
import torch

from .. import _rlx
from ..architectures.head_parameters import PolicyHeadParameters
from ..architectures.scheme_views import SchemeViews
from ..exploration_policies.categorical import CategoricalParameters
from ..memories.episodic.single_episode_buffer import SingleEpisodeBufferParameters
from ..nn.networks import PolicyGradientNet, policy_gradient_net_kwargs
from .policy_optimization_agent import PolicyGradientRescaler, PolicyOptimizationAgent
from .vector_agent import AlgorithmParameters


class PolicyGradientNetworkParameters(SchemeViews):      # policy_gradients_agent.py:35-41 + NetworkParameters defaults
    def __init__(self):
        self.activation_function = 'relu'
        self.embedder_scheme = 'Medium'
        self.middleware_scheme = 'Medium'
        self.heads_parameters = [PolicyHeadParameters()]
        self.async_training = True
        self.optimizer_type = 'Adam'
        self.batch_size = 32
        self.create_target_network = False
        self.learning_rate = 0.00025
        self.adam_optimizer_beta1 = 0.9
        self.adam_optimizer_beta2 = 0.99
        self.optimizer_epsilon = 0.0001
        self.scale_down_gradients_by_number_of_workers_for_sync_training = True
        self.clip_gradients = None                       # ClipByGlobalNorm threshold (base_parameters.py)


class PolicyGradientAlgorithmParameters(AlgorithmParameters):          # policy_gradients_agent.py:44-71
    def __init__(self):
        super().__init__()
        self.policy_gradient_rescaler = PolicyGradientRescaler.FUTURE_RETURN_NORMALIZED_BY_TIMESTEP
        self.apply_gradients_every_x_episodes = 5
        self.beta_entropy = 0
        self.num_steps_between_gradient_updates = 20000  # this is called t_max in all the papers


class PolicyGradientsAgentParameters(object):            # policy_gradients_agent.py:74-84
    def __init__(self):
        self.algorithm = PolicyGradientAlgorithmParameters()
        # the reference maps DiscreteActionSpace -> Categorical, BoxActionSpace -> AdditiveNoise; the Box branch needs
        # the continuous PolicyHead, which is not served
        self.exploration = CategoricalParameters()
        self.memory = SingleEpisodeBufferParameters()
        self.network_wrappers = {"main": PolicyGradientNetworkParameters()}
        self.seed = 0

    @property
    def path(self):
        return 'coach_amd.agents.policy_gradients_agent:PolicyGradientsAgent'


_RESCALERS = (PolicyGradientRescaler.TOTAL_RETURN, PolicyGradientRescaler.FUTURE_RETURN,
              PolicyGradientRescaler.FUTURE_RETURN_NORMALIZED_BY_EPISODE,
              PolicyGradientRescaler.FUTURE_RETURN_NORMALIZED_BY_TIMESTEP)


class PolicyGradientsAgent(PolicyOptimizationAgent):
    SIGNAL_NAMES = PolicyOptimizationAgent.SIGNAL_NAMES + ["Returns Mean", "Returns Variance"]      # :90-91

    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        rescaler = agent_parameters.algorithm.policy_gradient_rescaler
        if rescaler not in _RESCALERS:
            # the reference only warns and trains on the raw returns (:117-118); here the launch has no such branch
            raise ValueError("The requested policy gradient rescaler is not available: {} (vanilla Policy Gradients "
                             "rescales by one of {})".format(rescaler, [r.name for r in _RESCALERS]))
        super().__init__(agent_parameters, environment, device, dist, use_graphs)
        dev, L = self.device, self.L
        self.returns = torch.zeros(L, dtype=torch.float64, device=dev)      # n_step_discounted_rewards of the episode
        self.rescaled_returns = torch.zeros(L, dtype=torch.float64, device=dev)
        self.advantages = torch.zeros(L, dtype=torch.float32, device=dev)   # the head's fp32 placeholder
        self.window_stats = torch.zeros(4, dtype=torch.float64, device=dev)  # Returns Mean, Returns Variance, episode mean, std

    def _make_network(self, obs_shape, wrapper):
        return PolicyGradientNet(self.device, obs_shape, self.A,
                                 **policy_gradient_net_kwargs(wrapper, self.ap.algorithm, self.ap.seed or 0))

    def _window_device(self, env, start, end, complete):
        """learn_from_batch (:98-133) on steps [start, end) of env's episode, preceded by what train() does to the
        episode first (the returns, update_episode_statistics)."""
        alg, net, s = self.ap.algorithm, self.networks["main"], _rlx.current_stream()
        obs, actions, rewards = self.memory.episode_rows(env, start, end)
        self.lib.pg_episode_window(rewards, end, start, float(alg.discount), int(self.policy_gradient_rescaler.value),
                                   self.mean_return_over_multiple_episodes, self.num_episodes_where_step_has_been_seen,
                                   self.max_episode_length, self.returns, self.rescaled_returns, self.advantages,
                                   self.window_stats, self.status, s)
        loss = net.accumulate_window(obs, end - start, actions, self.advantages)
        self.signals = {"Loss": net.loss, "Grads (unclipped)": net.norm, "Returns Mean": self.window_stats[0:1],
                        "Returns Variance": self.window_stats[1:2]}
        if complete:                                     # handle_episode_ended: a sample per transition (agent.py:569-570)
            self.signals["Discounted Return"] = self.returns[:end]
        return loss
