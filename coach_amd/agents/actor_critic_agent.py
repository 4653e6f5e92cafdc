"""Actor-Critic (A3C) on one MI355X — host-side mirror of rl_coach/agents/actor_critic_agent.py (parameter classes
:36-90, ActorCriticAgent :94-190) over the on-policy base (agents/policy_optimization_agent.py).

Per vector step: states -> the policy head's logits (the V head is not run when acting) -> softmax + categorical draw
(host uniforms, reference order) -> the 'Entropy' sample -> env.step -> reward filter -> the env's episode row, with its
game-over byte and the observation before the reset.
Per update window (num_steps_between_gradient_updates visible steps, or the rest of a finished episode): forward on the
window's T states and on the state behind them (T + 1 rows, read in place while the episode runs); ONE launch,
rlx_a3c_window_loss (csrc/a3c.hip), restates learn_from_batch :138-165 — R = 0 on a game over or the bootstrap V, the
A_VALUE loop or the GAE recurrences in the reference's order and rounding, the fp32 placeholders — and both heads' losses
and gradients; backward; accumulated += gradients.  Every apply_gradients_every_x_episodes episodes: one TF1 Adam step.
Neither V nor the targets leave the device.  The window, pointer and apply cadence are the base's.
Discrete action spaces only: the continuous PolicyHead (and with it ContinuousEntropy exploration) is not served.
"""
import torch

from .. import _rlx
from ..architectures.head_parameters import PolicyHeadParameters, VHeadParameters
from ..architectures.scheme_views import SchemeViews
from ..exploration_policies.categorical import CategoricalParameters
from ..memories.episodic.single_episode_buffer import SingleEpisodeBufferParameters
from ..nn.networks import ActorCriticNet, actor_critic_net_kwargs
from .policy_optimization_agent import PolicyGradientRescaler, PolicyOptimizationAgent
from .vector_agent import AlgorithmParameters


class ActorCriticAlgorithmParameters(AlgorithmParameters):            # actor_critic_agent.py:36-66
    def __init__(self):
        super().__init__()
        self.policy_gradient_rescaler = PolicyGradientRescaler.A_VALUE
        self.apply_gradients_every_x_episodes = 5
        self.beta_entropy = 0
        self.num_steps_between_gradient_updates = 5000  # this is called t_max in all the papers
        self.gae_lambda = 0.96
        self.estimate_state_value_using_gae = False


class ActorCriticNetworkParameters(SchemeViews):         # actor_critic_agent.py:69-77 + NetworkParameters defaults
    def __init__(self):
        self.activation_function = 'relu'
        self.embedder_scheme = 'Medium'
        self.middleware_scheme = 'Medium'
        self.heads_parameters = [VHeadParameters(loss_weight=0.5), PolicyHeadParameters(loss_weight=1.0)]
        self.async_training = True
        self.optimizer_type = 'Adam'
        self.batch_size = 32
        self.create_target_network = False
        self.learning_rate = 0.00025
        self.adam_optimizer_beta1 = 0.9
        self.adam_optimizer_beta2 = 0.99
        self.optimizer_epsilon = 0.0001
        self.scale_down_gradients_by_number_of_workers_for_sync_training = True
        self.clip_gradients = 40.0                       # ClipByGlobalNorm threshold (base_parameters.py)


class ActorCriticAgentParameters(object):                # actor_critic_agent.py:80-90
    def __init__(self):
        self.algorithm = ActorCriticAlgorithmParameters()
        # the reference maps DiscreteActionSpace -> Categorical, BoxActionSpace -> ContinuousEntropy; the Box branch needs
        # the continuous PolicyHead, which is not served
        self.exploration = CategoricalParameters()
        self.memory = SingleEpisodeBufferParameters()
        self.network_wrappers = {"main": ActorCriticNetworkParameters()}
        self.seed = 0

    @property
    def path(self):
        return 'coach_amd.agents.actor_critic_agent:ActorCriticAgent'


_RESCALERS = (PolicyGradientRescaler.A_VALUE, PolicyGradientRescaler.GAE)


class ActorCriticAgent(PolicyOptimizationAgent):
    SIGNAL_NAMES = PolicyOptimizationAgent.SIGNAL_NAMES + ["Advantages", "Values", "Value Loss", "Policy Loss"]  # :98-101

    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        rescaler = agent_parameters.algorithm.policy_gradient_rescaler
        if rescaler not in _RESCALERS:
            # the reference only warns and trains on zero targets and advantages (:166-167); here the launch has no such
            # branch
            raise ValueError("The requested policy gradient rescaler is not available: {} (Actor-Critic rescales by one "
                             "of {})".format(rescaler, [r.name for r in _RESCALERS]))
        super().__init__(agent_parameters, environment, device, dist, use_graphs)
        dev, L = self.device, self.L
        self.value_targets = torch.zeros(L, dtype=torch.float64, device=dev)     # state_value_head_targets of the window
        self.advantages = torch.zeros(L, dtype=torch.float64, device=dev)        # action_advantages of the window
        self.returns = torch.zeros(L, dtype=torch.float64, device=dev)           # a finished episode's discounted returns
        self.debug_targets = None        # tests set this to a list: (V, value targets, advantages) clones per window

    def _make_network(self, obs_shape, wrapper):
        return ActorCriticNet(self.device, obs_shape, self.A,
                              **actor_critic_net_kwargs(wrapper, self.ap.algorithm, self.ap.seed or 0))

    def _window_device(self, env, start, end, complete):
        """learn_from_batch (:127-186) on steps [start, end) of env's episode.  The bootstrap state is always forwarded
        (one more row): whether the last transition is a game over is a device fact, and the launch gives that row no
        term and a zero gradient."""
        alg, net, T = self.ap.algorithm, self.networks["main"], end - start
        obs, actions, rewards = self.memory.episode_rows(env, start, end)
        rows, last_next_state, game_over = self.memory.bootstrap_rows(env, start, end, complete)
        if rows is None:                                 # the reset overwrote the state behind a finished episode
            rows = net.stage_rows(obs, last_next_state)
        loss = net.accumulate_window(rows, T, True, actions, self.value_targets, self.advantages, rewards[start:end],
                                     game_over, alg.discount, alg.gae_lambda, self.policy_gradient_rescaler.value,
                                     alg.estimate_state_value_using_gae)
        self.signals = {"Loss": net.loss, "Grads (unclipped)": net.norm, "Values": net.values[:T],
                        "Advantages": self.advantages[:T], "Value Loss": net.value_loss, "Policy Loss": net.policy_loss}
        if complete:                                     # handle_episode_ended: a sample per transition (agent.py:569-570)
            self.lib.episode_nstep_returns(rewards, None, self.returns, 0, end, 0, 1, end, float(alg.discount), -1,
                                           _rlx.current_stream())
            self.signals["Discounted Return"] = self.returns[:end]
        if self.debug_targets is not None:
            self.debug_targets.append((net.values[:T + 1].clone(), self.value_targets[:T].clone(),
                                       self.advantages[:T].clone(), game_over.clone()))
        return loss

    def check_status(self):
        super().check_status()
        self.networks["main"].check_status()
