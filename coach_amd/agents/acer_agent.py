"""ACER (Actor-Critic with Experience Replay) on one MI355X — host-side mirror of rl_coach/agents/acer_agent.py
(parameter classes :32-98, ACERAgent :102-201) over the on-policy base (agents/policy_optimization_agent.py): the one
member of the family that joins the on-policy windows to a replay memory.

Per vector step: states -> the policy head's logits (the Q head is not run when acting) -> softmax + categorical draw
(host uniforms, reference order) -> the 'Entropy' sample -> env.step -> reward filter -> the env's episode row, with its
game-over byte, the observation before the reset and the acting step's probabilities `mu`
(info['all_action_probabilities']).  When an env's episode ends, its rows enter the replay of complete episodes
(memories/episodic/episode_store.py), before that step's train().
Per update window (num_steps_between_gradient_updates visible steps, or the rest of a finished episode; the gate,
pointer and cadence are the base's), learn_from_batch :182-197:
  * the on-policy window, _learn_from_batch on the staging rows: the online network forward on the window's T states and
    the state behind them (always forwarded: whether the last transition is a game over is a device fact), the average
    (target) network's policy head on the T states, ONE launch, rlx_acer_window_loss (csrc/acer.hip) — state values,
    importance weights, the Q-retrace recurrence in the reference's order and rounding, both heads' losses and
    gradients — backward; the gradients REPLACE the gradient buffer and are applied at once (one TF1 Adam step); the
    average network moves by rate_for_copying_weights_to_target;
  * then, when ratio_of_replay > 0 and the memory holds more than num_transitions_to_start_replay transitions,
    n = np.random.poisson(ratio_of_replay) replayed windows of num_steps_between_gradient_updates consecutive transitions
    of one complete episode, each a contiguous slice of the store read in place, each with its own forward, launch,
    backward, Adam step and average-network move.  The host generator is consumed in the reference's order: the Poisson
    draw, then per window the episode index and (only for an episode longer than the window) the window's end.
The base's apply step stays as the reference has it: when current_episode % apply_gradients_every_x_episodes == 0 the
gradient buffer — which still holds the LAST window's gradients — is applied once more and then cleared
(network_wrapper.py:179-203).  `networks['main'].adam_steps` counts every Adam step.

The reference's use_trust_region_optimization changes no gradient there: ACERPolicyHead builds its losses from
policy_probs before `self.output = trust_region_layer(self.output)`, and tf.gradients(total_loss, weights) never passes
through that identity tensor.  The faithful default therefore computes and logs the KL and leaves the
gradient alone; `apply_trust_region_to_gradients` (a field of this package, default False) applies the layer's gradient
to dL/dp inside the launch — a deliberate divergence.
Nothing of a window leaves the device.  Discrete action spaces only, as in the reference; image observations and
data-parallel training are refused by the base.
"""
import numpy as np
import torch

from .. import _rlx
from ..architectures.head_parameters import ACERPolicyHeadParameters, QHeadParameters
from ..architectures.scheme_views import SchemeViews
from ..exploration_policies.categorical import CategoricalParameters
from ..memories.episodic.episode_store import EpisodeStore
from ..memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters
from ..memories.episodic.single_episode_buffer import SingleEpisodeBuffer
from ..nn.networks import ACERNet, acer_net_kwargs
from .policy_optimization_agent import PolicyOptimizationAgent
from .vector_agent import AlgorithmParameters


class ACERAlgorithmParameters(AlgorithmParameters):      # acer_agent.py:32-75
    def __init__(self):
        super().__init__()
        self.apply_gradients_every_x_episodes = 5
        self.num_steps_between_gradient_updates = 5000   # this is called t_max in all the papers
        self.ratio_of_replay = 4
        self.num_transitions_to_start_replay = 10000
        self.rate_for_copying_weights_to_target = 0.01
        self.importance_weight_truncation = 10.0
        self.use_trust_region_optimization = True        # builds a layer no gradient passes through (see the module text)
        self.max_KL_divergence = 1.0
        self.beta_entropy = 0
        # this package's: apply the trust-region layer's gradient to dL/dp (the reference never does)
        self.apply_trust_region_to_gradients = False


class ACERNetworkParameters(SchemeViews):                # acer_agent.py:78-87 + NetworkParameters defaults
    def __init__(self):
        self.activation_function = 'relu'
        self.embedder_scheme = 'Medium'
        self.middleware_scheme = 'Medium'
        self.heads_parameters = [QHeadParameters(loss_weight=0.5), ACERPolicyHeadParameters(loss_weight=1.0)]
        self.optimizer_type = 'Adam'
        self.async_training = True
        self.shared_optimizer = True
        self.clip_gradients = 40.0                      # ClipByGlobalNorm threshold (base_parameters.py)
        self.create_target_network = True
        self.batch_size = 32
        self.learning_rate = 0.00025
        self.adam_optimizer_beta1 = 0.9
        self.adam_optimizer_beta2 = 0.99
        self.optimizer_epsilon = 0.0001
        self.scale_down_gradients_by_number_of_workers_for_sync_training = True


class ACERAgentParameters(object):                       # acer_agent.py:90-98
    def __init__(self):
        self.algorithm = ACERAlgorithmParameters()
        self.exploration = CategoricalParameters()       # the reference maps DiscreteActionSpace -> Categorical only
        self.memory = EpisodicExperienceReplayParameters()
        self.network_wrappers = {"main": ACERNetworkParameters()}
        self.seed = 0

    @property
    def path(self):
        return 'coach_amd.agents.acer_agent:ACERAgent'


class ACERAgent(PolicyOptimizationAgent):
    SIGNAL_NAMES = PolicyOptimizationAgent.SIGNAL_NAMES + ["Q Loss", "Policy Loss", "Probability Loss",
                                                           "Bias Correction Loss", "Values", "KL Divergence"]  # :106-112

    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        super().__init__(agent_parameters, environment, device, dist, use_graphs)
        self.returns = torch.zeros(self.L, dtype=torch.float64, device=self.device)
        self.replayed_windows = 0        # replayed windows so far
        self.debug_targets = None        # tests set this to a list: one dict of clones per window, replayed ones included

    @property
    def is_on_policy(self):
        return False                                     # :114-116

    def _make_network(self, obs_shape, wrapper):
        return ACERNet(self.device, obs_shape, self.A, **acer_net_kwargs(wrapper, self.ap.algorithm, self.ap.seed or 0))

    def _make_episode_buffer(self, obs_shape):
        """the staging buffer with the mu column; it hands every finished episode to the replay of complete episodes"""
        self.replay = EpisodeStore(self.ap.memory.max_size, self.device, int(obs_shape[0]), self.A, self.L)
        return SingleEpisodeBuffer(self.device, self.n_env, obs_shape, self.L, action_probabilities=self.A,
                                   replay=self.replay)

    def _store_extra_host(self, dones_host, record):
        return {"action_probabilities": self.action_probabilities}

    # ------------------------------------------------------------------------------- training
    def _learn_from_rows(self, src, r0, T, whole_episode_behind, kind):
        """_learn_from_batch (:118-180) on rows [r0, r0 + T) of `src` (the staging buffer or the replay).  The state
        behind the window is the next row in place, or — behind an episode's last transition — its pre-reset next_obs."""
        alg, net = self.ap.algorithm, self.networks["main"]
        obs = src.obs[r0:r0 + T]
        rows = net.stage_rows(obs, src.next_obs[r0 + T - 1]) if whole_episode_behind else src.obs[r0:r0 + T + 1]
        game_over = src.game_over[r0 + T - 1:r0 + T]
        actions, mu = src.action[r0:r0 + T], src.mu[r0:r0 + T]
        loss = net.train_window(rows, T, True, actions, mu, src.reward[r0:r0 + T], game_over, alg.discount,
                                rate=alg.rate_for_copying_weights_to_target)
        w = net.window
        self.signals = {"Loss": net.loss, "Grads (unclipped)": net.norm, "Values": w["V"], "Q Loss": net.q_loss,
                        "Policy Loss": net.policy_loss, "Probability Loss": net.probability_loss,
                        "Bias Correction Loss": net.bias_correction_loss, "KL Divergence": net.kl_divergence}
        if self.debug_targets is not None:
            self.debug_targets.append(dict(
                kind=kind, T=T, q=net.q_online.clone(), logits=net.logits.clone(), mu=mu.clone(), actions=actions.clone(),
                rewards=src.reward[r0:r0 + T].clone(), game_over=game_over.clone(), adam_steps=net.adam_steps,
                **{k: v.clone() for k, v in w.items()}))
        return loss

    def _window_device(self, env, start, end, complete):
        """learn_from_batch (:182-197) for the window [start, end) of env's episode"""
        alg = self.ap.algorithm
        loss = self._learn_from_rows(self.memory, env * self.L + start, end - start, complete, "on-policy")
        if complete:                                     # handle_episode_ended: a sample per transition (agent.py:569-570)
            rewards = self.memory.reward[env * self.L:env * self.L + end]
            self.lib.episode_nstep_returns(rewards, None, self.returns, 0, end, 0, 1, end, float(alg.discount), -1,
                                           _rlx.current_stream())
            self.signals["Discounted Return"] = self.returns[:end]
        if alg.ratio_of_replay > 0 and self.replay.num_transitions() > alg.num_transitions_to_start_replay:
            n = np.random.poisson(alg.ratio_of_replay)
            for _ in range(n):
                if self.signal_stats is not None:        # every _learn_from_batch adds its own samples
                    self._accumulate_signals()
                off, T, whole = self.replay.sample(alg.num_steps_between_gradient_updates, True)
                self._learn_from_rows(self.replay, off, T, whole, "replay")
                self.replayed_windows += 1
        return loss

    def check_status(self):
        super().check_status()
        self.networks["main"].check_status()
