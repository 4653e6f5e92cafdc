"""Normalized Advantage Functions (NAF) on one MI355X — host-side mirror of rl_coach/agents/naf_agent.py (parameter
classes :34-63, NAFAgent.learn_from_batch :80-99, choose_action :101-131) and of the NAFHead
(architectures/tensorflow_components/heads/naf_head.py:27-86).  Gu et al. 2016, https://arxiv.org/abs/1603.00748.

The reference's only value-based continuous-control agent: one network whose head outputs V(s), the greedy action mu(s)
and a packed lower-triangular L(s), with Q(s, u) = V - 1/2 ||L^T (u - mu)||^2, so that argmax_u Q = mu.
Per step: online network -> mu (rlx_naf_head_forward) + Ornstein-Uhlenbeck noise, drawn on the host at the stream
positions where DDPG draws its own.
Per update: the target network's V(s') and the online head on s -> rlx_naf_head_loss (fp64 TD targets, Q, the mean
squared or Huber loss, dV / dmu / dl) -> backward -> clip -> TF1 Adam, captured into one hipGraph; the target network
follows at rate 0.001 after every environment step.
"""
from collections import OrderedDict

import numpy as np
import torch

from ..architectures.head_parameters import NAFHeadParameters
from ..architectures.scheme_views import SchemeViews
from ..core_types import EnvironmentSteps, GradientClippingMethod
from ..exploration_policies.ou_process import OUProcessParameters
from ..memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters
from ..nn.networks import NAFNet
from .vector_agent import AlgorithmParameters, BoxActionAgent, VectorOffPolicyAgent


class NAFNetworkParameters(SchemeViews):                  # naf_agent.py:34-43 + NetworkParameters defaults
    def __init__(self):
        self.activation_function = 'relu'
        self.embedder_scheme = 'Medium'
        self.middleware_scheme = 'Medium'
        self.heads_parameters = [NAFHeadParameters()]
        self.optimizer_type = 'Adam'
        self.batch_size = 32
        self.learning_rate = 0.001
        self.adam_optimizer_beta1 = 0.9
        self.adam_optimizer_beta2 = 0.99
        self.optimizer_epsilon = 0.0001
        self.replace_mse_with_huber_loss = False
        self.async_training = True
        self.create_target_network = True
        self.scale_down_gradients_by_number_of_workers_for_sync_training = True
        self.clip_gradients = None
        self.gradients_clipping_method = GradientClippingMethod.ClipByGlobalNorm


class NAFAlgorithmParameters(AlgorithmParameters):        # naf_agent.py:46-51
    def __init__(self):
        super().__init__()
        self.num_consecutive_training_steps = 5
        self.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(1)
        self.rate_for_copying_weights_to_target = 0.001


class NAFAgentParameters(object):                         # naf_agent.py:54-63
    def __init__(self):
        self.algorithm = NAFAlgorithmParameters()
        self.exploration = OUProcessParameters()
        self.memory = EpisodicExperienceReplayParameters()
        self.network_wrappers = OrderedDict([("main", NAFNetworkParameters())])
        self.seed = 0

    @property
    def path(self):
        return 'coach_amd.agents.naf_agent:NAFAgent'


class NAFAgent(BoxActionAgent):
    # value_optimization_agent.py:36 ("Q"), naf_agent.py:70-74
    SIGNAL_NAMES = VectorOffPolicyAgent.SIGNAL_NAMES + ["Q", "L", "Advantage", "Action", "V", "TD targets"]

    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        if getattr(environment.p, "action_dim", None) is None:
            raise ValueError('NAF works only for continuous control problems')          # naf_agent.py:102-103
        super().__init__(agent_parameters, environment, device, dist, use_graphs)
        if self.image:
            raise ValueError('NAF works only for continuous control problems (vector observations)')
        ep, net = environment.p, self.ap.network_wrappers["main"]
        self.obs_dim = int(ep.observation_shape[0])
        self._set_action_bounds(ep)
        self.batch_size = net.batch_size
        scale = np.maximum(np.abs(self.low), np.abs(self.high))                         # BoxActionSpace.max_abs_range
        method = getattr(net, "gradients_clipping_method", GradientClippingMethod.ClipByGlobalNorm)
        if net.clip_gradients and method == GradientClippingMethod.ClipByNorm:
            raise NotImplementedError("GradientClippingMethod.ClipByNorm has no device implementation")
        self.networks = OrderedDict([("main", NAFNet(
            self.device, (self.obs_dim,), self.A, scale, activation=net.activation_function,
            embedder=net.embedder_scheme, middleware=net.middleware_scheme, learning_rate=net.learning_rate,
            adam_beta1=net.adam_optimizer_beta1, adam_beta2=net.adam_optimizer_beta2,
            optimizer_epsilon=net.optimizer_epsilon, replace_mse_with_huber_loss=net.replace_mse_with_huber_loss,
            head_activation=net.heads_parameters[0].activation_function, clip_gradients=net.clip_gradients,
            clip_by_value=method == GradientClippingMethod.ClipByValue, seed=self.ap.seed or 0))])
        self.memory = self._make_memory(action_dim=self.A)
        self.exploration_policy = self._make_exploration()
        dev, B = self.device, self.batch_size
        self.actions = torch.zeros(self.n_env, self.A, dtype=torch.float32, device=dev)
        self.mu = torch.zeros(self.n_env, self.A, dtype=torch.float32, device=dev)
        self.td_targets = torch.zeros(B, dtype=torch.float32, device=dev)
        self._finish_init()

    # --------------------------------------------------------------------------------- acting
    def choose_action(self, states):
        """naf_agent.py:101-131: mu from the online network, the exploration policy's noise on it; with statistics
        enabled the head's values at u = mu (the reference feeds the network's own mu back as the action, :116-119)."""
        self.exploration_policy.phase = self.phase
        stats = self.signal_stats is not None
        self._run(("mu", stats), lambda: self._mu_forward(states, stats))
        self.exploration_policy.get_action(self.mu, self.actions)
        if stats:
            o = self._act_out
            self.signal_stats.accumulate({"Q": o["Q"], "L": o["L"], "Advantage": o["Advantage"], "Action": o["mu"],
                                          "V": o["V"]})
        return self.actions

    def _mu_forward(self, states, with_signals):
        self._act_out = self.networks["main"].head_forward(states, self.n_env, tag="act", mu_out=self.mu,
                                                           with_signals=with_signals)

    # ------------------------------------------------------------------------------- training
    def _learn_device(self, b, mix=None):
        net = self.networks["main"]
        net.learn_from_batch(b._states["observation"], b._next_states["observation"], self.batch_size, b.actions(),
                             b.rewards(), b.game_overs(), float(self.ap.algorithm.discount), self._grad_scale(),
                             sync=self if self.dist is not None else None, td_targets_out=self.td_targets,
                             mix_rate=mix)

    def _update_record_fields(self):
        return []            # no per-update host draws: the record is the sampled rows

    def learn_from_batch(self, batch):
        mix = self._mix_rate
        self._run(("learn", mix), lambda: self._learn_device(batch, mix))
        if mix is not None:
            self._mixed = self._mixed | {"main"}
        net = self.networks["main"]
        self.signals = {"Loss": net.loss[0], "Grads (unclipped)": net.norm, "TD targets": self.td_targets}
        return net.loss[0]
