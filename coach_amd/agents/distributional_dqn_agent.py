"""What the distributional DQN agents share (QuantileRegressionDQNAgent, CategoricalDQNAgent; the seam for a further
head such as Rainbow's or IQN's).

Everything but the head, its loss and the acting reduction is DQN's: torso, replay, epsilon-greedy host draws, target
copies, TF1 Adam, the staged record + one graph per env-step (DQNAgent._step_body, with this class's _q_forward and the
subclass's _select_actions).  The network outputs N atoms per action ([B, A * N], nn.networks.DistributionalDQNNet);
what an atom is, and so Q(s, a), the acting kernel and the loss kernel, is the subclass's.

A subclass gives: NET (the network class), _head_kwargs(algorithm parameters) for its constructor, _select_actions (its
acting kernel on self._head_act -> self.actions, fp64 action values into self._q_buf()) and its prioritized-replay
policy: either the loss kernel leaves an error per batch row in self.td_errors, which becomes the row's new priority, or
(PER_REFUSAL, a text) the agent refuses a prioritized memory.
"""
import torch

from ..memories.non_episodic.prioritized_experience_replay import PrioritizedExperienceReplay
from .dqn_agent import DQNAgent
from .vector_agent import VectorOffPolicyAgent


class DistributionalDQNAgent(DQNAgent):
    NET = None
    PER_REFUSAL = None            # None: the loss kernel's per-row errors are the priorities of a prioritized replay

    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        # not DQNAgent.__init__ (it builds a DQNNet), but its order: network, memory, exploration policy, buffers
        VectorOffPolicyAgent.__init__(self, agent_parameters, environment, device, dist, use_graphs)
        ep, net, alg = environment.p, self.ap.network_wrappers["main"], self.ap.algorithm
        self.A, self.N = ep.num_actions, int(alg.atoms)
        self.batch_size = net.batch_size
        obs_shape = tuple(ep.observation_shape) + (self.stack,) if self.image else tuple(ep.observation_shape)
        self.networks = {"main": self.NET(
            self.device, obs_shape, self.A, self.N, **self._head_kwargs(alg),
            activation=net.activation_function, embedder=net.embedder_scheme, middleware=net.middleware_scheme,
            learning_rate=net.learning_rate, adam_beta1=net.adam_optimizer_beta1,
            adam_beta2=net.adam_optimizer_beta2, optimizer_epsilon=net.optimizer_epsilon, seed=self.ap.seed or 0,
            head_activation=net.heads_parameters[0].activation_function,
            head_gradient_rescale=net.heads_parameters[0].rescale_gradient_from_head_by_factor,
            clip_gradients=net.clip_gradients, noisy=self._parameter_noise())}
        self._key_network_noise()
        self.memory = self._make_memory(action_dim=None)
        if self.PER_REFUSAL and isinstance(self.memory, PrioritizedExperienceReplay):
            raise ValueError(self.PER_REFUSAL)
        self.exploration_policy = self._make_exploration_policy()
        self.actions = torch.zeros(self.n_env, dtype=torch.int32, device=self.device)
        # the loss kernel's error per batch row: what update_priorities receives
        self.td_errors = None if self.PER_REFUSAL else \
            torch.zeros(self.batch_size, dtype=torch.float64, device=self.device)
        self.loss_acc = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._finish_init()

    # --------------------------------------------------------------------------------- acting
    def _q_buf(self):
        """the fp64 action values of the last acting step [n_env, A], written by the acting kernel."""
        if getattr(self, "_q_act", None) is None or self._q_act.shape != (self.n_env, self.A):
            self._q_act = torch.zeros(self.n_env, self.A, dtype=torch.float64, device=self.device)
        return self._q_act

    def _q_forward(self, states):
        self._head_act = self.networks["main"].head_output(states, self.n_env, tag="act").data.view(
            self.n_env, self.A * self.N)

    # ------------------------------------------------------------------------------- training
    PER_UPDATE_RIDES = False

    def _learn_device(self, b, weights, per_ride=None):
        # weights: a prioritized replay's importance weights, which neither head's loss uses (see the subclass's text)
        errors = {} if self.td_errors is None else {"per_errors": self.td_errors}
        self.networks["main"].learn_from_batch(
            b._states["observation"], b._next_states["observation"], self.batch_size, b.actions(), b.rewards(),
            b.game_overs(), self.ap.algorithm.discount, grad_scale=self._grad_scale(),
            sync=self if self.dist is not None else None, states_pair=b._info.get("states_pair"), **errors)

    def learn_from_batch(self, batch):
        """the reference agents' learn_from_batch (the subclass's text names the lines)."""
        per = isinstance(self.memory, PrioritizedExperienceReplay)       # (only where td_errors exist: see __init__)
        weights = batch.info("weight") if per else None
        self._run(("learn", per, False), lambda: self._learn_device(batch, weights))
        if per:
            self.memory.update_priorities(batch.info("idx"), self.td_errors)
        loss = self.networks["main"].loss
        self.signals = {"Loss": loss, "Grads (unclipped)": self.networks["main"].norm}
        return loss
