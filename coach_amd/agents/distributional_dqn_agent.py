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


class DistributionalDQNAgent(DQNAgent):
    NET = None

    def _check_parameters(self):
        super()._check_parameters()
        self.N = int(self.ap.algorithm.atoms)

    def _network_arguments(self, net):
        return (self.N,), dict(noisy=self.parameter_noise, **self._head_kwargs(self.ap.algorithm))

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
        per = isinstance(self.memory, PrioritizedExperienceReplay)       # (only where td_errors exist: _has_td_errors)
        weights = batch.info("weight") if per else None
        self._run(("learn", per, False), lambda: self._learn_device(batch, weights))
        if per:
            self.memory.update_priorities(batch.info("idx"), self.td_errors)
        return self._loss_signals()
