"""Behavioral Cloning on one MI355X — host-side mirror of rl_coach/agents/bc_agent.py (parameter classes :32-58,
BCAgent :62-84) over the imitation base (imitation_agent.py).

The network is the Policy Gradients one (nn.networks.PolicyGradientNet): BCNetworkParameters carries a discrete
PolicyHead.  learn_from_batch hands it the batch's actions and targets of ONES (:77): the head's loss
-mean(log pi(a) * 1) is then the mean negative log-likelihood of the logged actions, and BCAlgorithmParameters has no
beta_entropy, so the entropy term is off.  On the device that is rlx_pg_head_loss with a column of ones as the
advantages followed by one Adam step (PolicyGradientNet.learn_from_batch), one captured graph per batch size.
rlx_pg_head_loss walks its rows in strides, so it has no row limit of its own; the batch size is the wrapper's.

Acting: the softmax of the policy values (the head's output, through rlx_classification_head_loss's probs_out — the
project's one softmax) and rlx_egreedy over those probabilities, in the forced TEST phase (imitation_agent.py).

Memory: the default ExperienceReplay, or an EpisodicExperienceReplay that starts as a CsvDataset
(memory.load_memory_from_file_path).  num_consecutive_playing_steps = EnvironmentSteps(0) trains from the loaded memory
without stepping the environment (BasicRLGraphManager.train_and_act).
"""
import torch

from ..architectures.head_parameters import PolicyHeadParameters
from ..architectures.scheme_views import SchemeViews
from ..core_types import EnvironmentSteps
from ..exploration_policies.e_greedy import EGreedyParameters
from ..memories.non_episodic.experience_replay import ExperienceReplayParameters
from ..nn.networks import PolicyGradientNet, policy_gradient_net_kwargs
from .imitation_agent import ImitationAgent
from .vector_agent import AlgorithmParameters


class BCAlgorithmParameters(AlgorithmParameters):        # bc_agent.py:32-34
    def __init__(self):
        super().__init__()


class BCNetworkParameters(SchemeViews):                  # bc_agent.py:37-46 + NetworkParameters defaults
    def __init__(self):
        self.activation_function = 'relu'
        self.embedder_scheme = 'Medium'
        self.middleware_scheme = 'Medium'
        self.heads_parameters = [PolicyHeadParameters()]
        self.optimizer_type = 'Adam'
        self.batch_size = 32
        self.replace_mse_with_huber_loss = False
        self.create_target_network = False
        self.learning_rate = 0.00025
        self.adam_optimizer_beta1 = 0.9
        self.adam_optimizer_beta2 = 0.99
        self.optimizer_epsilon = 0.0001
        self.scale_down_gradients_by_number_of_workers_for_sync_training = True
        self.clip_gradients = None


class BCAgentParameters(object):                         # bc_agent.py:49-58
    def __init__(self):
        self.algorithm = BCAlgorithmParameters()
        self.exploration = EGreedyParameters()
        self.memory = ExperienceReplayParameters()
        self.network_wrappers = {"main": BCNetworkParameters()}
        self.seed = 0

    @property
    def path(self):
        return 'coach_amd.agents.bc_agent:BCAgent'


class BCAgent(ImitationAgent):
    def _build_network(self, obs_shape, wrapper):
        heads = list(wrapper.heads_parameters)
        if len(heads) != 1 or not isinstance(heads[0], PolicyHeadParameters):
            raise ValueError("BCAgent's network carries exactly one PolicyHeadParameters head, got %s"
                             % [type(h).__name__ for h in heads])
        net = PolicyGradientNet(self.device, obs_shape, self.A,
                                **policy_gradient_net_kwargs(wrapper, self.ap.algorithm, self.ap.seed or 0))
        assert net.beta_entropy == 0.0                   # BCAlgorithmParameters has no beta_entropy
        self._ones, self._probs = {}, {}
        return net

    def _predict(self, states, n):
        net = self.networks["main"]
        z = net.policy_values(states, n, tag="act")
        if n not in self._probs:
            self._probs[n] = (torch.zeros(n, self.A, dtype=torch.float32, device=self.device),
                              torch.zeros(n, dtype=torch.int32, device=self.device),
                              torch.zeros(2, dtype=torch.float32, device=self.device))
        probs, zero_actions, scalars = self._probs[n]
        # the head's softmax: the loss launch's probs_out (action 0 as the target, gradient scale 0: nothing else is read)
        self.lib.classification_head_loss(z.data, self.A, zero_actions, None, self.A, 0.0, n, self.A, z.ensure_grad(),
                                          self.A, probs, self.A, None, scalars, net.status, net.ctx.stream)
        return probs

    # ------------------------------------------------------------------------------- training
    def _training_phases_due(self):
        """num_consecutive_playing_steps = EnvironmentSteps(0): every train() call is one training phase on what the
        memory holds (the loaded dataset); otherwise the off-policy schedule"""
        playing = self.ap.algorithm.num_consecutive_playing_steps
        if isinstance(playing, EnvironmentSteps) and playing.num_steps == 0:
            return 1 if self.memory.num_transitions() > 0 else 0
        return super()._training_phases_due()

    def _bc_update(self, batch, B):
        ones = self._ones.get(B)
        if ones is None:                                 # targets = np.ones(batch size) (:77)
            ones = self._ones[B] = torch.ones(B, dtype=torch.float32, device=self.device)
        self.networks["main"].learn_from_batch(batch._states["observation"], B, batch.actions(), ones,
                                               grad_scale=self._grad_scale())

    def learn_from_batch(self, batch):
        """BCAgent.learn_from_batch (:70-84); one captured graph per batch size"""
        B = batch.size
        self._run(("bc_learn", B), lambda: self._bc_update(batch, B))
        return self._loss_signals()
