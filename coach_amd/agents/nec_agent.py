"""Neural Episodic Control on one MI355X — host-side mirror of rl_coach/agents/nec_agent.py (parameter classes :36-110,
NECAgent :114-227).  Pritzel et al. 2017, https://arxiv.org/abs/1703.01988.

Per vector step: states -> the trunk's embedding and the dictionary's Q rows over all A tables (nn.networks.NECNet over
csrc/dnd.hip) -> rlx_egreedy on the staged host draws (DQN's acting) -> env.step -> the episodic replay's row, with the
embedding the agent acted on and max_action_value = max_a Q.  A heat-up step draws its action at random, still stores
its embedding (act :163-171) and carries max_action_value = 0, as in the reference: a sampled action's ActionInfo keeps
the default action_value (core_types.py:385-402).  Nothing is stored in TEST.
Per finished episode of an env, outside TEST: the replay's episode-close launch with the old policy's bootstrap
(rlx_episode_nstep_returns_bootstrapped), then the episode's embeddings, actions and returns go to the dictionary in
episode order (rlx_dnd_add; handle_episode_ended :212-222).
Per update: nothing until every table holds more than number_of_knn entries (learn_from_batch :127-133: a zero loss, no
launch); then NECNet.learn_from_batch on the batch's states, actions and n_step_discounted_rewards.  No target network.
Launch shapes follow the tables' growth, so acting and updates are issued eagerly, not replayed from a captured graph.
Refused by name: image observations, data-parallel training, propagate_updates_to_DND.  Checkpointing the tables is out
of scope."""
import torch

from ..architectures.head_parameters import DNDQHeadParameters
from ..architectures.scheme_views import SchemeViews
from ..core_types import EnvironmentSteps
from ..exploration_policies.e_greedy import EGreedy, EGreedyParameters
from ..memories.episodic.episodic_experience_replay import EpisodicExperienceReplay, EpisodicExperienceReplayParameters
from ..memories.memory import MemoryGranularity
from ..nn.networks import NECNet, nec_net_kwargs
from ..schedules import ConstantSchedule
from .dqn_agent import DQNAgent
from .vector_agent import AlgorithmParameters


class NECNetworkParameters(SchemeViews):                 # nec_agent.py:36-43 + NetworkParameters defaults
    def __init__(self):
        self.activation_function = 'relu'
        self.embedder_scheme = 'Medium'
        self.middleware_scheme = 'Medium'
        self.heads_parameters = [DNDQHeadParameters()]
        self.optimizer_type = 'Adam'
        self.should_get_softmax_probabilities = False
        self.create_target_network = False
        self.batch_size = 32
        self.learning_rate = 0.00025
        self.adam_optimizer_beta1 = 0.9
        self.adam_optimizer_beta2 = 0.99
        self.optimizer_epsilon = 0.0001
        self.clip_gradients = None                       # ClipByGlobalNorm threshold (base_parameters.py)


class NECAlgorithmParameters(AlgorithmParameters):       # nec_agent.py:46-90
    def __init__(self):
        super().__init__()
        self.dnd_size = 500000
        self.l2_norm_added_delta = 0.001
        self.new_value_shift_coefficient = 0.1
        self.number_of_knn = 50
        self.DND_key_error_threshold = 0
        self.num_consecutive_playing_steps = EnvironmentSteps(4)
        self.propagate_updates_to_DND = False
        self.n_step = 100
        self.bootstrap_total_return_from_old_policy = True


class NECMemoryParameters(EpisodicExperienceReplayParameters):               # nec_agent.py:93-96
    def __init__(self):
        super().__init__()
        self.max_size = (MemoryGranularity.Transitions, 100000)


class NECAgentParameters(object):                        # nec_agent.py:99-110
    def __init__(self):
        self.algorithm = NECAlgorithmParameters()
        self.exploration = EGreedyParameters()
        self.memory = NECMemoryParameters()
        self.network_wrappers = {"main": NECNetworkParameters()}
        self.exploration.epsilon_schedule = ConstantSchedule(0.1)
        self.exploration.evaluation_epsilon = 0.01
        self.seed = 0

    @property
    def path(self):
        return 'coach_amd.agents.nec_agent:NECAgent'


class NECAgent(DQNAgent):
    NET = NECNet

    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        if dist is not None and dist.enabled:
            raise NotImplementedError("NECAgent: data-parallel training is not served (one dictionary per worker)")
        super(DQNAgent, self).__init__(agent_parameters, environment, device, dist, use_graphs)
        if self.image:
            raise NotImplementedError("NECAgent: image observations are not served (vector observations only)")
        if not isinstance(self.ap.memory, EpisodicExperienceReplayParameters):
            raise ValueError("NECAgent stores whole episodes: use NECMemoryParameters, not %s"
                             % type(self.ap.memory).__name__)
        ep, net, alg = environment.p, self.ap.network_wrappers["main"], self.ap.algorithm
        if self.L > alg.dnd_size:
            raise ValueError("NECAgent: an episode of up to %d steps does not fit dnd_size = %d" % (self.L, alg.dnd_size))
        self.parameter_noise = False
        self.A, self.batch_size = ep.num_actions, net.batch_size
        self.networks = {"main": NECNet(self.device, tuple(ep.observation_shape), self.A,
                                        **nec_net_kwargs(net, alg, self.ap.seed or 0))}
        self.W = self.networks["main"].W
        self.memory = self._make_memory()
        self.memory.episode_callback = self._episode_to_dictionary
        self.exploration_policy = EGreedy(self.A, self.n_env, self.device, self.ap.exploration)
        self.actions = torch.zeros(self.n_env, dtype=torch.int32, device=self.device)
        self.td_errors = None
        self._embedding = torch.zeros(self.n_env, self.W, dtype=torch.float32, device=self.device)
        self._max_action_value = torch.zeros(self.n_env, dtype=torch.float32, device=self.device)
        self._targets = torch.zeros(self.batch_size, dtype=torch.float32, device=self.device)
        self._zero_loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.training_started = False
        self._finish_init()

    def _make_memory(self, action_dim=None):
        mp, ep, alg = self.ap.memory, self.env.p, self.ap.algorithm
        return EpisodicExperienceReplay(mp.max_size, mp.allow_duplicates_in_batch_sampling, n_step=alg.n_step,
                                        discount=alg.discount, max_episode_length=self.L, embedding=self.W,
                                        max_action_value=bool(alg.bootstrap_total_return_from_old_policy),
                                        device=self.device, n_env=self.n_env, observation_shape=ep.observation_shape,
                                        stack=self.stack, action_dim=None,
                                        min_episode_length=getattr(ep, "min_episode_length", self.L))

    def _step_graph_ok(self):
        return False

    # --------------------------------------------------------------------------------- acting
    def random_actions(self):
        """heat-up: a sampled action, the state's embedding all the same (act :163-171), max_action_value 0"""
        actions = super().random_actions()
        self._embedding.copy_(self.networks["main"].state_embedding(self.memory.current_states(), self.n_env))
        self._max_action_value.zero_()
        return actions

    def choose_action(self, states):
        self.exploration_policy.phase = self.phase
        draws = self.exploration_policy.draw()                       # host RNG, per env, in order
        q, e = self.networks["main"].q_values(states, self.n_env)
        self._q_act = q
        self._embedding.copy_(e)
        torch.amax(q, dim=1, out=self._max_action_value)             # ActionInfo.max_action_value (:122 of the base agent)
        eps, d = self.exploration_policy.stage(draws)
        self._select_actions(d["u"], d["ra"], d["tie"], eps)
        return self.actions

    def _store_extra_host(self, dones_host, record):
        if not record:                                               # TEST: no embedding is kept
            return {}
        extra = {"embedding": self._embedding}
        if self.memory.max_action_value is not None:
            extra["max_action_value"] = self._max_action_value
        return extra

    def _episode_to_dictionary(self, env, rows):
        """handle_episode_ended (:212-222): the finished episode's embeddings, actions and bootstrapped returns, in
        episode order, into the dictionary"""
        mem = self.memory
        r = torch.from_numpy(rows).to(self.device)
        self.networks["main"].dnd.add(mem.embedding.index_select(0, r), mem.action.index_select(0, r).view(-1),
                                      mem.n_step_discounted_rewards.index_select(0, r).to(torch.float32))

    # ------------------------------------------------------------------------------- training
    def learn_from_batch(self, batch):
        net = self.networks["main"]
        if not self.training_started:
            if not net.dnd.has_enough_entries(self.ap.algorithm.number_of_knn):      # :128-129: (0, [], 0)
                self.signals = {"Loss": self._zero_loss, "Grads (unclipped)": self._zero_loss}
                return self._zero_loss
            self.training_started = True
        self._targets.copy_(batch.info("n_step_discounted_rewards"))
        net.learn_from_batch(batch._states["observation"], self.batch_size, batch.actions().view(-1), self._targets,
                             grad_scale=self._grad_scale())
        return self._loss_signals()

    def check_status(self):
        super().check_status()
        self.networks["main"].dnd.check_status()
