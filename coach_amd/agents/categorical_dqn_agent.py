"""Categorical DQN (C51) on one MI355X — host-side mirror of rl_coach/agents/categorical_dqn_agent.py (parameter classes
:29-71, CategoricalDQNAgent :75-167) and of the CategoricalQHead
(architectures/tensorflow_components/heads/categorical_q_head.py:26-66).

Everything but the head, its loss and the acting reduction is DQN's: torso, replay, epsilon-greedy host draws, target
copies, TF1 Adam, the staged record + one graph per env-step.  The network outputs N logits per action ([B, A * N]); the
softmax over an action's atoms is its return distribution on the support z = np.linspace(v_min, v_max, N), and Q(s, a)
is the fp64 expectation of z under it.
Per step: online logits -> rlx_categorical_egreedy (softmax, fp64 expectations, the epsilon-greedy choice with an fp64
isclose tie test).
Per update: target(s') and online(s) logits -> rlx_c51_head_loss (target action on the target's expectations, the
projection of the shifted support in the reference's order, softmax cross entropy summed over batch AND actions,
dlogits = softmax - labels on the taken action) -> backward -> TF1 Adam.
Prioritized replay: the reference creates the head's importance-weight placeholder but, with an empty loss_type, never
multiplies it in (heads/head.py:141-180), so the weights are read and have no effect; the new priorities are the taken
action's cross entropy (categorical_dqn_agent.py:162-165), which the kernel leaves as fp64 on the device.
"""
import torch

from .. import _rlx
from ..architectures.head_parameters import CategoricalQHeadParameters
from ..core_types import DeviceBatch
from ..exploration_policies.e_greedy import EGreedy, EGreedyParameters
from ..memories.non_episodic.prioritized_experience_replay import PrioritizedExperienceReplay
from ..nn.networks import C51Net
from ..schedules import LinearSchedule
from .dqn_agent import DQNAgent, DQNAgentParameters, DQNAlgorithmParameters, DQNNetworkParameters
from .vector_agent import VectorOffPolicyAgent


class CategoricalDQNNetworkParameters(DQNNetworkParameters):             # categorical_dqn_agent.py:29-32
    def __init__(self):
        super().__init__()
        self.heads_parameters = [CategoricalQHeadParameters()]


class CategoricalDQNAlgorithmParameters(DQNAlgorithmParameters):         # categorical_dqn_agent.py:35-53
    def __init__(self):
        super().__init__()
        self.v_min = -10.0                    # the support's ends and size: z = np.linspace(v_min, v_max, atoms)
        self.v_max = 10.0
        self.atoms = 51


class CategoricalDQNExplorationParameters(EGreedyParameters):            # categorical_dqn_agent.py:56-60
    def __init__(self):
        super().__init__()
        self.epsilon_schedule = LinearSchedule(1, 0.01, 1000000)
        self.evaluation_epsilon = 0.001


class CategoricalDQNAgentParameters(DQNAgentParameters):                 # categorical_dqn_agent.py:63-71
    def __init__(self):
        super().__init__()
        self.algorithm = CategoricalDQNAlgorithmParameters()
        self.exploration = CategoricalDQNExplorationParameters()
        self.network_wrappers = {"main": CategoricalDQNNetworkParameters()}

    @property
    def path(self):
        return 'coach_amd.agents.categorical_dqn_agent:CategoricalDQNAgent'


class CategoricalDQNAgent(DQNAgent):
    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        VectorOffPolicyAgent.__init__(self, agent_parameters, environment, device, dist, use_graphs)
        ep, net, alg = environment.p, self.ap.network_wrappers["main"], self.ap.algorithm
        self.A, self.N = ep.num_actions, int(alg.atoms)
        self.batch_size = net.batch_size
        obs_shape = tuple(ep.observation_shape) + (self.stack,) if self.image else tuple(ep.observation_shape)
        self.networks = {"main": C51Net(
            self.device, obs_shape, self.A, self.N, v_min=alg.v_min, v_max=alg.v_max,
            activation=net.activation_function, embedder=net.embedder_scheme, middleware=net.middleware_scheme,
            learning_rate=net.learning_rate, adam_beta1=net.adam_optimizer_beta1,
            adam_beta2=net.adam_optimizer_beta2, optimizer_epsilon=net.optimizer_epsilon, seed=self.ap.seed or 0,
            head_activation=net.heads_parameters[0].activation_function,
            head_gradient_rescale=net.heads_parameters[0].rescale_gradient_from_head_by_factor,
            clip_gradients=net.clip_gradients)}
        self.z_values = self.networks["main"].z_values                # categorical_dqn_agent.py:78
        self.memory = self._make_memory(action_dim=None)
        self.exploration_policy = EGreedy(self.A, self.n_env, self.device, self.ap.exploration)
        self.actions = torch.zeros(self.n_env, dtype=torch.int32, device=self.device)
        # the taken action's cross entropy per batch row: what update_priorities receives
        self.td_errors = torch.zeros(self.batch_size, dtype=torch.float64, device=self.device)
        self.loss_acc = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._finish_init()

    # --------------------------------------------------------------------------------- acting
    def _q_buf(self):
        """the fp64 expectations of the last acting step [n_env, A] (distribution_prediction_to_q_values, :86-87)."""
        if getattr(self, "_q_act", None) is None or self._q_act.shape != (self.n_env, self.A):
            self._q_act = torch.zeros(self.n_env, self.A, dtype=torch.float64, device=self.device)
        return self._q_act

    def _q_forward(self, states):
        self._logits_act = self.networks["main"].distribution_logits(states, self.n_env, tag="act").data.view(
            self.n_env, self.A * self.N)

    def _categorical_egreedy(self, u, ra, tie, eps):
        self.lib.categorical_egreedy(self._logits_act, self.A * self.N, self.networks["main"].z, self.N, u, ra, tie,
                                     float(eps), self.n_env, self.A, self._q_buf(), self.actions,
                                     _rlx.current_stream())

    def choose_action(self, states):
        self.exploration_policy.phase = self.phase
        draws = self.exploration_policy.draw()                       # host RNG, per env, in order
        self._run(("q", self.n_env), lambda: self._q_forward(states))
        eps, d = self.exploration_policy.stage(draws)
        self._categorical_egreedy(d["u"], d["ra"], d["tie"], eps)
        return self.actions

    # ------------------------------------------------------------------------------- training
    PER_UPDATE_RIDES = False

    def _learn_device(self, b, weights, per_ride=None):
        # weights: the prioritized replay's importance weights, deliberately unused (see the module text)
        self.networks["main"].learn_from_batch(
            b._states["observation"], b._next_states["observation"], self.batch_size, b.actions(), b.rewards(),
            b.game_overs(), self.ap.algorithm.discount, grad_scale=self._grad_scale(),
            sync=self if self.dist is not None else None, states_pair=b._info.get("states_pair"),
            per_errors=self.td_errors)

    def learn_from_batch(self, batch):
        """CategoricalDQNAgent.learn_from_batch (categorical_dqn_agent.py:104-167)."""
        per = isinstance(self.memory, PrioritizedExperienceReplay)
        weights = batch.info("weight") if per else None
        self._run(("learn", per, False), lambda: self._learn_device(batch, weights))
        if per:
            self.memory.update_priorities(batch.info("idx"), self.td_errors)
        loss = self.networks["main"].loss
        self.signals = {"Loss": loss, "Grads (unclipped)": self.networks["main"].norm}
        return loss

    # ------------------------------------------------------------- one staged record + one graph per env-step
    def _step_body(self, k, start, with_act):
        """DQNAgent._step_body with the categorical acting reduction."""
        v = self._step_record(self._rec_k)["views"]
        mem = self.memory
        if with_act:
            self._q_forward(mem.current_states())
            self._categorical_egreedy(v["u"], v["ra"], v["tie"], 0.0)
            self.env.launch_step()
            self._observe_device(v["dst"])
        B = self.batch_size
        b = mem._batch_buffers(B)
        for j in range(start, start + k):
            mem.gather_device(v["rows"][j], B, b)
            batch = DeviceBatch(B, {"observation": b["state"]}, {"observation": b["next_state"]}, b["action"],
                                b["reward"], b["game_over"], info={"states_pair": b["states_pair"]})
            self._learn_device(batch, None)
