"""Quantile-Regression DQN on one MI355X — host-side mirror of rl_coach/agents/qr_dqn_agent.py (parameter classes
:28-60, QuantileRegressionDQNAgent :63-137) and of the QuantileRegressionQHead loss
(architectures/tensorflow_components/heads/quantile_regression_q_head.py:40-81).

Everything but the head, its loss and the acting reduction is DQN's: torso, replay, epsilon-greedy host draws, target
copies, TF1 Adam, the staged record + one graph per env-step.  The network outputs N atoms per action ([B, A * N]);
Q(s, a) is the fp64 mean of action a's atoms.
Per step: online quantiles -> rlx_quantile_egreedy (fp64 means, the epsilon-greedy choice with an fp64 isclose tie test).
Per update: target(s') and online(s) quantiles -> rlx_qr_dqn_head_loss (target action on the target's means, fp64 TD
targets, the reference's argsort-indexed midpoints, the quantile Huber loss summed over the batch, dtheta) -> backward
-> TF1 Adam.  The reference never updates replay priorities for this agent: a prioritized memory is refused.
"""
import torch

from .. import _rlx
from ..architectures.head_parameters import QuantileRegressionQHeadParameters
from ..core_types import DeviceBatch
from ..memories.non_episodic.prioritized_experience_replay import PrioritizedExperienceReplay
from ..nn.networks import QRDQNNet
from ..exploration_policies.e_greedy import EGreedy
from ..schedules import LinearSchedule
from .dqn_agent import DQNAgent, DQNAgentParameters, DQNAlgorithmParameters, DQNNetworkParameters
from .vector_agent import VectorOffPolicyAgent


class QuantileRegressionDQNNetworkParameters(DQNNetworkParameters):      # qr_dqn_agent.py:28-33
    def __init__(self):
        super().__init__()
        self.heads_parameters = [QuantileRegressionQHeadParameters()]
        self.learning_rate = 0.00005
        self.optimizer_epsilon = 0.01 / 32


class QuantileRegressionDQNAlgorithmParameters(DQNAlgorithmParameters):  # qr_dqn_agent.py:36-49
    def __init__(self):
        super().__init__()
        self.atoms = 200                      # atoms (quantiles) per action
        self.huber_loss_interval = 1          # kappa: the quantile Huber loss is quadratic on [-kappa, kappa]


class QuantileRegressionDQNAgentParameters(DQNAgentParameters):          # qr_dqn_agent.py:52-60
    def __init__(self):
        super().__init__()
        self.algorithm = QuantileRegressionDQNAlgorithmParameters()
        self.network_wrappers = {"main": QuantileRegressionDQNNetworkParameters()}
        self.exploration.epsilon_schedule = LinearSchedule(1, 0.01, 1000000)
        self.exploration.evaluation_epsilon = 0.001

    @property
    def path(self):
        return 'coach_amd.agents.qr_dqn_agent:QuantileRegressionDQNAgent'


class QuantileRegressionDQNAgent(DQNAgent):
    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        VectorOffPolicyAgent.__init__(self, agent_parameters, environment, device, dist, use_graphs)
        ep, net, alg = environment.p, self.ap.network_wrappers["main"], self.ap.algorithm
        self.A, self.N = ep.num_actions, int(alg.atoms)
        self.batch_size = net.batch_size
        obs_shape = tuple(ep.observation_shape) + (self.stack,) if self.image else tuple(ep.observation_shape)
        self.networks = {"main": QRDQNNet(
            self.device, obs_shape, self.A, self.N, huber_loss_interval=alg.huber_loss_interval,
            activation=net.activation_function, embedder=net.embedder_scheme, middleware=net.middleware_scheme,
            learning_rate=net.learning_rate, adam_beta1=net.adam_optimizer_beta1,
            adam_beta2=net.adam_optimizer_beta2, optimizer_epsilon=net.optimizer_epsilon, seed=self.ap.seed or 0,
            head_activation=net.heads_parameters[0].activation_function,
            head_gradient_rescale=net.heads_parameters[0].rescale_gradient_from_head_by_factor,
            clip_gradients=net.clip_gradients)}
        self.memory = self._make_memory(action_dim=None)
        if isinstance(self.memory, PrioritizedExperienceReplay):
            raise ValueError("QuantileRegressionDQNAgent does not use replay priorities (the reference agent never "
                             "updates them and ignores importance weights): use an ExperienceReplay memory")
        self.exploration_policy = EGreedy(self.A, self.n_env, self.device, self.ap.exploration)
        self.actions = torch.zeros(self.n_env, dtype=torch.int32, device=self.device)
        self.td_errors = None
        self.loss_acc = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._finish_init()

    # --------------------------------------------------------------------------------- acting
    def _q_buf(self):
        """the fp64 atom means of the last acting step [n_env, A] (get_q_values, qr_dqn_agent.py:75-76)."""
        if getattr(self, "_q_act", None) is None or self._q_act.shape != (self.n_env, self.A):
            self._q_act = torch.zeros(self.n_env, self.A, dtype=torch.float64, device=self.device)
        return self._q_act

    def _q_forward(self, states):
        self._quant_act = self.networks["main"].quantiles(states, self.n_env, tag="act").data.view(
            self.n_env, self.A * self.N)

    def _quantile_egreedy(self, u, ra, tie, eps):
        self.lib.quantile_egreedy(self._quant_act, self.A * self.N, self.N, u, ra, tie, float(eps), self.n_env, self.A,
                                  self._q_buf(), self.actions, _rlx.current_stream())

    def choose_action(self, states):
        self.exploration_policy.phase = self.phase
        draws = self.exploration_policy.draw()                       # host RNG, per env, in order
        self._run(("q", self.n_env), lambda: self._q_forward(states))
        eps, d = self.exploration_policy.stage(draws)
        self._quantile_egreedy(d["u"], d["ra"], d["tie"], eps)
        return self.actions

    # ------------------------------------------------------------------------------- training
    PER_UPDATE_RIDES = False

    def _learn_device(self, b, weights, per_ride=None):
        self.networks["main"].learn_from_batch(
            b._states["observation"], b._next_states["observation"], self.batch_size, b.actions(), b.rewards(),
            b.game_overs(), self.ap.algorithm.discount, grad_scale=self._grad_scale(),
            sync=self if self.dist is not None else None, states_pair=b._info.get("states_pair"))

    def learn_from_batch(self, batch):
        """QuantileRegressionDQNAgent.learn_from_batch (qr_dqn_agent.py:99-137): no priorities, no importance weights."""
        self._run(("learn", False, False), lambda: self._learn_device(batch, None))
        loss = self.networks["main"].loss
        self.signals = {"Loss": loss, "Grads (unclipped)": self.networks["main"].norm}
        return loss

    # ------------------------------------------------------------- one staged record + one graph per env-step
    def _step_body(self, k, start, with_act):
        """DQNAgent._step_body with the quantile acting reduction."""
        v = self._step_record(self._rec_k)["views"]
        mem = self.memory
        if with_act:
            self._q_forward(mem.current_states())
            self._quantile_egreedy(v["u"], v["ra"], v["tie"], 0.0)
            self.env.launch_step()
            self._observe_device(v["dst"])
        B = self.batch_size
        b = mem._batch_buffers(B)
        for j in range(start, start + k):
            mem.gather_device(v["rows"][j], B, b)
            batch = DeviceBatch(B, {"observation": b["state"]}, {"observation": b["next_state"]}, b["action"],
                                b["reward"], b["game_over"], info={"states_pair": b["states_pair"]})
            self._learn_device(batch, None)

