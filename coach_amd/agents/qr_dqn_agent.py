"""Quantile-Regression DQN on one MI355X — host-side mirror of rl_coach/agents/qr_dqn_agent.py (parameter classes
:28-60, QuantileRegressionDQNAgent :63-137) and of the QuantileRegressionQHead loss
(architectures/tensorflow_components/heads/quantile_regression_q_head.py:40-81).

The head over DistributionalDQNAgent (agents/distributional_dqn_agent.py): the network's N atoms per action are
quantiles; Q(s, a) is the fp64 mean of action a's atoms.
Per step: online quantiles -> rlx_quantile_egreedy (fp64 means, the epsilon-greedy choice with an fp64 isclose tie test).
Per update: target(s') and online(s) quantiles -> rlx_qr_dqn_head_loss (target action on the target's means, fp64 TD
targets, the reference's argsort-indexed midpoints, the quantile Huber loss summed over the batch, dtheta) -> backward
-> TF1 Adam.  The reference never updates replay priorities for this agent: a prioritized memory is refused.
"""
from .. import _rlx
from ..architectures.head_parameters import QuantileRegressionQHeadParameters
from ..nn.networks import QRDQNNet
from ..schedules import LinearSchedule
from .distributional_dqn_agent import DistributionalDQNAgent
from .dqn_agent import DQNAgentParameters, DQNAlgorithmParameters, DQNNetworkParameters


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


class QuantileRegressionDQNAgent(DistributionalDQNAgent):
    NET = QRDQNNet
    PER_REFUSAL = ("QuantileRegressionDQNAgent does not use replay priorities (the reference agent never "
                   "updates them and ignores importance weights): use an ExperienceReplay memory")

    @staticmethod
    def _head_kwargs(alg):
        return dict(huber_loss_interval=alg.huber_loss_interval)

    def _select_actions(self, u, ra, tie, eps):
        """get_q_values (qr_dqn_agent.py:75-76) + the epsilon-greedy choice on the fp64 atom means."""
        self.lib.quantile_egreedy(self._head_act, self.A * self.N, self.N, u, ra, tie, float(eps), self.n_env, self.A,
                                  self._q_buf(), self.actions, _rlx.current_stream())

    def _argmax_actions(self):
        """ParameterNoise: np.argmax of the same fp64 atom means (the first maximum, no draws)."""
        self.lib.quantile_argmax(self._head_act, self.A * self.N, self.N, self.n_env, self.A, self._q_buf(),
                                 self.actions, _rlx.current_stream())
