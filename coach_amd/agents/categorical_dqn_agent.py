"""Categorical DQN (C51) on one MI355X — host-side mirror of rl_coach/agents/categorical_dqn_agent.py (parameter classes
:29-71, CategoricalDQNAgent :75-167) and of the CategoricalQHead
(architectures/tensorflow_components/heads/categorical_q_head.py:26-66).

The head over DistributionalDQNAgent (agents/distributional_dqn_agent.py): the network's N atoms per action are logits;
the softmax over an action's atoms is its return distribution on the support z = np.linspace(v_min, v_max, N), and
Q(s, a) is the fp64 expectation of z under it.
Per step: online logits -> rlx_categorical_egreedy (softmax, fp64 expectations, the epsilon-greedy choice with an fp64
isclose tie test).
Per update: target(s') and online(s) logits -> rlx_c51_head_loss (target action on the target's expectations, the
projection of the shifted support in the reference's order, softmax cross entropy summed over batch AND actions,
dlogits = softmax - labels on the taken action) -> backward -> TF1 Adam.
Prioritized replay: the reference creates the head's importance-weight placeholder but, with an empty loss_type, never
multiplies it in (heads/head.py:141-180), so the weights are read and have no effect; the new priorities are the taken
action's cross entropy (categorical_dqn_agent.py:162-165), which the kernel leaves as fp64 on the device.
"""
from .. import _rlx
from ..architectures.head_parameters import CategoricalQHeadParameters
from ..exploration_policies.e_greedy import EGreedyParameters
from ..nn.networks import C51Net
from ..schedules import LinearSchedule
from .distributional_dqn_agent import DistributionalDQNAgent
from .dqn_agent import DQNAgentParameters, DQNAlgorithmParameters, DQNNetworkParameters


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


class CategoricalDQNAgent(DistributionalDQNAgent):
    NET = C51Net                  # (its loss kernel's per-row error: the taken action's cross entropy)

    @staticmethod
    def _head_kwargs(alg):
        return dict(v_min=alg.v_min, v_max=alg.v_max)

    @property
    def z_values(self):                                               # categorical_dqn_agent.py:78
        return self.networks["main"].z_values

    def _select_actions(self, u, ra, tie, eps):
        """distribution_prediction_to_q_values (:86-87) + the epsilon-greedy choice on the fp64 expectations."""
        self.lib.categorical_egreedy(self._head_act, self.A * self.N, self.networks["main"].z, self.N, u, ra, tie,
                                     float(eps), self.n_env, self.A, self._q_buf(), self.actions,
                                     _rlx.current_stream())

    def _argmax_actions(self):
        """ParameterNoise: np.argmax of the same fp64 expectations (the first maximum, no draws)."""
        self.lib.categorical_argmax(self._head_act, self.A * self.N, self.networks["main"].z, self.N, self.n_env,
                                    self.A, self._q_buf(), self.actions, _rlx.current_stream())
