"""UCB exploration over an ensemble of Q heads for N lockstep envs — mirror of rl_coach/exploration_policies/ucb.py
(UCBParameters :29-42, UCB :45-92).

The K heads' predictions of an action are read as an estimate and its uncertainty: while training the action values are
``mean_k Q_k + lamb * std_k Q_k`` (the population standard deviation), in HEATUP and TEST the mean alone — TEST does NOT
take Bootstrapped's majority vote.  The values go through EGreedy.get_action unchanged, so a step's host draws are
EGreedy's; the reduction and the choice are the agent's acting kernel (rlx_ucb_egreedy, csrc/bootstrapped_dqn.hip; the
arithmetic order is written down in tests/ucb_ref.py).

``select_head`` draws nothing (the reference's is ``pass``): unlike Bootstrapped, no np.random.randint is made when an
episode starts, and no head is staged.
"""
import torch

from ..core_types import EnvironmentSteps, RunPhase
from ..schedules import LinearSchedule, PieceWiseSchedule
from .e_greedy import EGreedy, EGreedyParameters


class UCBParameters(EGreedyParameters):                  # ucb.py:29-42
    def __init__(self):
        super().__init__()
        self.architecture_num_q_heads = 10
        self.bootstrapped_data_sharing_probability = 1.0
        self.epsilon_schedule = PieceWiseSchedule([
            (LinearSchedule(1, 0.1, 1000000), EnvironmentSteps(1000000)),
            (LinearSchedule(0.1, 0.01, 4000000), EnvironmentSteps(4000000))
        ])
        self.lamb = 0.1

    @property
    def path(self):
        return 'coach_amd.exploration_policies.ucb:UCB'


class UCB(EGreedy):
    def __init__(self, num_actions, n_env, device, params):
        super().__init__(num_actions, n_env, device, params)
        self.num_heads = int(params.architecture_num_q_heads)
        self.lamb = params.lamb
        # the heads' standard deviation per env and action, as the last TRAIN step's launch left it (:82)
        self.std = torch.zeros(n_env, num_actions, dtype=torch.float32, device=device)

    def select_head(self, envs=None):                    # :73-74
        pass

    @property
    def use_std(self):
        """the uncertainty bonus is added while training only (:81-85)"""
        return self.phase == RunPhase.TRAIN

    def get_control_param(self):
        """np.mean(std) of every env in TRAIN (one device->host copy), 0 otherwise (:88-92)"""
        if self.phase == RunPhase.TRAIN:
            return self.std.cpu().numpy().mean(axis=1)
        return 0
