"""Bootstrapped exploration for N lockstep envs — mirror of rl_coach/exploration_policies/bootstrapped.py
(BootstrappedParameters :29-38, Bootstrapped :41-88).

An ensemble of K Q heads; every env follows ONE head per episode (``select_head`` = np.random.randint(K) at the episode's
start) while training, and the heads' majority vote otherwise.  Either way the resulting action values go through
EGreedy.get_action unchanged, so the host draws of a step are EGreedy's (including the tie-break draw, which decides
nothing on the vote's one-hot vector); the reduction itself is the agent's acting kernel (rlx_bootstrapped_egreedy).
"""
import numpy as np
import torch

from ..schedules import LinearSchedule
from .e_greedy import EGreedy, EGreedyParameters


class BootstrappedParameters(EGreedyParameters):         # bootstrapped.py:29-38
    def __init__(self):
        super().__init__()
        self.architecture_num_q_heads = 10
        self.bootstrapped_data_sharing_probability = 1.0
        self.epsilon_schedule = LinearSchedule(1, 0.01, 1000000)

    @property
    def path(self):
        return 'coach_amd.exploration_policies.bootstrapped:Bootstrapped'


class Bootstrapped(EGreedy):
    def __init__(self, num_actions, n_env, device, params):
        super().__init__(num_actions, n_env, device, params)
        self.num_heads = int(params.architecture_num_q_heads)
        self.selected_head = np.zeros(n_env, dtype=np.int32)           # :66, one per env
        from ..staging import Stager
        self._st["head"] = Stager((n_env,), torch.int32, device)

    def select_head(self, envs=None):
        """select_head (:69-70) of every env in `envs` (all of them when None): one np.random.randint(K) each, in env
        order."""
        for e in (range(self.n_env) if envs is None else envs):
            self.selected_head[int(e)] = np.random.randint(self.num_heads)

    def stage_heads(self):
        """the envs' selected heads -> a static device buffer (int32 [n_env])"""
        return self._st["head"].push(self.selected_head)

    def get_control_param(self):
        return self.selected_head
