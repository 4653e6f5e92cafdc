"""Epsilon-greedy for N lockstep envs — mirror of rl_coach/exploration_policies/e_greedy.py
(EGreedyParameters :28-46, EGreedy.get_action :84-101, step_epsilon :112-117).

Every env keeps its own ``current_random_value`` exactly like one reference policy instance; the
host makes each env's draws from the global legacy np.random stream in env order
(explore: ``action_space.sample()`` = np.random.choice(n); greedy: np.random.random(n) for the
tie-break; then np.random.rand() for the next step) and stages them; the agent's acting kernel applies them to its
action values (rlx_egreedy for DQN).
"""
import numpy as np
import torch

from ..core_types import RunPhase
from ..schedules import LinearSchedule


class EGreedyParameters(object):                         # e_greedy.py:28-46
    def __init__(self):
        self.epsilon_schedule = LinearSchedule(0.5, 0.01, 50000)
        self.evaluation_epsilon = 0.05

    @property
    def path(self):
        return 'coach_amd.exploration_policies.e_greedy:EGreedy'


class EGreedy(object):
    def __init__(self, num_actions, n_env, device, params):
        self.A, self.n_env, self.device = num_actions, n_env, device
        self.epsilon_schedule = params.epsilon_schedule
        self.evaluation_epsilon = params.evaluation_epsilon
        self.phase = RunPhase.HEATUP
        self.current_random_value = np.array([np.random.rand() for _ in range(n_env)])   # :82
        from ..staging import Stager
        self._st = dict(u=Stager((n_env,), torch.float64, device), ra=Stager((n_env,), torch.int32, device),
                        tie=Stager((n_env, num_actions), torch.float64, device))

    def epsilon(self):
        return self.evaluation_epsilon if self.phase == RunPhase.TEST else self.epsilon_schedule.current_value

    def draw(self):
        """Host draws of one vector step, env by env, in the reference's per-call order: n_env sequential
        get_action calls, each seeing the epsilon the previous call's step_epsilon left behind.
        -> (epsilon of every call [n_env], its current_random_value [n_env], random actions, tie-break randoms)."""
        u = self.current_random_value.copy()
        eps = np.empty(self.n_env)
        ra = np.zeros(self.n_env, dtype=np.int32)
        tie = np.zeros((self.n_env, self.A))
        nxt = np.empty(self.n_env)
        for e in range(self.n_env):
            eps[e] = self.epsilon()                               # this call's epsilon
            if u[e] < eps[e]:                                     # :88
                ra[e] = np.random.choice(self.A)                  # action_space.sample() (:89)
            else:
                tie[e] = np.random.random(self.A)                 # :93
            if self.phase == RunPhase.TRAIN:
                self.epsilon_schedule.step()                      # step_epsilon (:112-117)
            nxt[e] = np.random.rand()
        self.current_random_value = nxt
        return eps, u, ra, tie

    def stage(self, draws):
        """ship one step's host draws -> (epsilon, {u, ra, tie} static device buffers).  The explore / exploit decision
        of every env (its own epsilon) is made here and shipped as data: uniform -1 (explore) or 2 (greedy) against a
        device-side epsilon of 0."""
        eps, u, ra, tie = draws
        st = self._st
        coded = np.where(u < eps, -1.0, 2.0)
        return 0.0, dict(u=st["u"].push(coded), ra=st["ra"].push(ra), tie=st["tie"].push(tie))
