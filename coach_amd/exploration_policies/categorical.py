"""Categorical exploration for N lockstep envs — mirror of rl_coach/exploration_policies/categorical.py
(CategoricalParameters :26-29, Categorical.get_action :45-56).

TRAIN: ``np.random.choice(actions, p=probabilities)`` of the legacy generator draws ONE uniform (random_sample) and
takes ``cdf.searchsorted(u, side='right')`` on the fp64 cumulative sum divided by its last entry.  The host draws that
uniform for every env in env order — what n_env sequential get_action calls consume — and the device applies it to the
probabilities it just formed (rlx_softmax_categorical_sample).  Any other phase: np.argmax of the probabilities, the
first maximum (rlx_argmax_rows), and no draw.  Unlike EGreedy, the policy draws nothing when it is constructed.
"""
import numpy as np
import torch

from .. import _rlx
from ..core_types import RunPhase


class CategoricalParameters(object):                     # categorical.py:26-29
    @property
    def path(self):
        return 'coach_amd.exploration_policies.categorical:Categorical'


class Categorical(object):
    def __init__(self, num_actions, n_env, device, params=None):
        self.A, self.n_env, self.device = int(num_actions), int(n_env), device
        self.phase = RunPhase.HEATUP
        self._stager = None

    def draw(self):
        """the host draws of one vector step: one uniform per env in TRAIN (env order), None otherwise"""
        if self.phase != RunPhase.TRAIN:
            return None
        return np.array([np.random.random_sample() for _ in range(self.n_env)], dtype=np.float64)

    def stage(self, uniforms):
        if self._stager is None:
            from ..staging import Stager
            self._stager = Stager((self.n_env,), torch.float64, self.device)
        return self._stager.push(uniforms)

    def select(self, logits, ld, probs_out, actions, uniforms=None):
        """the policy head's logits [n_env][ld] -> probabilities (probs_out [n_env][A]) and actions: the categorical
        draw on staged uniforms (TRAIN) or the first maximum."""
        lib, s = _rlx.lib(), _rlx.current_stream()
        if uniforms is not None:
            lib.softmax_categorical_sample(logits, ld, uniforms, self.n_env, self.A, probs_out, self.A, actions, s)
        else:
            lib.softmax(logits, ld, self.n_env, self.A, probs_out, self.A, s)
            lib.argmax_rows(probs_out, self.A, self.n_env, self.A, actions, s)

    def get_action(self, action_values):
        """Categorical.get_action on the host for ONE probability row -> (action, probabilities): the reference's
        call, draw for draw (a host twin of `select`, used where no device is at hand)."""
        p = np.asarray(action_values)
        if self.phase == RunPhase.TRAIN:
            cdf = p.astype(np.float64).cumsum()
            cdf /= cdf[-1]
            return int(min(cdf.searchsorted(np.random.random_sample(), side='right'), self.A - 1)), action_values
        action = int(np.argmax(p))
        one_hot = np.zeros(self.A)
        one_hot[action] = 1
        return action, one_hot

    def get_control_param(self):
        return 0
