"""Greedy "exploration" for N lockstep envs — mirror of rl_coach/exploration_policies/greedy.py (GreedyParameters :26-29,
Greedy.get_action :44-51): a discrete space takes np.argmax of the action values (the first maximum; rlx_argmax_rows —
NOT rlx_egreedy at epsilon 0, which breaks ties among isclose maxima at random and consumes draws), a box space
returns the action values unchanged.  No host draw in either case.
"""
from .. import _rlx
from ..core_types import RunPhase


class GreedyParameters(object):                          # greedy.py:26-29
    @property
    def path(self):
        return 'coach_amd.exploration_policies.greedy:Greedy'


class Greedy(object):
    def __init__(self, n_env, device, num_actions=None, params=None):
        """num_actions: the size of a discrete action space; None for a box space"""
        self.A, self.n_env, self.device = num_actions, int(n_env), device
        self.phase = RunPhase.HEATUP

    def act(self, q_values, ld, actions):
        """discrete: q_values fp32 [n_env][ld] -> actions int32 [n_env], the first maximum of every row"""
        _rlx.lib().argmax_rows(q_values, ld, self.n_env, self.A, actions, _rlx.current_stream())

    def get_action(self, action_means, out_actions, action_stds=None):
        """box: the agent's action, as it is"""
        out_actions.copy_(action_means.view_as(out_actions))
        return out_actions

    def get_control_param(self):
        return 0
