"""Action filters of an OutputFilter — mirror of rl_coach/filters/action/ for the one filter with a device form.

BoxDiscretization (filters/action/box_discretization.py:26-72, on PartialDiscreteActionSpaceMap,
partial_discrete_action_space_map.py:25-58): the agent acts in a DiscreteActionSpace of prod(bins) actions, the
environment receives `target_actions[action]`, a point of its BoxActionSpace.  The table is built once on the host with
the reference's own numpy expression — per dimension np.linspace(low[i], high[i], bins[i]), the actions their Cartesian
product with the last dimension running fastest (itertools.product's order) — as ONE [n][A] array, not a Python list of
n lists, in the dtype numpy gives the expression for the bounds it is handed (the agents hand it the fp32 bounds a gym
box has); it is cast to fp32 where it meets a network or the environment.  On the device the filter is a row gather
(rlx_wolpertinger_select's tail for acting, rlx_discrete_to_box for a batch).
"""
import numpy as np


class BoxDiscretization(object):
    def __init__(self, num_bins_per_dimension, force_int_bins=False):
        """num_bins_per_dimension: one number for every dimension of the box, or one per dimension.
        force_int_bins: truncate the bins to integers (0, 2, 5, 7, 10 instead of 0, 2.5, 5, 7.5, 10)."""
        self.num_bins_per_dimension = num_bins_per_dimension
        self.force_int_bins = force_int_bins
        self.target_actions = None

    def bins_per_dimension(self, action_dim):
        b = self.num_bins_per_dimension
        if isinstance(b, (int, np.integer)):
            return np.ones(action_dim).astype(int) * int(b)               # box_discretization.py:58-59
        if len(b) != action_dim:                                          # validate_output_action_space (:50-55)
            raise ValueError("The length of the list of bins per dimension ({}) does not match the number of "
                             "dimensions in the action space ({})".format(len(b), action_dim))
        return np.asarray(b).astype(int)

    def get_unfiltered_action_space(self, low, high):
        """low, high: the box's bounds per dimension -> the number of discrete actions; sets target_actions [n][A]."""
        low, high = np.atleast_1d(low), np.atleast_1d(high)
        bins = []
        for i, n in enumerate(self.bins_per_dimension(len(low))):
            dim_bins = np.linspace(low[i], high[i], n)                    # :63-64
            if self.force_int_bins:
                dim_bins = dim_bins.astype(int)
            bins.append(dim_bins)
        grid = np.meshgrid(*bins, indexing="ij")                          # product(*bins): the last dimension fastest
        self.target_actions = np.stack([g.reshape(-1) for g in grid], axis=1)
        return len(self.target_actions)

    def filter(self, action):
        """one discrete action -> its point of the box (partial_discrete_action_space_map.py:52-55)"""
        if not 0 <= int(action) < len(self.target_actions):
            raise ValueError("The given action ({}) does not match the action space of {} actions"
                             .format(action, len(self.target_actions)))
        return self.target_actions[int(action)]
