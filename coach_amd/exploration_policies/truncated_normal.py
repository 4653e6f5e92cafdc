"""Truncated-normal action noise for N lockstep envs — mirror of rl_coach/exploration_policies/truncated_normal.py
(TruncatedNormalParameters :28-39, TruncatedNormal.get_action :78-112).

The reference builds ``scipy.stats.truncnorm((clip_low - mean) / std, (clip_high - mean) / std, loc=mean, scale=std)`` and
draws one value per action dimension: the normal distribution restricted to [clip_low, clip_high], without the mass
that clipping Gaussian noise piles on the bounds.  Here the draw is an inverse CDF in fp64 on the device
(rlx_truncated_normal_sample, csrc/explore_dist.hip: ndtri(ndtr(a) + u (ndtr(b) - ndtr(a))), through the upper tail
where the window lies right of the mean), one thread per element.  The uniforms u come from the host — np.random's
legacy stream, [n_env, A] in element order; scipy's own draw sequence is NOT reproduced — or, with the agent's
noise_source = "device", from the Philox generator of csrc/noise.hip on a stream of its own, at a draw counter that lives
in device memory and advances with every launch, so a replayed acting graph draws new values.

The standard deviation is the schedule's value (the evaluation noise in TEST), as a fraction of the action range
(per dimension) or absolute, or — outside TEST — the per-sample values a network gave with the means.  The schedule
steps once per env outside TEST, as AdditiveNoise's does.
"""
import numpy as np
import torch

from .. import _rlx
from ..core_types import RunPhase
from ..schedules import LinearSchedule


class TruncatedNormalParameters(object):                 # truncated_normal.py:28-39
    def __init__(self):
        self.noise_schedule = LinearSchedule(0.1, 0.1, 50000)
        self.evaluation_noise = 0.05
        self.clip_low = 0
        self.clip_high = 1
        self.noise_as_percentage_from_action_space = True

    @property
    def path(self):
        return 'coach_amd.exploration_policies.truncated_normal:TruncatedNormal'


class TruncatedNormal(object):
    def __init__(self, action_low, action_high, n_env, device, params, action_space_name="DiscreteActionSpace"):
        if action_low is None or action_high is None:                         # :70-72 (not a BoxActionSpace)
            raise ValueError("Truncated normal exploration works only for continuous controls."
                             "The given action space is of type: {}".format(action_space_name))
        self.low = np.atleast_1d(np.asarray(action_low, dtype=np.float32))
        self.high = np.atleast_1d(np.asarray(action_high, dtype=np.float32))
        if not (np.all(-np.inf < self.high) and np.all(self.high < np.inf)
                and np.all(-np.inf < self.low) and np.all(self.low < np.inf)):    # :74-76
            raise ValueError("Additive noise exploration requires bounded actions")
        self.A, self.n_env, self.device = self.low.size, int(n_env), device
        self.noise_schedule = params.noise_schedule
        self.evaluation_noise = params.evaluation_noise
        self.noise_as_percentage_from_action_space = params.noise_as_percentage_from_action_space
        self.clip_low = np.broadcast_to(np.asarray(params.clip_low, dtype=np.float32), (self.A,)).copy()
        self.clip_high = np.broadcast_to(np.asarray(params.clip_high, dtype=np.float32), (self.A,)).copy()
        self.phase = RunPhase.HEATUP
        self.lib = _rlx.lib()
        self.d_clip_low = torch.from_numpy(self.clip_low).to(device)
        self.d_clip_high = torch.from_numpy(self.clip_high).to(device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        from ..staging import Stager
        self._std = Stager((self.A,), torch.float32, device)
        self._u = Stager((self.n_env, self.A), torch.float64, device)
        self.draw_state = torch.zeros(2, dtype=torch.int64, device=device)    # [draw counter, ticket] of the device draws
        self.device_key = None               # (seed, rank) once the agent's noise_source is "device"

    def current_std(self):
        noise = self.evaluation_noise if self.phase == RunPhase.TEST else self.noise_schedule.current_value
        if self.noise_as_percentage_from_action_space:                        # :86-89
            return (noise * (self.high - self.low)).astype(np.float32)
        return np.full(self.A, noise, dtype=np.float32)

    def get_action(self, action_means, out_actions, action_stds=None):
        """action_means: device fp32 [n_env, A] -> out_actions.  action_stds: device fp32 [n_env, A], the standard
        deviations a network gave with the means (:101-104): outside TEST they replace the schedule's value."""
        C = _rlx.CONSTANTS
        std = self.current_std()
        if self.phase != RunPhase.TEST:
            for _ in range(self.n_env):
                self.noise_schedule.step()                                    # :100-101
        if action_stds is not None and self.phase != RunPhase.TEST:
            d_std, kind = action_stds, C["RLX_TN_STD_PER_ELEMENT"]
        else:
            d_std = self._std.push(std)
            kind = C["RLX_TN_STD_PER_DIM"] if self.noise_as_percentage_from_action_space else C["RLX_TN_STD_SCALAR"]
        if self.device_key is None:
            u, seed, rank = self._u.push(np.random.random_sample((self.n_env, self.A))), 0, 0
        else:
            u, (seed, rank) = None, self.device_key
        self.lib.truncated_normal_sample(action_means, d_std, kind, self.d_clip_low, self.d_clip_high, u,
                                         self.draw_state, seed, rank, self.n_env, self.A, out_actions, None,
                                         self.status, _rlx.current_stream())
        return out_actions

    def check(self):
        """std <= 0 or clip_low >= clip_high, which scipy answers with NaN samples (syncs: not inside a captured graph)"""
        if int(self.status.item()) & _rlx.CONSTANTS["RLX_EXPLORE_STATUS_BAD_WINDOW"]:
            self.status.zero_()
            raise ValueError("TruncatedNormal: a standard deviation <= 0 or clip_low >= clip_high")

    def get_control_param(self):
        return np.ones(self.A) * self.noise_schedule.current_value
