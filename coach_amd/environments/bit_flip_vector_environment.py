"""N BitFlip environments resident on one GPU — the toy problem of the reference's BitFlip_DQN / BitFlip_DQN_HER presets
(rl_coach/environments/toy_problems/bit_flip.py:29-90, named as
`GymVectorEnvironment(level='rl_coach.environments.toy_problems.bit_flip:BitFlip')`).

Action a flips bit a; the reward is 0 when the state equals the goal and -1 otherwise; an episode ends when they are
equal or after `max_steps` steps (default `bit_length`; the reference's `max_steps = 0`, "no limit", is refused: the
memories size their rings by the limit).  With `mean_zero` the emitted values are (x - 0.5) / 0.5.

The observation is ONE fp32 vector of 2 * bit_length values, [desired_goal | state] — the order in which the reference
concatenates its embedders (sorted names).  `observation_slices` of the parameters is the slice table; nothing else
hard-codes the layout.  Reset draws are Philox words keyed by (seed, env id) and counted by the episode
(coach_amd/csrc/bit_flip.hip; numpy twin tests/bit_flip_ref.py), so N envs restart on different steps without a host
round trip; one small device->host copy per step tells the host which envs finished (`dones_host`)."""
import numpy as np
import torch

from .. import _rlx
from ..core_types import RunPhase

LEVEL = 'rl_coach.environments.toy_problems.bit_flip:BitFlip'


class BitFlipVectorEnvironmentParameters(object):
    def __init__(self, num_envs=1, bit_length=16, max_steps=None, mean_zero=False, seed=1234):
        bit_length = int(bit_length)
        if bit_length < 1:
            raise ValueError('bit_length must be >= 1, found {}'.format(bit_length))
        if max_steps is not None and int(max_steps) <= 0:
            raise ValueError("BitFlip on the device needs a step limit: max_steps = {} (the reference's 0 means no "
                             "limit) is not supported, the memories size their rings by it".format(max_steps))
        self.kind, self.num_envs, self.observation_shape = "vector", num_envs, (2 * bit_length,)
        self.num_actions, self.action_dim = bit_length, None
        self.bit_length, self.mean_zero, self.seed = bit_length, bool(mean_zero), seed
        self.episode_length = bit_length if max_steps is None else int(max_steps)
        self.min_episode_length = 1
        self.observation_slices = {"desired_goal": (0, bit_length), "state": (bit_length, 2 * bit_length)}
        self.level = LEVEL

    @property
    def path(self):
        return 'coach_amd.environments.bit_flip_vector_environment:BitFlipVectorEnvironment'


class BitFlipVectorEnvironment(object):
    def __init__(self, params, device, rank=0):
        self.p, self.device = params, device
        self.lib = _rlx.lib()
        self.n = n = params.num_envs
        self.L = L = params.bit_length
        self.seed, self.env_id0 = params.seed, rank * n
        f32, i32 = torch.float32, torch.int32
        self.bits = torch.zeros((n, 2 * L), dtype=torch.uint8, device=device)        # [goal | state]
        self.obs = torch.zeros((n, 2 * L), dtype=f32, device=device)
        self.next_obs = torch.zeros((n, 2 * L), dtype=f32, device=device)
        self.reset_obs = torch.zeros((n, 2 * L), dtype=f32, device=device)
        self.reward = torch.zeros(n, dtype=f32, device=device)
        self.game_over = torch.zeros(n, dtype=torch.uint8, device=device)
        self.episode = torch.zeros(n, dtype=i32, device=device)
        self.step_in_episode = torch.zeros(n, dtype=i32, device=device)
        self.status = torch.zeros(1, dtype=i32, device=device)
        self._go = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        self.dones_host = np.zeros(n, dtype=bool)
        self.phase = RunPhase.HEATUP
        self.total_steps = 0
        self._started = False

    def reset_internal_state(self, force_environment_reset=True):
        """every env starts a new episode now (the first call starts episode 0)."""
        self.lib.bitflip_reset(self.bits, self.obs, self.episode, self.step_in_episode, self.n, self.L,
                               int(self.p.mean_zero), self.seed, self.env_id0, int(self._started),
                               _rlx.current_stream())
        self._started = True
        self.dones_host[:] = False
        return self.obs

    def step(self, actions):
        """actions: device int32[n_env] in [0, bit_length).  -> (next_obs, reset_obs, reward, game_over); `dones_host`
        says which envs finished (the one device->host sync of a step)."""
        if actions.dtype != torch.int32:
            raise TypeError("BitFlip takes int32 actions, got %s" % actions.dtype)
        self.lib.bitflip_step(actions, self.bits, self.episode, self.step_in_episode, self.next_obs, self.reset_obs,
                              self.reward, self.game_over, self.n, self.L, self.p.episode_length,
                              int(self.p.mean_zero), self.seed, self.env_id0, self.status, _rlx.current_stream())
        self._go.copy_(self.game_over, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        np.not_equal(self._go.numpy(), 0, out=self.dones_host)
        return self.next_obs, self.reset_obs, self.reward, self.game_over

    def check_status(self):
        if int(self.status.item()) & 2:
            raise RuntimeError("BitFlip: an action outside [0, bit_length) was stepped")
