"""N Pendulum-v0 / Acrobot-v1 environments resident on one GPU — the ``Environment`` plug point
(rl_coach/environments/environment.py:276-327) for the two classic-control levels the reference steps through gym
(`GymVectorEnvironment(level='Pendulum-v0')`, `GymVectorEnvironment(level='Acrobot-v1')`,
presets/Acrobot_DDQN_BCQ_BatchRL.py:97).

The physics are gym 0.12.5's in fp64 (coach_amd/csrc/classic_control.hip: pendulum.py's Euler step and acrobot.py's
"book" dynamics under one RK4 step, sin / cos through the full-range restatement of glibc's, csrc/libm_sincos_full.hpp;
CPU restatement in tests/test_classic_control.py), so the continuous-control agents have a Box level and Batch RL an
Acrobot they can LEARN on.  Shaped like the device CartPole (cartpole_vector_environment.py): one launch per vector
step, auto-reset with Philox reset draws, one small device->host copy per step for `dones_host`, envs sharded across
ranks by `env_id0 = rank * num_envs`.
"""
import numpy as np
import torch

from .. import _rlx
from ..core_types import RunPhase


class _ClassicControlParameters(object):
    LEVEL, LIMIT = None, None                # gym/envs/__init__.py registration: id, max_episode_steps

    def __init__(self, num_envs=1, level=None, seed=1234, episode_length=None):
        if level not in (None, self.LEVEL):
            raise ValueError("this is {}, not {!r}".format(self.LEVEL, level))
        self.kind, self.num_envs = "vector", num_envs
        self.level, self.seed = self.LEVEL, seed
        self.episode_length = int(episode_length or self.LIMIT)                      # the TimeLimit
        self.min_episode_length = 1          # a forced reset or a swing-up may end an episode early


class PendulumVectorEnvironmentParameters(_ClassicControlParameters):
    LEVEL, LIMIT = "Pendulum-v0", 200

    def __init__(self, num_envs=1, level=None, seed=1234, episode_length=None):
        super().__init__(num_envs, level, seed, episode_length)
        self.observation_shape = (3,)
        self.num_actions, self.action_dim = None, 1
        self.action_low, self.action_high = -2.0, 2.0                # BoxActionSpace bounds: max_torque

    @property
    def path(self):
        return 'coach_amd.environments.classic_control_vector_environment:PendulumVectorEnvironment'


class AcrobotVectorEnvironmentParameters(_ClassicControlParameters):
    LEVEL, LIMIT = "Acrobot-v1", 500

    def __init__(self, num_envs=1, level=None, seed=1234, episode_length=None):
        super().__init__(num_envs, level, seed, episode_length)
        self.observation_shape = (6,)
        self.num_actions, self.action_dim = 3, None

    @property
    def path(self):
        return 'coach_amd.environments.classic_control_vector_environment:AcrobotVectorEnvironment'


class _ClassicControlVectorEnvironment(object):
    NAME, STATE_DIM, BAD_ACTION = None, None, None       # rlx_<NAME>_reset / _step, fp64 words per env, status bit 1

    def __init__(self, params, device, rank=0):
        self.p, self.device = params, device
        self.lib = _rlx.lib()
        self._reset, self._step = getattr(self.lib, self.NAME + "_reset"), getattr(self.lib, self.NAME + "_step")
        self.n = n = params.num_envs
        self.seed, self.env_id0 = params.seed, rank * n
        f32, i32 = torch.float32, torch.int32
        obs = (n,) + tuple(params.observation_shape)
        self.state = torch.zeros((n, self.STATE_DIM), dtype=torch.float64, device=device)     # the simulators' fp64 state
        self.next_state64 = torch.zeros((n, self.STATE_DIM), dtype=torch.float64, device=device)
        self.obs = torch.zeros(obs, dtype=f32, device=device)
        self.next_obs = torch.zeros(obs, dtype=f32, device=device)
        self.reset_obs = torch.zeros(obs, dtype=f32, device=device)
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
        self._reset(self.state, self.obs, self.episode, self.step_in_episode, self.n, self.seed, self.env_id0,
                    int(self._started), _rlx.current_stream())
        self._started = True
        self.dones_host[:] = False
        return self.obs

    def _check_actions(self, actions):
        raise NotImplementedError

    def step(self, actions):
        """-> (next_obs, reset_obs, reward, game_over) like the synthetic environment; `dones_host` says which envs
        finished (the one device->host sync of a step)."""
        self._check_actions(actions)
        self._step(actions, self.state, self.episode, self.step_in_episode, self.next_obs, self.reset_obs,
                   self.next_state64, self.reward, self.game_over, self.n, self.p.episode_length, self.seed,
                   self.env_id0, self.status, _rlx.current_stream())
        self._go.copy_(self.game_over, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        np.not_equal(self._go.numpy(), 0, out=self.dones_host)
        return self.next_obs, self.reset_obs, self.reward, self.game_over

    def check_status(self):
        st = int(self.status.item())
        if st & 1:
            raise RuntimeError("%s: an angle left the range of rlx::libm_sin_full / libm_cos_full (|x| < 2^20)"
                               % self.p.level)
        if st & 2:
            raise RuntimeError("%s: %s" % (self.p.level, self.BAD_ACTION))


class PendulumVectorEnvironment(_ClassicControlVectorEnvironment):
    NAME, STATE_DIM = "pendulum", 2
    BAD_ACTION = "a non-finite action was stepped"

    def _check_actions(self, actions):
        """actions: device float32[n_env][1], clipped to [-2, 2] by the simulator."""
        if actions.dtype != torch.float32 or tuple(actions.shape) != (self.n, 1) or not actions.is_contiguous():
            raise TypeError("Pendulum takes contiguous float32 actions [%d][1], got %s %s"
                            % (self.n, actions.dtype, tuple(actions.shape)))


class AcrobotVectorEnvironment(_ClassicControlVectorEnvironment):
    NAME, STATE_DIM = "acrobot", 4
    BAD_ACTION = "an action outside {0, 1, 2} was stepped"

    def _check_actions(self, actions):
        """actions: device int32[n_env] in {0, 1, 2}."""
        if actions.dtype != torch.int32 or actions.numel() != self.n or not actions.is_contiguous():
            raise TypeError("Acrobot takes contiguous int32 actions [%d], got %s %s"
                            % (self.n, actions.dtype, tuple(actions.shape)))
