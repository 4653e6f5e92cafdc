"""Import harness for running the REFERENCE's own numpy code (from /root/reference) in the build
container, where tensorflow / gym / redis / ... are not installed.

Used only by tests/golden/make_golden.py (fixture generation) and by the optional
`reference`-marked tests that run when /root/reference is present.  It never travels to the GPU
box: nothing in the `-m gpu` tests, smoke() or bench.py imports this module.
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types

REFERENCE_ROOT = os.environ.get("COACH_REFERENCE_ROOT", "/root/reference")
_STUBBED = {"tensorflow", "redis", "pygame", "skimage", "minio", "kubernetes", "annoy", "bokeh",
            "OpenGL", "mxnet", "gym", "horovod", "mujoco_py", "roboschool", "pybullet_envs",
            "vizdoom", "carla", "pysc2", "dm_control", "robosuite"}


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__") and name.endswith("__"):
            raise AttributeError(name)
        full = self.__name__ + "." + name
        mod = sys.modules.get(full)
        if mod is None:
            mod = _Stub(full)
            sys.modules[full] = mod
        return mod

    def __call__(self, *a, **k):
        return None

    def __mro_entries__(self, bases):   # `class X(gym.Wrapper)` -> plain object subclass
        return (object,)


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in _STUBBED:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


def reference_available():
    return os.path.isdir(os.path.join(REFERENCE_ROOT, "rl_coach"))


def install():
    """Make `import rl_coach...` resolve to the reference tree with absent packages stubbed."""
    if not reference_available():
        raise RuntimeError("reference tree not found at %s" % REFERENCE_ROOT)
    sys.dont_write_bytecode = True      # /root/reference is read-only
    if not any(isinstance(f, _Finder) for f in sys.meta_path):
        sys.meta_path.insert(0, _Finder())
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)


# ---- opt-in: enough of gym for the reference's GymEnvironment to construct over a fake Atari emulator ----------------
# Our own restatement of the few gym 0.12.5 classes the reference's front end touches (gym/core.py Wrapper,
# gym/wrappers/time_limit.py, the space classes it type-checks against).  What runs on top of it — GymEnvironment,
# MaxOverFramesAndFrameskipEnvWrapper, Environment.step / reset_internal_state — is the reference's own code, imported.
# gym and ALE themselves stay UNPINNED by this: the stand-ins below are ours, and a real game never runs.

class GymWrapper(object):
    """gym.Wrapper: holds `env`, forwards step / reset / seed and every attribute it does not have itself."""

    def __init__(self, env):
        self.env = env
        self.action_space = env.action_space
        self.observation_space = env.observation_space
        self.spec = getattr(env, "spec", None)

    def __getattr__(self, name):
        if name == "env" or (name.startswith("__") and name.endswith("__")):
            raise AttributeError(name)
        return getattr(self.env, name)

    @property
    def unwrapped(self):
        return self.env.unwrapped

    def step(self, action):
        return self.env.step(action)

    def reset(self, **kwargs):
        return self.env.reset(**kwargs)

    def seed(self, seed=None):
        return self.env.seed(seed)


class GymTimeLimit(GymWrapper):
    """gym.wrappers.TimeLimit: counts the steps since reset() and reports done from `max_episode_steps` on."""

    def __init__(self, env, max_episode_steps):
        super().__init__(env)
        self._max_episode_steps = max_episode_steps
        self._elapsed_steps = None
        self.truncations = 0            # bookkeeping of ours: steps the limit ended although the game went on

    def step(self, action):
        assert self._elapsed_steps is not None, "step() before the first reset()"
        observation, reward, done, info = self.env.step(action)
        self._elapsed_steps += 1
        if self._elapsed_steps >= self._max_episode_steps:
            info['TimeLimit.truncated'] = not done
            self.truncations += int(not done)
            done = True
        return observation, reward, done, info

    def reset(self, **kwargs):
        self._elapsed_steps = 0
        return self.env.reset(**kwargs)


class GymDiscrete(object):
    def __init__(self, n):
        self.n, self.shape = n, ()


class GymBox(object):
    def __init__(self, low, high, shape, dtype):
        import numpy as np
        self.shape, self.dtype = tuple(shape), dtype
        self.low, self.high = np.full(self.shape, low, dtype), np.full(self.shape, high, dtype)


class GymDict(object):
    def __init__(self, spaces):
        self.spaces = dict(spaces)


class _Ale(object):
    def __init__(self, emulator):
        self._emulator = emulator

    def lives(self):
        return self._emulator.lives()


class FakeAtariEnv(object):
    """The bare gym env behind gym.make: an emulator (reset() / step(a) -> (frame, reward, done) / lives() /
    action_meanings()) with gym's 4-tuple and the attributes GymEnvironment reads.  'Atari' in the class name is what
    the reference looks for (gym_environment.py:305)."""

    def __init__(self, emulator):
        import numpy as np
        self.emulator, self.ale = emulator, _Ale(emulator)
        self.action_space = GymDiscrete(len(emulator.action_meanings()))
        self.observation_space = GymBox(0, 255, emulator.shape, np.uint8)
        self.spec, self.frameskip = None, None
        self.steps, self.resets = 0, 0   # bookkeeping of ours, for locating events in a trace

    @property
    def unwrapped(self):
        return self

    def get_action_meanings(self):
        return self.emulator.action_meanings()

    def seed(self, seed=None):
        return [seed]

    def reset(self):
        self.resets += 1
        return self.emulator.reset()

    def step(self, action):
        self.steps += 1
        frame, reward, done = self.emulator.step(action)
        return frame, reward, done, {}


_LEVELS = {}


def register_level(env_id, emulator, max_episode_steps):
    """gym.make(env_id) will return TimeLimit(FakeAtariEnv(emulator)) — once: an emulator is one game."""
    _LEVELS[env_id] = (emulator, max_episode_steps)


def _gym_make(env_id):
    emulator, max_episode_steps = _LEVELS.pop(env_id)
    return GymTimeLimit(FakeAtariEnv(emulator), max_episode_steps)


def install_gym_front_end():
    """install(), then give the stubbed `gym` the real classes above.  Must run before the reference's
    gym_environment module is imported: its wrapper class derives from gym.Wrapper at import time."""
    install()
    if "rl_coach.environments.gym_environment" in sys.modules:
        raise RuntimeError("rl_coach.environments.gym_environment was imported before the gym stand-ins were in place")
    import gym
    import gym.spaces
    import gym.spaces.box
    import gym.spaces.dict
    import gym.spaces.discrete
    import gym.wrappers
    gym.Wrapper = GymWrapper
    gym.make = _gym_make
    gym.wrappers.TimeLimit = GymTimeLimit
    gym.spaces.discrete.Discrete = gym.spaces.Discrete = GymDiscrete
    gym.spaces.box.Box = gym.spaces.Box = GymBox
    gym.spaces.dict.Dict = gym.spaces.Dict = GymDict
