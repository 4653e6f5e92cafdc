"""numpy restatement of the BitFlip toy problem (rl_coach/environments/toy_problems/bit_flip.py:54-90) and of the
device environment's reset draws (coach_amd/csrc/bit_flip.hip).

`BitFlip` is the dynamics alone, started from an imposed (state, goal) pair: tests/golden/bit_flip.npz holds what the
reference's own class emitted for recorded action lists, and this class must reproduce it exactly.
`draw_episode` is the Philox twin of the device's reset: key (seed, env), counter (episode, word index, 0, 3), the first
output word of each call, one bit per state / goal bit, low bit first; words [0, nw) are the state, words
[nw (1 + t), nw (2 + t)) the t-th goal draw, redrawn while the goal equals the state; after 32 redraws bit 0 of the goal
is flipped.  `VectorBitFlip` puts both together the way rlx_bitflip_reset / rlx_bitflip_step do for n_env envs."""
import numpy as np

from noise_ref import philox4x32_10

STREAM = 3
MAX_REDRAWS = 32


class BitFlip(object):
    """bit_flip.py:29-90 without gym and without the random reset."""

    def __init__(self, bit_length=16, max_steps=None, mean_zero=False, state=None, goal=None):
        if bit_length < 1:
            raise ValueError('bit_length must be >= 1, found {}'.format(bit_length))
        self.bit_length, self.mean_zero = bit_length, mean_zero
        if max_steps == 0:
            raise ValueError("max_steps = 0 (no limit) is not supported: the memories size their rings by the limit")
        self.max_steps = bit_length if max_steps is None else max_steps
        self.steps = 0
        self.state = np.array(state, dtype=np.int64).copy()
        self.goal = np.array(goal, dtype=np.int64).copy()

    def _emit(self, x):
        return (x - 0.5) / 0.5 if self.mean_zero else x

    def obs(self):
        return {'state': self._emit(self.state), 'desired_goal': self._emit(self.goal),
                'achieved_goal': self._emit(self.state)}

    def step(self, action):
        self.state[action] = int(not self.state[action])
        self.steps += 1
        reward = -1 if (self.state != self.goal).any() else 0
        done = bool((self.state == self.goal).all() or self.steps >= self.max_steps)
        return self.obs(), reward, done


def draw_word(seed, env, episode, w):
    return int(philox4x32_10(episode, w, 0, STREAM, seed, env)[0])


def _bits(seed, env, episode, first_word, L):
    nw = (L + 31) // 32
    words = [draw_word(seed, env, episode, first_word + w) for w in range(nw)]
    return np.array([(words[i // 32] >> (i % 32)) & 1 for i in range(L)], dtype=np.uint8)


def draw_episode(seed, env, episode, L):
    """-> (goal, state, redraws): uint8[L] each; redraws = how many goal draws equalled the state (33: bit 0 flipped)."""
    nw = (L + 31) // 32
    state = _bits(seed, env, episode, 0, L)
    for t in range(MAX_REDRAWS + 1):
        goal = _bits(seed, env, episode, nw * (1 + t), L)
        if not np.array_equal(goal, state):
            return goal, state, t
    goal[0] ^= 1
    return goal, state, MAX_REDRAWS + 1


def find_forced_redraw(L, n_env, seeds=range(64), episodes=range(4)):
    """-> (seed, env, episode) whose first goal draw equals the state (searched on the CPU)."""
    for seed in seeds:
        for env in range(n_env):
            for ep in episodes:
                if draw_episode(seed, env, ep, L)[2] >= 1:
                    return seed, env, ep
    raise LookupError("no forced redraw among the searched seeds")


class VectorBitFlip(object):
    """rlx_bitflip_reset / rlx_bitflip_step for n_env envs: [goal | state] fp32 observations, the terminal observation
    in next_obs and the next episode's first observation in reset_obs (written only where done)."""

    def __init__(self, n_env, L, max_steps=None, mean_zero=False, seed=1234, env_id0=0):
        self.n, self.L, self.mean_zero, self.seed, self.env_id0 = n_env, L, mean_zero, seed, env_id0
        self.max_steps = L if max_steps is None else max_steps
        self.bits = np.zeros((n_env, 2 * L), dtype=np.uint8)
        self.episode = np.zeros(n_env, dtype=np.int32)
        self.steps = np.zeros(n_env, dtype=np.int32)
        self.status = 0
        self.reset_obs = np.zeros((n_env, 2 * L), dtype=np.float32)

    def _emit(self, b):
        b = b.astype(np.float32)
        return (b - np.float32(0.5)) / np.float32(0.5) if self.mean_zero else b

    def _draw(self, e, ep):
        goal, state, _ = draw_episode(self.seed, self.env_id0 + e, ep, self.L)
        self.bits[e] = np.concatenate([goal, state])
        self.episode[e], self.steps[e] = ep, 0

    def reset(self, next_episode=False):
        for e in range(self.n):
            self._draw(e, int(self.episode[e]) + 1 if next_episode else 0)
        return self._emit(self.bits)

    def step(self, actions):
        L = self.L
        reward = np.zeros(self.n, dtype=np.float32)
        done = np.zeros(self.n, dtype=np.uint8)
        next_obs = np.zeros((self.n, 2 * L), dtype=np.float32)
        for e, a in enumerate(np.asarray(actions).tolist()):
            if a < 0 or a >= L:
                self.status |= 2
            else:
                self.bits[e, L + a] ^= 1
            t = int(self.steps[e]) + 1
            equal = np.array_equal(self.bits[e, :L], self.bits[e, L:])
            next_obs[e] = self._emit(self.bits[e])
            reward[e] = 0.0 if equal else -1.0
            done[e] = 1 if (equal or t >= self.max_steps) else 0
            if done[e]:
                self._draw(e, int(self.episode[e]) + 1)
                self.reset_obs[e] = self._emit(self.bits[e])
            else:
                self.steps[e] = t
        return next_obs, self.reset_obs.copy(), reward, done
