"""A replay of COMPLETE episodes for consecutive-transition sampling — what ACER asks of the reference's
`EpisodicExperienceReplay` (rl_coach/memories/episodic/episodic_experience_replay.py: `store_episode` :294-317,
`_enforce_max_length` :210-222, `sample(size, is_consecutive_transitions=True)` :112-119, `num_transitions` :93-94).

When an env's episode completes, its rows are appended from the staging buffer (single_episode_buffer.py) into an
episode-major store in HBM: obs, the pre-reset next_obs, action, reward, game_over and the behaviour policy's
probabilities `mu`.  A host table holds (offset, length) per episode, oldest first; whole oldest episodes leave while the
store holds more than `max_size` transitions, as `_enforce_max_length` does right after the episode was added.  One store
is shared by all envs: episodes enter in completion order, in env order when several end on the same step.

An episode is always CONTIGUOUS, so a replayed window is a slice read in place and nothing is gathered.  How: the
physical store has max_size + 2 L rows (L = the environment's episode limit).  The live episodes form one circular run
from the oldest episode's offset to the end of the newest.  A new episode goes behind the newest; when it does not fit
before the physical end, it goes to row 0 and the (< L) rows behind the newest stay unused until the run has passed
them.  Before an append the run holds at most max_size rows, so the two free stretches together have at least 2 L rows
less that gap: one of them holds L.  `append_episode` checks the stretch it picked against the oldest episode and raises
rather than overwrite.

`sample` restates the reference's draws one for one on np.random (tests/acer_ref.py: sample_consecutive; pinned to the
reference memory's own recorded choices): an episode index below the number of complete episodes, then — only when the
episode is longer than `size` — `randint(size, length)` as the window's END, which therefore never reaches the episode's
last transition.  `num_transitions()` counts what the reference's counts for an agent that stores whole episodes: the
transitions of the complete episodes held.  Evaluation never writes (the staging buffer does not record then).
"""
from collections import deque

import numpy as np
import torch

from ..memory import Memory, MemoryGranularity


class EpisodeStore(Memory):
    def __init__(self, max_size, device, observation_dim, n_actions, max_episode_length):
        super().__init__(max_size)
        if self.max_size[0] != MemoryGranularity.Transitions:
            raise ValueError("the episode store is bounded in transitions (got {!r})".format(max_size))
        self.device, self.L = device, int(max_episode_length)
        self.capacity = cap = self.max_size[1] + 2 * self.L
        f32 = dict(dtype=torch.float32, device=device)
        self.obs = torch.zeros(cap, int(observation_dim), **f32)
        self.next_obs = torch.zeros(cap, int(observation_dim), **f32)
        self.action = torch.zeros(cap, dtype=torch.int32, device=device)
        self.reward = torch.zeros(cap, **f32)
        self.game_over = torch.zeros(cap, dtype=torch.uint8, device=device)
        self.mu = torch.zeros(cap, int(n_actions), **f32)
        self.episodes = deque()                          # (offset, length), oldest first
        self._num_transitions = 0

    # ---------------------------------------------------------------- Memory interface
    def num_transitions(self):
        return self._num_transitions

    def num_complete_episodes(self):
        return len(self.episodes)

    def length(self):
        return len(self.episodes)

    def clean(self):
        self.episodes.clear()
        self._num_transitions = 0

    # ---------------------------------------------------------------- the host table
    def place(self, n):
        """where an episode of n rows goes -> offset (see the module text); raises rather than overwrite"""
        if not 1 <= n <= self.L:
            raise ValueError("an episode of %d transitions does not fit the episode limit of %d" % (n, self.L))
        if not self.episodes:
            return 0
        head = self.episodes[0][0]
        tail = self.episodes[-1][0] + self.episodes[-1][1]
        if tail > head:                                  # the run does not wrap
            if tail + n <= self.capacity:
                return tail
            ok, off = n <= head, 0
        else:
            ok, off = tail + n <= head, tail
        if not ok:
            raise RuntimeError("the episode store has no contiguous stretch of %d rows (oldest episode at %d, newest "
                               "ends at %d, capacity %d)" % (n, head, tail, self.capacity))
        return off

    def note_episode(self, n):
        """the table's half of store_episode: the new episode's offset, after which whole oldest episodes leave while
        more than max_size transitions are held (:210-222) -> offset"""
        off = self.place(n)
        self.episodes.append((off, int(n)))
        self._num_transitions += int(n)
        size = self.max_size[1]
        while size != 0 and self._num_transitions > size:
            self._num_transitions -= self.episodes.popleft()[1]
        return off

    def append_episode(self, staging, env, n):
        """rows [0, n) of env's running episode in the staging buffer -> the store"""
        off, r0 = self.note_episode(n), env * staging.L
        for name in ("obs", "next_obs", "action", "reward", "game_over", "mu"):
            getattr(self, name)[off:off + n].copy_(getattr(staging, name)[r0:r0 + n])

    # ---------------------------------------------------------------- sampling
    def sample(self, size, is_consecutive_transitions=True):
        """-> (offset of the window's first row, T, whether the window ends at its episode's last transition): rows
        [offset, offset + T) of every column, read in place"""
        if not is_consecutive_transitions:
            raise ValueError("the episode store serves consecutive transitions only")
        if not self.episodes:
            raise ValueError("The episodic replay buffer cannot be sampled since there are no complete episodes yet.")
        off, n = self.episodes[np.random.randint(0, len(self.episodes))]                 # :114
        if n <= size:                                                                    # :115-116
            return off, n, True
        end = np.random.randint(size, n)                                                 # :118
        return off + end - size, int(size), False
