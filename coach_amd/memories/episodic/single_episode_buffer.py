"""`SingleEpisodeBuffer` (rl_coach/memories/episodic/single_episode_buffer.py:21-33) for N lockstep envs: the memory
of the on-policy agents that learn from the running episode (Policy Gradients, Actor-Critic, N-step Q, ACER).

In the reference the memory holds ONE finished episode and the agent trains from its `current_episode_buffer`, a list
of Transition objects.  Here both are one staging buffer per env: row (e, t) of `obs` / `action` / `reward` is step t
of env e's running episode, [n_env, L] with L the environment's episode limit.  A step writes one row per env at the
env's own position (the envs' episodes end on different steps), shipped as n_env int32 destination rows; nothing is
sampled and nothing is gathered: an update window is a contiguous slice of an env's rows, which the network reads in
place.  An episode that outgrows L raises (the environment's limit was wrong), before anything is written.

WHEN a transition is visible to train() is the agent's bookkeeping (the response of a non-terminal step is observed at
the start of the next step, level_manager.py:236-264): the rows are written at once, the agent counts them one step
late.  A bootstrapping agent (Actor-Critic) also reads the stored `game_over` byte of a window's last row and the state
behind the window: for a running episode that is row `end` of the env's rows, already written (the state the step whose
response is not yet counted started from), so the window's T + 1 states are `obs[start : end + 1]` in place; for a
finished episode it is `next_obs[end - 1]`, the observation BEFORE the reset (`last_next_state`).
ACER adds two things, both optional: a per-row column `mu` for the behaviour policy's probabilities of the acting step,
and a replay of complete episodes (memories/episodic/episode_store.py) that receives an env's rows when its episode ends.
Evaluation never writes: `begin_evaluation` only redirects the acting state, as the device replays do.
"""
import numpy as np
import torch

from ... import _rlx
from ..memory import Memory, MemoryGranularity, MemoryParameters


class SingleEpisodeBufferParameters(MemoryParameters):                  # single_episode_buffer.py:21-28 (no max_size)
    @property
    def path(self):
        return 'coach_amd.memories.episodic.single_episode_buffer:SingleEpisodeBuffer'


class SingleEpisodeBuffer(Memory):
    def __init__(self, device=None, n_env=1, observation_shape=None, max_episode_length=None,
                 action_probabilities=0, replay=None):
        """action_probabilities: A > 0 adds a per-row column [rows, A] for the behaviour policy's probabilities of the
        acting step (ACER's info['all_action_probabilities']), written by the step's one copy launch; replay: an
        EpisodeStore that receives every finished episode's rows (ACER).  Without them the rows and launches are the
        on-policy agents'."""
        super().__init__((MemoryGranularity.Episodes, 1))                   # single_episode_buffer.py:33
        if device is None or observation_shape is None or not max_episode_length:
            raise ValueError("the device episode buffer needs a device, an observation shape and the episode limit")
        if len(observation_shape) != 1:
            raise ValueError("the single-episode buffer stages vector observations; image observations are not served")
        self.lib = _rlx.lib()
        self.device, self.n_env, self.L = device, int(n_env), int(max_episode_length)
        self.obs_dim = int(observation_shape[0])
        rows = self.rows = self.n_env * self.L
        self.obs = torch.zeros(rows, self.obs_dim, dtype=torch.float32, device=device)
        self.action = torch.zeros(rows, dtype=torch.int32, device=device)
        self.reward = torch.zeros(rows, dtype=torch.float32, device=device)
        self.game_over = torch.zeros(rows, dtype=torch.uint8, device=device)
        self.next_obs = torch.zeros(rows, self.obs_dim, dtype=torch.float32, device=device)     # before the reset
        self.mu = torch.zeros(rows, int(action_probabilities), dtype=torch.float32, device=device) \
            if action_probabilities else None
        self.replay = replay
        self.cur_state = torch.empty(self.n_env, self.obs_dim, dtype=torch.float32, device=device)
        self._eval_state = torch.empty_like(self.cur_state)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.steps = np.zeros(self.n_env, dtype=np.int64)           # rows written of every env's running episode
        self.last_episode_lengths = np.zeros(self.n_env, dtype=np.int64)
        self._evaluating = False
        from ...staging import Stager
        self._dst = Stager((self.n_env,), torch.int32, device, depth=32)

    # ---------------------------------------------------------------- Memory interface
    def num_transitions(self):
        """the reference's memory holds the last finished episode (of every env here)"""
        return int(self.last_episode_lengths.sum())

    def length(self):
        return int((self.last_episode_lengths > 0).sum())

    def clean(self):
        self.steps[:] = 0
        self.last_episode_lengths[:] = 0

    def episode_rows(self, env, start, end):
        """(obs, action, reward) of steps [start, end) of env's running episode: views, no copy"""
        r0 = env * self.L
        return (self.obs[r0 + start:r0 + end], self.action[r0 + start:r0 + end], self.reward[r0:r0 + end])

    def bootstrap_rows(self, env, start, end, complete):
        """what a bootstrapping window [start, end) reads beside episode_rows: (the T + 1 states in place, or None when
        the episode is complete and the state behind the window is `last_next_state`; that state [obs_dim]; the window's
        last game-over byte [1]) — views, no copy"""
        r0 = env * self.L
        in_place = None if complete else self.obs[r0 + start:r0 + end + 1]
        last_next_state = self.next_obs[r0 + end - 1] if complete else self.obs[r0 + end]
        return in_place, last_next_state, self.game_over[r0 + end - 1:r0 + end]

    # ---------------------------------------------------------------- rollout side (the replays' calls)
    def _state(self):
        return self._eval_state if self._evaluating else self.cur_state

    def reset(self, first_obs):
        self._state().copy_(first_obs)

    def current_states(self):
        return self._state()

    def commit_pending(self):
        pass

    def drop_open_episode(self):
        self.steps[:] = 0

    def begin_evaluation(self, first_obs):
        self.drop_open_episode()
        self._evaluating = True
        self.reset(first_obs)

    def end_evaluation(self, first_obs):
        self._evaluating = False
        self.reset(first_obs)

    def store(self, actions, rewards, game_overs, next_obs, reset_obs, record=True, dones=None, defer=False,
              episode_end=False, dones_host=None, action_probabilities=None):
        """one transition per env at its own position, then the envs' next current state (the post-reset observation
        where the episode ended).  record=False (evaluation) only advances the state.  action_probabilities [n_env, A]:
        the acting step's probabilities, one more pair of the copy launch when the buffer has the column."""
        s = _rlx.current_stream()
        stored_game_overs = game_overs
        if dones is not None:
            game_overs = dones
        state = self._state()
        if record:
            if self._evaluating:
                raise RuntimeError("the episode buffer is not written during evaluation")
            if dones_host is None:
                raise ValueError("the episode buffer needs the host's episode-end flags")
            if (self.steps >= self.L).any():
                raise IndexError("an episode outgrew the environment's episode limit of %d steps" % self.L)
            dst = self._dst.push((np.arange(self.n_env) * self.L + self.steps).astype(np.int32))
            pairs = [(actions, self.action), (rewards, self.reward), (state, self.obs),
                     (stored_game_overs, self.game_over), (next_obs, self.next_obs)]
            if self.mu is not None:
                if action_probabilities is None:
                    raise ValueError("the episode buffer has a column for the acting step's action probabilities")
                pairs.append((action_probabilities, self.mu))
            self.lib.copy_columns(_rlx.make_columns(pairs), len(pairs), None, dst, 0, 0, self.n_env, self.rows,
                                  self.n_env, self.status, s)
            self.steps += 1
            ended = np.asarray(dones_host, dtype=bool)
            if self.replay is not None:                  # store_episode (agent.py:576-580), in env order
                for e in np.nonzero(ended)[0].tolist():
                    self.replay.append_episode(self, e, int(self.steps[e]))
            self.last_episode_lengths[ended] = self.steps[ended]
            self.steps[ended] = 0
        self.lib.select_rows(game_overs, reset_obs, next_obs, state, self.n_env, self.obs_dim * 4, s)

    def check_status(self):
        st = int(self.status.item())
        if st:
            self.status.zero_()
            raise IndexError("episode-buffer kernel reported an out-of-range row (status bits %d)" % st)
