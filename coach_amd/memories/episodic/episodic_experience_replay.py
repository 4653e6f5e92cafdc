"""Episodic replay in HBM — the ``EpisodicExperienceReplay`` plug point of DDPG / TD3
(rl_coach/memories/episodic/episodic_experience_replay.py:49-130,240-317,412-426 and Episode,
core_types.py:700-820) for N envs per GPU whose episodes may end on DIFFERENT steps.

What the reference does: an agent keeps the running episode in `current_episode_buffer` and hands it to the
memory when it ends (`store_episode`, agent.py:576-584); the memory appends the episode's transitions to one flat
`transitions` list, computes the n-step discounted returns of the episode (`close_last_episode` ->
`Episode.update_transitions_rewards_and_bootstrap_data`), and evicts WHOLE oldest episodes while it holds more
transitions than `max_size` (`_enforce_max_length` :300-317).  `sample` draws
`np.random.randint(num_transitions_in_complete_episodes(), size=B)` into that list (:121).

Here the payload never moves: every vector step writes its n_env rows time-major into a ring
(row = (step mod ring_steps) * n_env + env), exactly like the flat replay.  The episode structure lives in a small
HOST table — the env front end knows which envs finished a step without asking the device — that lists, in
completion order (ties in env order), the ring rows of every complete episode: logical index i of the reference's
`transitions` list -> `order[(head + i) mod len]` -> ring row.  Completing an episode appends its rows to the table
and launches ONE small kernel for its n-step returns (rlx_episode_nstep_returns, the reference's summation order in
fp64); eviction pops whole episodes from the front; an abandoned episode (a reset in the middle) is simply never
listed.  The ring is sized so that no listed row can be overwritten: capacity + 3 * max_episode_length vector steps
(complete rows <= capacity + one episode, open rows <= n_env * max_episode_length).

With n_env = 1 the table is the identity and every draw selects what the reference selects.
"""
import math
import random
from collections import deque

import numpy as np
import torch

from ... import _rlx
from ...core_types import DeviceBatch
from ..memory import MemoryGranularity
from ..non_episodic.experience_replay import ExperienceReplay, ExperienceReplayParameters


class EpisodicExperienceReplayParameters(ExperienceReplayParameters):        # :32-42
    def __init__(self):
        super().__init__()
        self.max_size = (MemoryGranularity.Transitions, 1000000)
        self.n_step = -1
        self.train_to_eval_ratio = 1

    @property
    def path(self):
        return 'coach_amd.memories.episodic.episodic_experience_replay:EpisodicExperienceReplay'


class EpisodicExperienceReplay(ExperienceReplay):
    def __init__(self, max_size, allow_duplicates_in_batch_sampling=True, n_step=-1, discount=0.99,
                 max_episode_length=None, measurements_dim=None, future_measurements=None, train_to_eval_ratio=1,
                 action_probabilities=0, **device_kwargs):
        """
        :param max_size: (MemoryGranularity.Transitions | Episodes, n)               (reference signature)
        :param n_step: steps summed into n_step_discounted_rewards (-1: to the episode end)   (reference signature)
        :param discount: Episode(discount=...) — the agent's discount factor (agent.py:619)
        :param max_episode_length: the env's time limit; bounds the ring (defaults to min_episode_length)
        :param measurements_dim: M — keep an fp64 column [rows][M] of the STATE's measurements (Direct Future Prediction;
                                 store() then takes them per step); absent (None) unless asked for
        :param future_measurements: (steps S, scale factors [M], last_step) — keep an fp32 column [rows][S * M] of every
                                 transition's future-measurement targets as well, written from the episode's own future
                                 when an env's episode is stored (DFPAgent._update_measurements_targets,
                                 rlx_dfp_future_measurements); last_step: HandlingTargetsAfterEpisodeEnd.LastStep, else NAN
        :param train_to_eval_ratio: Batch RL: the share of the frozen dataset that is trained on          (reference signature)
        :param action_probabilities: A > 0 — keep an fp32 column [rows][A] of what the reference stores as a transition's
                                 info['all_action_probabilities'] (off-policy evaluation divides by it; store() then takes
                                 the step's rows); absent (0) unless asked for
        """
        if not isinstance(n_step, int) or (n_step < 1 and n_step != -1):
            raise ValueError("n-step should be an integer with value >= 1, or set to -1 for always setting to "
                             "episode length.")
        if device_kwargs.get("stack") is not None:
            raise ValueError("the episodic replay holds vector observations (DDPG / TD3); image agents use the "
                             "frame-dedup replay")
        self.n_step, self.discount = n_step, float(discount)
        self.Tmax = int(max_episode_length or device_kwargs.get("min_episode_length", 1))
        unit, amount = max_size
        n_env = int(device_kwargs.get("n_env", 1))
        if unit == MemoryGranularity.Episodes:
            self.max_episodes, transitions = int(amount), int(amount) * self.Tmax
        else:
            self.max_episodes, transitions = None, int(amount)
        transitions = -(-transitions // n_env) * n_env            # the parent wants a multiple of n_env
        self._ring_steps = transitions // n_env + 3 * self.Tmax + 2
        super().__init__((MemoryGranularity.Transitions, transitions), allow_duplicates_in_batch_sampling,
                         **device_kwargs)
        self.max_size = (unit, int(amount))
        self.n_step_discounted_rewards = torch.zeros(self.rows, dtype=torch.float64, device=self.device)
        self.measurements = self.future_measurements = None
        if future_measurements is not None and measurements_dim is None:
            raise ValueError("the future-measurements column is computed from the measurements column")
        if measurements_dim is not None:
            self.M = int(measurements_dim)
            self.measurements = torch.zeros(self.rows, self.M, dtype=torch.float64, device=self.device)
        if future_measurements is not None:
            steps, scale, last_step = future_measurements
            if len(scale) != self.M:
                raise ValueError("one scale factor per measurement: got {} for {}".format(len(scale), self.M))
            self.future_steps, self.future_last_step = int(steps), bool(last_step)
            self.future_scale = torch.tensor([float(x) for x in scale], dtype=torch.float64, device=self.device)
            self.future_measurements = torch.zeros(self.rows, self.future_steps * self.M, dtype=torch.float32,
                                                   device=self.device)
        self.action_probabilities = None
        if action_probabilities:
            self.action_probabilities = torch.zeros(self.rows, int(action_probabilities), dtype=torch.float32,
                                                    device=self.device)
        self._order = np.zeros(transitions + 2 * self.Tmax + 1, dtype=np.int64)   # ring of listed rows
        self.train_to_eval_ratio = train_to_eval_ratio            # used in batch-rl (:69-75)
        self.last_training_set_episode_id = None
        self.last_training_set_transition_id = None
        self.evaluation_dataset_as_episodes = None
        self.evaluation_dataset_as_transitions = None
        self.frozen = False
        self.clean()

    def _physical_rows(self, cap, n_env):
        return n_env * self._ring_steps

    # ------------------------------------------------------------------ Memory interface
    def clean(self):                                              # :412-426
        super().clean()
        self._gstep = 0                                           # vector steps written so far
        self._ep_start = np.zeros(self.n_env, dtype=np.int64)     # step at which each env's running episode began
        self._episodes = deque()                                  # lengths of the complete episodes, oldest first
        self._episode_first_step = deque()                        # ... and the vector step each one began at
        self._order_head, self._order_len = 0, 0

    def length(self):
        """episodes in the memory (the reference counts a non-empty open episode too; agents that store whole
        episodes never have one)."""
        return len(self._episodes)

    def num_complete_episodes(self):
        return len(self._episodes)

    def num_transitions(self):
        return self._order_len

    def num_transitions_in_complete_episodes(self):               # :84-88
        return self._order_len

    def open_transitions(self):
        """rows of the running episodes (written, not sampleable): n_env sequential current_episode_buffers."""
        return int((self._gstep - self._ep_start).sum())

    # ------------------------------------------------------------------------------ rollout side
    def store(self, actions, rewards, game_overs, next_obs, reset_obs, record=True, dones=None, defer=False,
              episode_end=False, dones_host=None, measurements=None, action_probabilities=None):
        """measurements: the STATES' measurements of this step's transitions (device fp64 [n_env][M]); required where
        the memory keeps the column.
        action_probabilities: the step's all_action_probabilities (device fp32 [n_env][A]); required where the memory keeps
        the column.
        One vector step (Agent.observe_transition -> current_episode_buffer.insert, agent.py:956-962), then
        `store_episode` for every env whose episode ended (dones_host: host bool[n_env]; None = lockstep envs,
        all ended iff episode_end).  `defer` is irrelevant here: an episode becomes sampleable only when it is
        complete, and its terminal transition is observed at once (level_manager.py:260-264)."""
        s = _rlx.current_stream()
        stored_go = game_overs
        if dones is not None:
            game_overs = dones
        if record:
            self.assert_not_frozen()
            if self._evaluating:
                raise RuntimeError("the replay memory is not written during evaluation")
            # BEFORE the write: the ring slot of this step may still hold the oldest listed episode when steps were
            # written and never listed (open episodes dropped by a forced reset / an evaluation): evict it, like the
            # reference keeps evicting its oldest episodes (:300-317).  A RUNNING episode that old is a sizing error.
            while self._episode_first_step and self._gstep - self._episode_first_step[0] >= self._ring_steps:
                self._evict_first()
            if self._gstep - int(self._ep_start.min()) >= self._ring_steps:
                raise RuntimeError("episodic replay ring overrun: a running episode is %d vector steps old, the ring "
                                   "holds %d (episodes longer than max_episode_length=%d?)"
                                   % (self._gstep - int(self._ep_start.min()), self._ring_steps, self.Tmax))
            row0 = (self._gstep % self._ring_steps) * self.n_env
            pairs = [(actions, self.action), (rewards, self.reward), (stored_go, self.game_over),
                     (self.cur_state, self.obs), (next_obs, self.next_obs)]
            if (measurements is None) != (self.measurements is None):
                raise ValueError("a memory with a measurements column is stored with measurements, one without it "
                                 "without them")
            if measurements is not None:
                pairs.append((measurements, self.measurements))
            if (action_probabilities is None) != (self.action_probabilities is None):
                raise ValueError("a memory with an action-probabilities column is stored with action_probabilities, one "
                                 "without it without them")
            if action_probabilities is not None:
                pairs.append((action_probabilities, self.action_probabilities))
            self.lib.copy_columns(_rlx.make_columns(pairs), len(pairs), None, None, 0, row0, self.n_env,
                                  self.rows, self.n_env, self.status, s)
        self.lib.select_rows(game_overs, reset_obs, next_obs, self.cur_state, self.n_env, self.obs_dim * 4, s)
        if not record:
            return
        self._gstep += 1
        if dones_host is None:
            ended = range(self.n_env) if episode_end else ()
        else:
            ended = np.nonzero(dones_host)[0]
        for e in ended:
            self._store_episode(int(e))

    def _store_episode(self, e):
        """EpisodicExperienceReplay.store_episode + close_last_episode (:264-317) for env e's finished episode."""
        s0, T = int(self._ep_start[e]), int(self._gstep - self._ep_start[e])
        self._ep_start[e] = self._gstep
        if T <= 0:
            return
        if T > self.Tmax:
            raise ValueError("an episode of %d steps exceeds max_episode_length=%d the ring was sized for"
                             % (T, self.Tmax))
        k = np.arange(T, dtype=np.int64)
        rows = ((s0 + k) % self._ring_steps) * self.n_env + e
        pos = (self._order_head + self._order_len + k) % self._order.size
        self._order[pos] = rows
        self._order_len += T
        self._episodes.append(T)
        self._episode_first_step.append(s0)
        self.lib.episode_nstep_returns(self.reward, self.n_step_discounted_rewards, None, s0, T, e, self.n_env,
                                       self._ring_steps, self.discount, self.n_step, _rlx.current_stream())
        if self.future_measurements is not None:
            self.lib.dfp_future_measurements(self.measurements, self.future_measurements, self.future_scale, s0, T, e,
                                             self.n_env, self._ring_steps, self.future_steps, self.M,
                                             int(self.future_last_step), _rlx.current_stream())
        # _enforce_max_length: whole oldest episodes leave (:300-317)
        if self.max_episodes is not None:
            while len(self._episodes) > self.max_episodes:
                self._evict_first()
        else:
            while self.max_size[1] != 0 and self._order_len > self.max_size[1]:
                self._evict_first()

    def _evict_first(self):
        T = self._episodes.popleft()
        self._episode_first_step.popleft()
        self._order_head = (self._order_head + T) % self._order.size
        self._order_len -= T

    def close_last_episode(self):
        """kept for callers that signal lockstep episode ends separately: store() already did the work."""

    def commit_pending(self):
        pass

    def drop_pending(self):
        pass

    def drop_open_episode(self):
        """Agent.reset_internal_state in the middle of an episode replaces current_episode_buffer
        (agent.py:619): the transitions of every running episode never reach the memory."""
        self._ep_start[:] = self._gstep

    # ----------------------------------------------------------------------------- training side
    def sample_indices(self, size):
        if self.num_complete_episodes() < 1:                      # :112,126-128
            raise ValueError("The episodic replay buffer cannot be sampled since there are no complete "
                             "episodes yet. There is currently 1 episodes with {} transitions"
                             .format(self.open_transitions()))
        return np.random.randint(self.num_transitions_in_complete_episodes(), size=size)   # :121

    def physical_rows(self, logical_idx):
        pos = (self._order_head + np.asarray(logical_idx, dtype=np.int64)) % self._order.size
        return self._order[pos].astype(np.int32)

    def _batch_buffers(self, size):
        b = super()._batch_buffers(size)
        if "n_step_discounted_rewards" not in b:
            b["n_step_discounted_rewards"] = torch.empty(size, dtype=torch.float64, device=self.device)
            if self.measurements is not None:
                b["measurements64"] = torch.empty(size, self.M, dtype=torch.float64, device=self.device)
                b["measurements"] = torch.empty(size, self.M, dtype=torch.float32, device=self.device)
            if self.future_measurements is not None:
                b["future_measurements"] = torch.empty(size, self.future_steps * self.M, dtype=torch.float32,
                                                       device=self.device)
            if self.action_probabilities is not None:
                b["action_probabilities"] = torch.empty(size, self.action_probabilities.shape[1], dtype=torch.float32,
                                                        device=self.device)
        return b

    def _extra_gather_columns(self):
        cols = [(self.n_step_discounted_rewards, "n_step_discounted_rewards")]
        if self.measurements is not None:
            cols.append((self.measurements, "measurements64"))
        if self.future_measurements is not None:
            cols.append((self.future_measurements, "future_measurements"))
        if self.action_probabilities is not None:
            cols.append((self.action_probabilities, "action_probabilities"))
        return cols

    def collate(self, drawn, size, rows_dev=None):
        b = self._gather_rows(drawn, size, rows_dev)
        states = {"observation": b["state"]}
        info = {"logical_idx": drawn, "states_pair": b["states_pair"],
                "n_step_discounted_rewards": b["n_step_discounted_rewards"]}
        if self.measurements is not None:
            b["measurements"].copy_(b["measurements64"])          # the network's input is fp32 (a cast, no arithmetic)
            states["measurements"] = b["measurements"]
        if self.future_measurements is not None:
            info["future_measurements"] = b["future_measurements"]
        if self.action_probabilities is not None:
            info["all_action_probabilities"] = b["action_probabilities"]
        return DeviceBatch(size, states, {"observation": b["next_state"]}, b["action"], b["reward"], b["game_over"],
                           info=info)

    def _steps_written_now(self):
        return self._gstep

    def episode_lengths(self):
        return list(self._episodes)

    # ------------------------------------------------------------------ Batch RL: a dataset from a file (:440-495)
    def load_csv(self, csv_dataset, reward_filter=None, n_actions=None, n_step_returns=False):
        """EpisodicExperienceReplay.load_csv: the file's episodes become the memory's contents.  The host parses the file
        into flat tables once (csv_dataset.py), uploads them once, and one launch (rlx_dataset_ingest) writes the
        transitions to physical rows 0 .. N - 1, which the listed-rows table names in order.
        reward_filter: (rescale_factor, (clipping_low, clipping_high) or None) — the agent's reward filters, applied to the
        fp32 reward by the arithmetic of rlx_reward_filter; None is no filter.
        n_actions: A of the action space, for a memory without the action-probabilities column (one with it knows).
        n_step_returns: n_step_discounted_rewards of the loaded rows is NaN unless this is set — no training path of the
        Batch RL agents reads the column.  The off-policy evaluators do (weighted importance sampling reads every episode's
        first row), so an agent that evaluates asks for it: one rlx_episode_nstep_returns launch per episode then fills the
        column as the reference's store_episode does for an episode built by load_csv — Episode()'s own defaults, discount
        0.99 and n_step -1, not the agent's — from the stored fp32 rewards.
        Departures from the reference: the memory is left FROZEN (the reference freezes a few lines later, in improve());
        a memory that already holds transitions refuses; a bad cell is a ValueError."""
        self.assert_not_frozen()                                  # :447
        from .csv_dataset import read_csv_dataset
        if self.num_transitions() or self.open_transitions():
            raise ValueError("load_csv fills an empty memory: this one holds {} transitions"
                             .format(self.num_transitions() + self.open_transitions()))
        if self.n_env != 1 or self.measurements is not None:
            raise ValueError("load_csv serves a one-environment memory of observations, actions, rewards and action "
                             "probabilities")
        keeps = self.action_probabilities is not None
        A = self.action_probabilities.shape[1] if keeps else n_actions
        if A is None:
            raise ValueError("load_csv into a memory without the action-probabilities column needs n_actions")
        tables = read_csv_dataset(csv_dataset.filepath, int(A), keeps, observation_dim=self.obs_dim,
                                  max_size=self.max_size)
        N = tables.n_transitions
        if N < 1:
            raise ValueError("{}: no episode of at least 2 rows survives in the memory (max_size {})"
                             .format(csv_dataset.filepath, self.max_size))
        if N > self.rows:
            raise ValueError("{}: {} transitions do not fit the memory's {} rows".format(csv_dataset.filepath, N, self.rows))
        rescale, clip = (1.0, None) if reward_filter is None else reward_filter
        lo, hi = clip if clip is not None else (0.0, 0.0)
        dev = self.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        features, action, reward = up(tables.features), up(tables.action), up(tables.reward)
        probs = up(tables.probabilities) if tables.probabilities is not None else None
        src, src_next, last = up(tables.src), up(tables.src_next), up(tables.last)
        self.status.zero_()
        self.lib.dataset_ingest(features, features.shape[1], action, reward, probs,
                                probs.shape[1] if probs is not None else 0, tables.n_file_rows, self.obs_dim,
                                int(A), src, src_next, last, N,
                                int(bool(csv_dataset.is_episodic)), 0, self.rows, float(rescale), int(clip is not None),
                                float(lo), float(hi), self.obs, self.next_obs, self.action, self.reward, self.game_over,
                                self.action_probabilities, self.status, _rlx.current_stream())
        self.n_step_discounted_rewards[:N].fill_(float("nan"))
        bits = int(self.status.item())                            # (the sync also keeps the uploaded tables alive)
        if bits:
            self.status.zero_()
            what = [text for bit, text in ((1, "an action outside the action space"),
                                           (2, "a feature or reward that is not finite"),
                                           (4, "a row index outside the file")) if bits & bit]
            raise ValueError("{}: {} (status bits {})".format(csv_dataset.filepath, ", ".join(what), bits))
        if N > self._order.size:
            self._order = np.zeros(N, dtype=np.int64)
        self._order[:N] = np.arange(N)
        self._order_head, self._order_len = 0, N
        self._episodes = deque(int(T) for T in tables.episode_lengths)
        self._episode_first_step = deque(int(s) for s in np.cumsum([0] + list(tables.episode_lengths[:-1])))
        self._gstep = N
        self._ep_start[:] = N
        if n_step_returns:                                        # Episode() of :468: discount 0.99, n_step -1
            for first, T in zip(self._episode_first_step, self._episodes):
                self.lib.episode_nstep_returns(self.reward, self.n_step_discounted_rewards, None, first, T, 0, 1,
                                               self.rows, 0.99, -1, _rlx.current_stream())
        self.freeze()
        return tables

    def save_csv(self, path):
        """the complete episodes, in logical order, in the schema load_csv reads (csv_dataset.py): an episode of T
        transitions gives T + 1 rows, the last one carrying the final next state (action 0, reward 0, uniform
        probabilities); a memory without the action-probabilities column writes no such column.  The rewards written are the STORED
        ones: they have been through the agent's reward filters already, so a file written here is loaded without one.
        Every float is written with repr(float(x)), so the fp32 values survive the round trip exactly."""
        from .csv_dataset import write_csv_dataset
        n = self.num_transitions_in_complete_episodes()
        cols = {k: [] for k in ("obs", "next_obs", "action", "reward", "probabilities")}
        chunk = 4096
        for i in range(0, n, chunk):
            m = min(chunk, n - i)
            b = self.gather(self.physical_rows(np.arange(i, i + m)), m)
            cols["obs"].append(b["state"].cpu().numpy().copy())
            cols["next_obs"].append(b["next_state"].cpu().numpy().copy())
            cols["action"].append(b["action"].cpu().numpy().copy())
            cols["reward"].append(b["reward"].cpu().numpy().copy())
            if self.action_probabilities is not None:
                cols["probabilities"].append(b["action_probabilities"].cpu().numpy().copy())
        host = {k: (np.concatenate(v) if v else None) for k, v in cols.items()}
        episodes, first = [], 0
        for T in self._episodes:
            episodes.append({k: (None if v is None else v[first:first + T]) for k, v in host.items()})
            first += T
        write_csv_dataset(path, episodes,
                          self.action_probabilities.shape[1] if self.action_probabilities is not None else None)

    # ------------------------------------------------------------------ Batch RL: a frozen dataset (:167-187, :497-546)
    def freeze(self):
        """no new transitions from here on: the memory is a dataset (batch-rl)"""
        self.frozen = True

    def assert_not_frozen(self):
        assert self.frozen is False, "Memory is frozen, and cannot be changed."

    def get_last_training_set_episode_id(self):
        return self.last_training_set_episode_id

    def _split_training_and_evaluation_datasets(self):
        """:532-546.  The transition at round(ratio * transitions) names the last training episode; the training set is
        every whole episode up to and including it."""
        if self.last_training_set_transition_id is None:
            if self.train_to_eval_ratio < 0 or self.train_to_eval_ratio >= 1:
                raise ValueError('train_to_eval_ratio should be in the (0, 1] range.')
            index = round(self.train_to_eval_ratio * self.num_transitions_in_complete_episodes())
            if index >= self.num_transitions_in_complete_episodes():      # self.transitions[index] of the reference
                raise IndexError('train_to_eval_ratio {} of {} transitions selects transition {}, past the last one'
                                 .format(self.train_to_eval_ratio, self.num_transitions_in_complete_episodes(), index))
            seen = 0
            for episode_num, T in enumerate(self._episodes):
                seen += T
                if index < seen:
                    break
            self.last_training_set_episode_id = episode_num
            self.last_training_set_transition_id = seen

    def prepare_evaluation_dataset(self):
        """:512-530, with the evaluation set held as ranges of logical rows, not as copies: one (first, end) per episode
        in evaluation_dataset_as_episodes, the whole span in evaluation_dataset_as_transitions."""
        self._split_training_and_evaluation_datasets()
        first, episodes = self.last_training_set_transition_id, []
        for T in list(self._episodes)[self.get_last_training_set_episode_id() + 1:]:
            episodes.append((first, first + T))
            first += T
        self.evaluation_dataset_as_episodes = episodes
        if len(self.evaluation_dataset_as_episodes) == 0:
            raise ValueError('train_to_eval_ratio is too high causing the evaluation set to be empty. '
                             'Consider decreasing its value.')
        self.evaluation_dataset_as_transitions = (self.last_training_set_transition_id, first)

    def shuffled_training_index_batches(self, size):
        """the host half of get_shuffled_training_data_generator (:179-184): one random.shuffle of the training set's
        logical indices, cut into ceil(n / size) batches, the last one smaller"""
        shuffled_transition_indices = list(range(self.last_training_set_transition_id))
        random.shuffle(shuffled_transition_indices)
        return [shuffled_transition_indices[i * size: (i + 1) * size]
                for i in range(math.ceil(len(shuffled_transition_indices) / size))]

    def get_shuffled_training_data_generator(self, size):
        """:167-187 -> one DeviceBatch per batch of the shuffled training set (gathered through the listed-rows table by
        the memory's gather launch; a batch size has its own buffers, so the last, smaller batch has too).  A batch is
        valid until the next one of its size is drawn."""
        for part in self.shuffled_training_index_batches(size):
            yield self.collate(np.asarray(part, dtype=np.int64), len(part))
