"""Prioritized replay fed whole n-step episodes — what the reference's Agent does around a
``PrioritizedExperienceReplay`` when ``algorithm.store_transitions_only_when_episodes_are_terminated`` is set (Rainbow):

  * observe_transition keeps every transition in ``current_episode_buffer`` (agents/agent.py:945-973);
  * handle_episode_ended (agents/agent.py:558-584) runs ``Episode.update_transitions_rewards_and_bootstrap_data``
    (core_types.py:803-820: every transition's next_state becomes the state n steps ahead, or the episode's last next
    state; info['should_bootstrap_next_state'] says which; n_step_discounted_rewards is filled) and only then stores the
    episode's transitions, in episode order, through ``PrioritizedExperienceReplay.store``.

Here every env stages its running episode in device columns [n_env][max_episode_length].  When an env's episode ends,
ONE launch (rlx_nstep_episode_store, coach_amd/csrc/nstep_store.hip) writes its T rows — next states redirected, the two
new columns filled — at the ring cursor, and the T rows become visible at once through the parent's ``_became_visible``:
T leaves of maximal priority, the doubled ``num_transitions()``.  Envs that finish on the same step are stored in env
order.  Nothing is pending or deferred: a terminal response is observed on its own step (level_manager.py:260-264), and a
non-terminal one only joins the staged episode.  Sampling, importance weights and priority updates are the parent's; the
payload row of a leaf is the one the parent's arithmetic gives (store number modulo the ring's rows).

``drop_pending`` / ``begin_evaluation`` and a reset in the middle of an episode discard the staged rows, as the reference
replaces ``current_episode_buffer``.  Staged open episodes are not part of a checkpoint: one written in the middle of an
episode restores the stored transitions and the envs' current states, and the episode's earlier steps are lost.

Image observations are refused: the n-step next state in the frame-dedup ring is not built.
"""
import numpy as np
import torch

from ... import _rlx
from ...core_types import DeviceBatch
from .prioritized_experience_replay import PrioritizedExperienceReplay


class NStepPrioritizedExperienceReplay(PrioritizedExperienceReplay):
    def __init__(self, max_size, alpha=0.6, beta=None, epsilon=1e-6, allow_duplicates_in_batch_sampling=True,
                 exact_pow="device", n_step=3, discount=0.99, max_episode_length=None, **device_kwargs):
        """n_step, discount: the algorithm's; max_episode_length: rows of an env's staging area (an episode that is
        longer, or longer than the ring, is refused)."""
        if device_kwargs.get("stack") is not None:
            raise ValueError("n-step next states in the frame-dedup ring are not built: the n-step prioritized replay "
                             "takes vector observations only")
        if not isinstance(n_step, int) or n_step < 2:
            raise ValueError("the n-step prioritized replay needs n_step >= 2 (the reference sets no "
                             "should_bootstrap_next_state otherwise), got %r" % (n_step,))
        if not max_episode_length or int(max_episode_length) < 1:
            raise ValueError("the n-step prioritized replay needs the environment's maximal episode length")
        super().__init__(max_size, alpha, beta, epsilon, allow_duplicates_in_batch_sampling, exact_pow, **device_kwargs)
        self.n_step, self.discount, self.L = n_step, float(discount), int(max_episode_length)
        dev, n, L = self.device, self.n_env, self.L
        self.n_step_discounted_rewards = torch.zeros(self.rows, dtype=torch.float64, device=dev)
        self.should_bootstrap_next_state = torch.zeros(self.rows, dtype=torch.uint8, device=dev)
        self.action_words = 1 if self.action_dim is None else int(self.action_dim)
        self._stage = dict(obs=torch.zeros(n * L, self.obs_dim, dtype=torch.float32, device=dev),
                           next_obs=torch.zeros(n * L, self.obs_dim, dtype=torch.float32, device=dev),
                           action=torch.zeros((n * L,) + tuple(self.action.shape[1:]), dtype=self.action.dtype, device=dev),
                           reward=torch.zeros(n * L, dtype=torch.float32, device=dev),
                           game_over=torch.zeros(n * L, dtype=torch.uint8, device=dev))
        self._staged_steps = np.zeros(n, dtype=np.int64)        # rows of every env's open episode
        self._stage_rows = None                                 # Stager of the step's staging rows (n_env > 1)

    def _check_capacity(self, cap):
        if cap <= 0:
            raise ValueError("replay capacity %d must be positive" % cap)

    def _extra_gather_columns(self):
        return super()._extra_gather_columns() + [(self.n_step_discounted_rewards, "n_step_discounted_rewards"),
                                                  (self.should_bootstrap_next_state, "should_bootstrap_next_state")]

    def _batch_buffers(self, size):
        b = super()._batch_buffers(size)
        if "n_step_discounted_rewards" not in b:
            b["n_step_discounted_rewards"] = torch.empty(size, dtype=torch.float64, device=self.device)
            b["should_bootstrap_next_state"] = torch.empty(size, dtype=torch.uint8, device=self.device)
        return b

    # ------------------------------------------------------------------------------ staged episodes
    def clean(self):
        super().clean()
        self._staged_steps[:] = 0

    def drop_pending(self):
        """a reset before the episode ended: the staged rows are never stored."""
        self._staged_steps[:] = 0

    def commit_pending(self):
        """nothing is ever pending: rows become visible when their episode ends."""

    def reset(self, first_obs):
        if not self._evaluating:
            self._staged_steps[:] = 0
        super().reset(first_obs)

    def staged_transitions(self):
        return int(self._staged_steps.sum())

    def episode_discounted_returns(self, env, length, discount, n_step=-1):
        """the 'Discounted Return' samples of env's episode that was just stored, from its staged rewards (they stay
        where they are until the env's next episode overwrites them)."""
        if length > self.L:
            raise ValueError("the episode is longer than the staging area")
        if getattr(self, "_dr_scratch", None) is None or self._dr_scratch.numel() < length:
            self._dr_scratch = torch.empty(max(length, 1024), dtype=torch.float64, device=self.device)
        self.lib.episode_nstep_returns(self._stage["reward"][env * self.L:], None, self._dr_scratch, 0, length, 0, 1,
                                       self.L, float(discount), int(n_step), _rlx.current_stream())
        return self._dr_scratch[:length]

    def store(self, actions, rewards, game_overs, next_obs, reset_obs, record=True, dones=None, defer=False,
              episode_end=False, dones_host=None, masks=None):
        """The parent's signature.  The step's n_env transitions join their envs' staged episodes and the envs' current
        states advance; every env that `dones_host` (host flags of this step's episode ends) marks finished has its
        episode stored and made visible, in env order.  `defer` is not read: see the module text."""
        s = _rlx.current_stream()
        stored_go = game_overs
        if dones is not None:
            game_overs = dones
        if record and self._evaluating:
            raise RuntimeError("the replay memory is not written during evaluation")
        if record:
            if dones_host is None:
                raise ValueError("the n-step prioritized replay needs the host flags of the step's episode ends")
            if (self._staged_steps >= self.L).any():
                raise ValueError("an episode is longer than the staging area (%d steps)" % self.L)
            st = self._stage
            pairs = [(actions, st["action"]), (rewards, st["reward"]), (stored_go, st["game_over"]),
                     (self.cur_state, st["obs"]), (next_obs, st["next_obs"])] + self._mask_pair(masks)
            n, L = self.n_env, self.L
            if n == 1:
                dst_idx, dst_start = None, int(self._staged_steps[0])
            else:
                if self._stage_rows is None:
                    from ...staging import Stager
                    self._stage_rows = Stager((n,), torch.int32, self.device)
                dst_idx, dst_start = self._stage_rows.push((np.arange(n) * L + self._staged_steps).astype(np.int32)), 0
            self.lib.copy_columns(_rlx.make_columns(pairs), len(pairs), None, dst_idx, 0, dst_start, n, n * L, n,
                                  self.status, s)
            self._staged_steps += 1
        # the next state of a finished episode is the post-reset observation
        self.lib.select_rows(game_overs, reset_obs, next_obs, self.cur_state, self.n_env, self.obs_dim * 4, s)
        if record:
            for e in np.nonzero(np.asarray(dones_host))[0].tolist():
                self._store_episode(int(e))

    def _store_episode(self, env):
        T = int(self._staged_steps[env])
        self._staged_steps[env] = 0
        if T == 0:
            return
        if T > self.cap:
            raise ValueError("an episode of %d transitions is longer than the replay ring (%d)" % (T, self.cap))
        st = self._stage
        assert self.cursor == self.committed_total % self.rows
        self.lib.nstep_episode_store(st["obs"], st["next_obs"], st["action"], st["reward"], st["game_over"], env,
                                     self.n_env, self.L, T, self.n_step, self.discount, self.obs_dim, self.action_words,
                                     self.obs, self.next_obs, self.action, self.reward, self.game_over,
                                     self.n_step_discounted_rewards, self.should_bootstrap_next_state, self.cursor,
                                     self.rows, _rlx.current_stream())
        self.cursor = (self.cursor + T) % self.rows
        self._became_visible(T)

    def reserve_step(self, defer):
        raise NotImplementedError("the n-step prioritized replay stores whole episodes: it has no per-step rows")

    def store_device(self, *args, **kw):
        raise NotImplementedError("the n-step prioritized replay stores whole episodes: it has no per-step rows")

    # ----------------------------------------------------------------------------- training side
    def collate(self, drawn, size):
        batch = super().collate(drawn, size)
        b = self._batch_buffers(size)
        batch._info["n_step_discounted_rewards"] = b["n_step_discounted_rewards"]
        batch._info["should_bootstrap_next_state"] = b["should_bootstrap_next_state"]
        return batch
