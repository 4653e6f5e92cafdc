"""The on-policy base of the policy-optimisation family on one MI355X — host-side mirror of
rl_coach/agents/policy_optimization_agent.py (PolicyGradientRescaler :30-39, PolicyOptimizationAgent :45-162) for N
lockstep envs.  Its simplest member is PolicyGradientsAgent (agents/policy_gradients_agent.py); ActorCriticAgent
(agents/actor_critic_agent.py) bootstraps; NStepQAgent (agents/n_step_q_agent.py) trains a Q head with a target network
from the same windows and acts epsilon-greedily (`_make_exploration_policy`); ACERAgent (agents/acer_agent.py) trains
every window at once and adds replayed windows of complete episodes (`_make_episode_buffer`).

Every env is ONE reference agent's episode buffer (memories/episodic/single_episode_buffer.py: a staging buffer
[n_env, L]) with its own `last_gradient_update_step_idx`; the envs share the network, the per-timestep statistics and
the episode counter, as N reference agents run one after the other on one network would.  Stepping — act(), the reward
filter, the episode totals, evaluation, resets — is the vector agents' (agents/vector_agent.py; nothing of its replay
sampling or target-network cadence is used).

train(), called after every vector step like the reference's (graph_manager.py:463-489), restates :85-135 per env, in
env order:
  * the gate: `num_steps_between_gradient_updates` visible steps have passed since the env's last window, or its episode
    is complete.  A non-terminal step's response is observed at the start of the NEXT step (level_manager.py:236-264),
    so after such a step the episode buffer is one transition short of the steps taken; a terminal response is observed
    at once;
  * the window `episode[last_idx:]`, and the pointer move (:109-112): 0 when the episode is complete, else its length;
  * `_window_device`: returns, statistics, rescaling and the head's targets (one launch, rlx_pg_episode_window), then
    forward, head loss, backward and `accumulated += gradients` (PolicyGradientNet.accumulate_window);
  * the accumulated gradients are applied (one Adam step, then cleared) when `current_episode %
    apply_gradients_every_x_episodes == 0` — checked at EVERY window, as the reference does — with `current_episode` as
    handle_episode_ended left it: it counts an env's finished episode before that env's train();
  * `training_iteration` counts windows.
Window lengths differ from update to update, so train() issues its launches eagerly (the network context keys its
buffers by shape); acting is a captured graph.  Data-parallel training is refused: the reference's on-policy agents
train asynchronously (`async_training`), which has no mapping onto the synchronous gradient all-reduce yet.
"""
from enum import Enum

import numpy as np
import torch

from .. import _rlx
from ..core_types import RunPhase
from ..exploration_policies.categorical import Categorical
from ..memories.episodic.single_episode_buffer import SingleEpisodeBuffer
from .vector_agent import VectorOffPolicyAgent


class PolicyGradientRescaler(Enum):                      # policy_optimization_agent.py:30-39
    TOTAL_RETURN = 0
    FUTURE_RETURN = 1
    FUTURE_RETURN_NORMALIZED_BY_EPISODE = 2
    FUTURE_RETURN_NORMALIZED_BY_TIMESTEP = 3  # baselined
    Q_VALUE = 4
    A_VALUE = 5
    TD_RESIDUAL = 6
    DISCOUNTED_TD_RESIDUAL = 7
    GAE = 8


class PolicyOptimizationAgent(VectorOffPolicyAgent):
    """the stepping machinery of the vector agents under an on-policy train(); a subclass gives `_make_network` and
    `_window_device` (the reference's learn_from_batch on one window)."""
    SIGNAL_NAMES = VectorOffPolicyAgent.SIGNAL_NAMES + ["Entropy"]            # policy_optimization_agent.py:58

    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        # refused before anything touches the device
        if dist is not None and getattr(dist, "enabled", True):
            raise ValueError("data-parallel on-policy training is not served: the reference's policy-optimisation agents "
                             "train asynchronously (async_training), which has no mapping onto the gradient all-reduce")
        ep = environment.p
        if getattr(ep, "action_dim", None) is not None or not getattr(ep, "num_actions", None):
            raise ValueError("a Box action space needs the continuous PolicyHead, which is not served: the "
                             "policy-optimisation agents take discrete action spaces only")
        if getattr(ep, "kind", "vector") == "image":
            raise ValueError("image observations are not served by the on-policy agents' episode buffer")
        super().__init__(agent_parameters, environment, device, None, use_graphs)
        alg = self.ap.algorithm
        self.A = int(ep.num_actions)
        self.policy_gradient_rescaler = getattr(alg, "policy_gradient_rescaler", None)      # :49-51
        self.networks = {"main": self._make_network(tuple(ep.observation_shape), self.ap.network_wrappers["main"])}
        self.memory = self._make_episode_buffer(tuple(ep.observation_shape))
        self.exploration_policy = self._make_exploration_policy()
        dev, n, L = self.device, self.n_env, self.L
        self.actions = torch.zeros(n, dtype=torch.int32, device=dev)
        self.action_probabilities = torch.zeros(n, self.A, dtype=torch.float32, device=dev)
        self.entropy = torch.zeros(n, dtype=torch.float32, device=dev)         # the 'Entropy' samples of the last step
        # statistics for variance reduction (:53-57): sized by the environment's episode limit, not 100 000
        self.last_gradient_update_step_idx = np.zeros(n, dtype=np.int64)
        self.max_episode_length = L
        self.mean_return_over_multiple_episodes = torch.zeros(L, dtype=torch.float64, device=dev)
        self.num_episodes_where_step_has_been_seen = torch.zeros(L, dtype=torch.float64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.current_episode = 0
        self.debug_windows = None        # tests set this to a list: (env, start, end, current_episode, applied) per window
        self._finish_init()

    @property
    def is_on_policy(self):
        return True

    def _make_network(self, obs_shape, wrapper):
        raise NotImplementedError

    def _make_episode_buffer(self, obs_shape):
        """the staging buffer of the running episodes; ACER's also keeps the acting probabilities and feeds a replay"""
        return SingleEpisodeBuffer(self.device, self.n_env, obs_shape, self.L)

    def _make_exploration_policy(self):
        """the family acts by a categorical draw on the policy head; a value-based member (N-step Q) gives its own"""
        return Categorical(self.A, self.n_env, self.device, self.ap.exploration)

    def _window_device(self, env, start, end, complete):
        """learn_from_batch on steps [start, end) of env's episode: the gradients are accumulated -> the loss"""
        raise NotImplementedError("PolicyOptimizationAgent is an abstract agent. Not to be used directly.")

    # --------------------------------------------------------------------------------- acting
    def random_actions(self):
        a = np.array([np.random.choice(self.A) for _ in range(self.n_env)], dtype=np.int32)
        self.actions.copy_(self._to_device("rand_act", a, torch.int32))
        return self.actions

    def _act_device(self, states, uniforms):
        z = self.networks["main"].policy_values(states, self.n_env, tag="act")
        self.exploration_policy.select(z.data, self.A, self.action_probabilities, self.actions, uniforms)
        # -sum p log(p + eps) (:154), a sample per env
        self.lib.action_entropy(self.action_probabilities, self.A, self.n_env, self.A, self.entropy,
                                _rlx.current_stream())

    def choose_action(self, states):
        pol = self.exploration_policy
        pol.phase = self.phase
        u = pol.draw()                                               # host RNG, per env, in order
        staged = pol.stage(u) if u is not None else None
        self._run(("act", staged is not None, states.data_ptr()), lambda: self._act_device(states, staged))
        if self.signal_stats is not None:
            self.signal_stats.accumulate({"Entropy": self.entropy})
        return self.actions

    def handle_episode_ended(self):
        if self.phase == RunPhase.HEATUP:                            # agent.py:572-573 (TRAIN: counted per env in train())
            self.current_episode += len(self.ended_episode_lengths)

    def _note_finished_episodes(self, ended):
        """the episode log of the CSV rows; the 'Discounted Return' samples come from the window launch"""
        host = torch.empty(self.n_env, dtype=torch.float64, pin_memory=True)
        host.copy_(self.last_return, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        for e, length in zip(ended.tolist(), self.ended_episode_lengths.tolist()):
            self._episode_log.append((int(e), int(length), host, ev))

    def reset_internal_state(self):
        """the running episodes are abandoned with their update pointers (a pointer into an episode that no longer
        exists would slice the next one in the middle)"""
        self.last_gradient_update_step_idx[:] = 0
        return super().reset_internal_state()

    # ------------------------------------------------------------------------------- training
    def _apply_gradients(self):
        self.networks["main"].apply_accumulated(self._grad_scale())

    def train(self):
        """PolicyOptimizationAgent.train (:85-135) for every env, in env order -> the loss of the last window (a device
        scalar), or None when nothing was due."""
        if self.phase != RunPhase.TRAIN:
            return None
        alg = self.ap.algorithm
        t_max = alg.num_steps_between_gradient_updates
        ended = (self._episode_steps == 0) if self._episode_just_ended else np.zeros(self.n_env, dtype=bool)
        lengths = dict(zip(np.nonzero(ended)[0].tolist(), self.ended_episode_lengths.tolist())) \
            if self._episode_just_ended else {}
        last, loss = self.last_gradient_update_step_idx, None
        for e in range(self.n_env):
            complete = bool(ended[e])
            if complete:
                self.current_episode += 1                            # handle_episode_ended ran before this env's train()
            # the transitions the env's episode buffer holds now (see the module text)
            length = int(lengths[e]) if complete else int(self._episode_steps[e]) - 1
            passed = length - int(last[e])
            if not (passed >= t_max or complete) or passed <= 0:
                continue
            start = int(last[e])
            loss = self._window_device(e, start, length, complete)
            last[e] = 0 if complete else length                      # :109-112
            applied = self.current_episode % alg.apply_gradients_every_x_episodes == 0
            if applied:
                self._apply_gradients()                              # apply_gradients_and_sync_networks
            self.training_iteration += 1
            if self.debug_windows is not None:
                self.debug_windows.append((e, start, length, self.current_episode, applied))
            if self.signal_stats is not None:
                self._accumulate_signals()
            if self.debug_losses is not None:
                self.debug_losses.append(float(loss.sum().item()))
        return loss

    def check_status(self):
        super().check_status()
        st = int(self.status.item())
        if st:
            self.status.zero_()
            raise ValueError("an episode is longer than the per-timestep statistics arrays (%d steps; status bits %d)"
                             % (self.max_episode_length, st))
