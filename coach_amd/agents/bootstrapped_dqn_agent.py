"""Bootstrapped DQN on one MI355X — host-side mirror of rl_coach/agents/bootstrapped_dqn_agent.py (parameter classes
:26-41, BootstrappedDQNAgent :45-92) and rl_coach/exploration_policies/bootstrapped.py.

K copies of the Q head on one torso (nn.networks.BootstrappedDQNNet: one Dense(feat, K * A)).  Every stored transition
carries a K-bit mask — which heads learn from it — in the replay's mask column; every env follows one head per episode
while training and the heads' majority vote otherwise.  With UCBParameters as the exploration parameters
(exploration_policies/ucb.py) the same ensemble is acted on by mean + lamb * std over the heads instead: no head is
selected or staged, the masks are drawn as before.
Per step: every head's Q values -> rlx_bootstrapped_egreedy (selected head or vote, then the epsilon-greedy choice) or
rlx_ucb_egreedy.
Per update: online(s'), target(s'), online(s) -> rlx_bootstrapped_dqn_head_loss (per head a Double-DQN target where the
mask has its bit, the K head losses and their sum, dQ) -> backward (the torso gets 1 / K of the heads' summed gradient)
-> TF1 Adam.

Host draws, on the global legacy np.random stream, where the reference makes them (level_manager.py:215-269):
  * reset_internal_state -> select_head: np.random.randint(K) for every env that starts an episode, in env order, at
    the start of the step (every phase) -- Bootstrapped only, UCB draws nothing here;
  * observe -> np.random.binomial(1, p, K) per env, in env order: at the start of every step (the previous response —
    at an episode's first step the initial one, whose draw is discarded as in the reference) and once more right after
    the env step for every env whose episode ended on it (a terminal response is observed at once);
  * then EGreedy's draws and the replay's, as for DQN.
A transition's mask is therefore drawn AFTER its row was written (rows are written at once and become visible at the next
step): the store writes all ones, the row's word is corrected by a small launch after the draw when p < 1 (with p = 1
the draw is made — it consumes K doubles — but cannot differ).
"""
import numpy as np
import torch

from .. import _rlx
from ..core_types import RunPhase
from ..exploration_policies.bootstrapped import Bootstrapped, BootstrappedParameters
from ..exploration_policies.parameter_noise import network_is_noisy
from ..exploration_policies.ucb import UCB, UCBParameters
from ..memories.non_episodic.experience_replay import ExperienceReplay
from ..nn.networks import BootstrappedDQNNet
from .dqn_agent import DQNAgent, DQNAgentParameters, DQNNetworkParameters


class BootstrappedDQNNetworkParameters(DQNNetworkParameters):            # bootstrapped_dqn_agent.py:26-30
    def __init__(self):
        super().__init__()
        self.heads_parameters[0].num_output_head_copies = 10
        self.heads_parameters[0].rescale_gradient_from_head_by_factor = \
            1.0 / self.heads_parameters[0].num_output_head_copies


class BootstrappedDQNAgentParameters(DQNAgentParameters):                # bootstrapped_dqn_agent.py:33-41
    def __init__(self):
        super().__init__()
        self.exploration = BootstrappedParameters()
        self.network_wrappers = {"main": BootstrappedDQNNetworkParameters()}

    @property
    def path(self):
        return 'coach_amd.agents.bootstrapped_dqn_agent:BootstrappedDQNAgent'


def mask_words(bits):
    """[..., K] 0 / 1 draws -> the rows' 32-bit words (bit h = head h) as int32 (the uint32 bit pattern)."""
    bits = np.asarray(bits, dtype=np.uint64)
    w = (bits << np.arange(bits.shape[-1], dtype=np.uint64)).sum(axis=-1).astype(np.uint32)
    return w.view(np.int32) if w.ndim else np.array([w], np.uint32).view(np.int32)[0]


class BootstrappedDQNAgent(DQNAgent):
    MASK_COLUMN = True
    ucb = False                      # True with UCBParameters: mean + lamb * std over the heads, no selected head
    PER_REFUSAL = ("BootstrappedDQNAgent does not use replay priorities (the reference agent passes no importance "
                   "weights to its heads and never updates priorities), and its transitions carry a head mask: use "
                   "an ExperienceReplay memory")
    NET = BootstrappedDQNNet

    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        super().__init__(agent_parameters, environment, device, dist, use_graphs)
        self.share_p = float(self.ap.exploration.bootstrapped_data_sharing_probability)
        self.last_action_values = torch.zeros(self.n_env, self.A, dtype=torch.float32, device=self.device)
        self._needs_head = np.ones(self.n_env, dtype=bool)          # envs whose next step starts an episode
        self._open_rows = None          # physical rows of the last stored step whose masks are not drawn yet, per env
        self.debug_masks = None         # tests set this to a list: (physical row, mask word) of every stored transition

    def _check_parameters(self):
        exp = self.ap.exploration
        if not isinstance(exp, (BootstrappedParameters, UCBParameters)):
            raise ValueError("BootstrappedDQNAgent explores with the Bootstrapped policy (BootstrappedParameters) or "
                             "with UCB over its heads (UCBParameters)")
        self.ucb = isinstance(exp, UCBParameters)
        self.K = int(self.ap.network_wrappers["main"].heads_parameters[0].num_output_head_copies)
        if int(exp.architecture_num_q_heads) != self.K:
            raise ValueError("exploration.architecture_num_q_heads (%d) and the head's num_output_head_copies (%d) differ"
                             % (exp.architecture_num_q_heads, self.K))
        self.parameter_noise = False

    def _network_arguments(self, net):
        return (self.K,), dict(noisy=network_is_noisy(net))          # (a noisy network: refused by the network)

    def _check_memory(self):
        if type(self.memory) is not ExperienceReplay:
            raise ValueError(self.PER_REFUSAL)

    # ------------------------------------------------------------------------ host draws (see the module text)
    def _draw_mask(self):
        return mask_words(np.random.binomial(1, self.share_p, self.K))       # observe (:88-92)

    def _observe_previous_host(self, record):
        starting = np.nonzero(self._needs_head)[0]
        if starting.size:
            self.exploration_policy.select_head(starting)                     # reset_internal_state (:53-55)
            self._needs_head[:] = False
        words = np.array([self._draw_mask() for _ in range(self.n_env)], dtype=np.int32)
        rows, self._open_rows = self._open_rows, None
        if rows is None or not record:
            return
        live = rows >= 0                     # (an env whose last response was terminal was observed at once)
        if self.debug_masks is not None:
            self.debug_masks.extend((int(r), int(w)) for r, w in zip(rows[live], words[live].view(np.uint32)))
        if self.share_p < 1.0 and live.any():
            # rows of envs that are not open any more repeat a live one: the same word twice, whatever the order
            first = int(np.nonzero(live)[0][0])
            rows = np.where(live, rows, rows[first]).astype(np.int32)
            words = np.where(live, words, words[first]).astype(np.int32)
            self.memory.set_masks(self._to_device("mask_rows", rows, torch.int32),
                                  self._to_device("mask_fix", words, torch.int32), self.n_env)

    def _store_extra_host(self, dones_host, record):
        ended = np.nonzero(dones_host)[0]
        # all K bits until the row's own draw (see the module text)
        words = np.full(self.n_env, (1 << self.K) - 1, dtype=np.uint32).view(np.int32)
        for e in ended:
            words[e] = self._draw_mask()                         # the terminal response is observed at once
        self._needs_head[ended] = True
        if not record:
            return {}
        mem = self.memory
        rows = ((mem.cursor + np.arange(self.n_env)) % mem.rows).astype(np.int32)
        if self.debug_masks is not None:
            self.debug_masks.extend((int(rows[e]), int(words[e:e + 1].view(np.uint32)[0])) for e in ended)
        rows[ended] = -1
        self._open_rows = rows if (rows >= 0).any() else None
        return {"masks": self._to_device("mask_store", words, torch.int32)}

    def reset_internal_state(self):
        self._needs_head[:] = True
        self._open_rows = None               # the last response is never observed: its row is dropped, its draw never made
        return super().reset_internal_state()

    # --------------------------------------------------------------------------------- acting
    def _make_exploration_policy(self):
        policy = UCB if isinstance(self.ap.exploration, UCBParameters) else Bootstrapped
        return policy(self.A, self.n_env, self.device, self.ap.exploration)

    def choose_action(self, states):
        pol = self.exploration_policy
        pol.phase = self.phase
        draws = pol.draw()                                                   # EGreedy's, per env, in order
        self._run(("q", self.n_env), lambda: self._q_forward(states))
        eps, d = pol.stage(draws)
        self._heads_dev = None if self.ucb else pol.stage_heads()
        self._select_actions(d["u"], d["ra"], d["tie"], eps)
        return self.actions

    def _q_forward(self, states):
        self._q_act = self.networks["main"].head_output(states, self.n_env, tag="act").data.view(
            self.n_env, self.K * self.A)

    def _select_actions(self, u, ra, tie, eps):
        """Bootstrapped.get_action (bootstrapped.py:72-85): the selected head's values in TRAIN, the vote otherwise.
        UCB.get_action (ucb.py:76-86): the heads' mean + lamb * std in TRAIN, the mean otherwise."""
        if self.ucb:
            pol = self.exploration_policy
            self.lib.ucb_egreedy(self._q_act, self.K * self.A, self.K, float(pol.lamb), int(pol.use_std), u, ra, tie,
                                 float(eps), self.n_env, self.A, self.last_action_values, pol.std, self.actions,
                                 _rlx.current_stream())
            return
        self.lib.bootstrapped_egreedy(self._q_act, self.K * self.A, self.K, self._heads_dev,
                                      int(self.phase != RunPhase.TRAIN), u, ra, tie, float(eps), self.n_env, self.A,
                                      self.last_action_values, self.actions, _rlx.current_stream())

    # ------------------------------------------------------------------------------- training
    def _step_graph_ok(self):
        """the one-graph-per-env-step path of DQNAgent is declined: its record has no masks and no selected heads"""
        return False

    def _learn_device(self, b, weights=None, per_ride=None):
        self.networks["main"].learn_from_batch(
            b._states["observation"], b._next_states["observation"], self.batch_size, b.actions(), b.rewards(),
            b.game_overs(), b.info("mask"), self.ap.algorithm.discount, grad_scale=self._grad_scale(),
            sync=self if self.dist is not None else None, states_pair=b._info.get("states_pair"))

    def learn_from_batch(self, batch):
        """BootstrappedDQNAgent.learn_from_batch (bootstrapped_dqn_agent.py:57-86)."""
        self._run(("learn", False, False), lambda: self._learn_device(batch))
        # 'Q': every head's online prediction on the batch's states (the reference samples its TD-target arrays in the
        # middle of the loop that fills them, :75)
        return self._loss_signals(Q=self.networks["main"].last_q.view(-1))
