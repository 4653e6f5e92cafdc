"""Off-policy evaluation of the trained Q network's softmax policy on the evaluation set of a Batch RL dataset —
the device form of rl_coach/off_policy_evaluators/ope_manager.py with bandits/doubly_robust.py,
rl/sequential_doubly_robust.py and rl/weighted_importance_sampling.py behind it.

The reference makes a Batch per inference batch, writes an info dictionary per transition and walks the episodes in two
nested Python loops.  Here the evaluation set's static columns (reward-model outputs, actions, rewards, the stored
behaviour probabilities, the first-row returns, the states, the episode offsets) are gathered to the device once
(``gather_static_shared_stats``), and one ``evaluate`` is the Q network's forward passes over the evaluation states, in
chunks, then three launches — rlx_ope_rows, and the two of rlx_ope_reduce — and ONE device-to-host copy of the five
estimates with the status word.  The arithmetic is stated in include/rlx.h and restated in tests/ope_ref.py.

The direct method's reward-model row.  ope_manager.py:80 multiplies the policy probabilities of inference batch i by
``all_reward_model_rewards[i]`` — the reward model's output for dataset ROW i, the array being concatenated over the whole
set already — so every row j is paired with row j // batch_size, not with its own.  That is reproduced by default (the
estimates are the reference's); ``OpeManager(per_row_direct_method=True)`` pairs row j with row j, the definition of the
paper (arXiv:1103.4601).  The doubly robust estimate's own correction term uses the right row either way, and adds
whichever direct method was computed.
"""
from collections import namedtuple

import numpy as np
import torch

from .. import _rlx

OpeEstimation = namedtuple("OpeEstimation", ['ips', 'dm', 'dr', 'seq_dr', 'wis'])
# the reference's dashboard signals, in OpeEstimation's order (value_optimization_agent.py:167-171)
SIGNAL_NAMES = ('Inverse Propensity Score', 'Direct Method Reward', 'Doubly Robust', 'Sequential Doubly Robust',
                'Weighted Importance Sampling')
ROW_COLUMNS = _rlx.CONSTANTS["RLX_OPE_ROW_COLUMNS"]
EPISODE_COLUMNS = _rlx.CONSTANTS["RLX_OPE_EPISODE_COLUMNS"]
OUT = _rlx.CONSTANTS["RLX_OPE_OUT"]
MAX_ACTIONS = _rlx.CONSTANTS["RLX_OPE_MAX_ACTIONS"]


def check_plain_q_head(agent, wrapper):
    """Only a plain Q head is served: the estimators read Q(s, .) of `networks['main']` and its softmax."""
    from ..agents.dqn_agent import DQNAgent
    from ..architectures.head_parameters import QHeadParameters
    from ..nn.networks import DQNNet
    heads = list(getattr(wrapper, "heads_parameters", []))
    if len(heads) != 1 or type(heads[0]) is not QHeadParameters or agent.NET is not DQNNet or \
            type(agent).choose_action is not DQNAgent.choose_action:
        raise ValueError("off-policy evaluation (should_get_softmax_probabilities) serves a plain Q head only, not "
                         "{} of {}".format([type(h).__name__ for h in heads], type(agent).__name__))
    if not 1 <= agent.A <= MAX_ACTIONS:
        raise ValueError("off-policy evaluation serves 1 to %d actions, got %d" % (MAX_ACTIONS, agent.A))


class OpeManager(object):
    CHUNK = 1024                  # rows of one forward pass over the evaluation set

    def __init__(self, per_row_direct_method=False):
        self.per_row_direct_method = bool(per_row_direct_method)
        self.lib = _rlx.lib()
        self.is_gathered_static_shared_data = False
        self.all_reward_model_rewards = self.all_old_policy_probs = self.all_rewards = self.all_actions = None
        self.all_returns = self.all_states = self.episode_offsets = None
        # what the reference writes into every transition's info / keeps in OpeSharedStats, as device columns
        self.all_q_values = self.all_policy_probs = self.row_columns = self.episode_columns = None

    @staticmethod
    def _evaluation_rows(memory):
        if getattr(memory, "evaluation_dataset_as_transitions", None) is None:
            raise ValueError("the memory has no evaluation dataset (prepare_evaluation_dataset)")
        if getattr(memory, "action_probabilities", None) is None:
            raise ValueError("the memory keeps no action-probabilities column: the dataset was collected without "
                             "should_get_softmax_probabilities")
        return memory.evaluation_dataset_as_transitions

    def gather_static_shared_stats(self, memory, batch_size, reward_model):
        """ope_manager.py:103-127, once per dataset: the reward model's forward over the evaluation set and the set's
        action / reward / behaviour-probability / return columns and states, gathered in chunks through the memory's
        listed-rows table; the episode offsets table.  Everything stays on the device."""
        first, end = self._evaluation_rows(memory)
        n, A, dev = end - first, memory.action_probabilities.shape[1], memory.device
        self.n, self.A, self.device = n, A, dev
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        self.all_reward_model_rewards, self.all_old_policy_probs, self.all_rewards = f32(n, A), f32(n, A), f32(n)
        self.all_actions = torch.empty(n, dtype=torch.int32, device=dev)
        self.all_returns = torch.empty(n, dtype=torch.float64, device=dev)
        self.all_states = f32(n, memory.obs_dim)
        for i in range(0, n, self.CHUNK):
            m = min(self.CHUNK, n - i)
            b = memory.gather(memory.physical_rows(np.arange(first + i, first + i + m)), m)
            self.all_states[i:i + m].copy_(b["state"])
            self.all_actions[i:i + m].copy_(b["action"])
            self.all_rewards[i:i + m].copy_(b["reward"])
            self.all_old_policy_probs[i:i + m].copy_(b["action_probabilities"])
            self.all_returns[i:i + m].copy_(b["n_step_discounted_rewards"])
            rm = reward_model.q_values(self.all_states[i:i + m], m, tag="ope_rm")
            self.all_reward_model_rewards[i:i + m].copy_(rm.data.view(m, A))
        offsets = [0] + [e - first for _, e in memory.evaluation_dataset_as_episodes]
        assert offsets[-1] == n
        self.episodes = len(offsets) - 1
        self.episode_offsets = torch.from_numpy(np.asarray(offsets, dtype=np.int32)).to(dev)
        self.all_q_values, self.all_policy_probs = f32(n, A), f32(n, A)
        self.row_columns = torch.zeros(ROW_COLUMNS, n, dtype=torch.float64, device=dev)
        self.episode_columns = torch.zeros(EPISODE_COLUMNS, self.episodes, dtype=torch.float64, device=dev)
        # the estimates and the status word leave in one copy: [OUT] doubles, then the int32 status in an eighth
        self._result = torch.zeros(OUT + 1, dtype=torch.float64, device=dev)
        self._status = self._result[OUT:].view(torch.int32)
        self._result_host = torch.zeros(OUT + 1, dtype=torch.float64).pin_memory()
        self.is_gathered_static_shared_data = True

    def evaluate(self, memory, batch_size, discount_factor, q_network, temperature):
        """ope_manager.py:129-151 -> OpeEstimation of Python floats.  Consumes no host random number and changes no
        weight.  Afterwards all_q_values / all_policy_probs [n, A], row_columns (rho, v, q of the taken action and the
        three per-row terms) and episode_columns (the episodes' sequential doubly robust values, weights w_e and w_e R_e)
        hold what the reference writes into the transitions' info."""
        assert self.is_gathered_static_shared_data, "gather_static_shared_stats() should be called once before " \
                                                    "calling _prepare_ope_shared_stats()"
        first, end = self._evaluation_rows(memory)
        if end - first != self.n:
            raise ValueError("the evaluation dataset changed since gather_static_shared_stats()")
        n, A, s = self.n, self.A, _rlx.current_stream()
        for i in range(0, n, self.CHUNK):
            m = min(self.CHUNK, n - i)
            q = q_network.q_values(self.all_states[i:i + m], m, tag="ope_q")
            self.all_q_values[i:i + m].copy_(q.data.view(m, A))
        divisor = 1 if self.per_row_direct_method else int(batch_size)
        self.lib.ope_rows(self.all_q_values, A, self.all_reward_model_rewards, A, divisor, self.all_actions,
                          self.all_rewards, self.all_old_policy_probs, A, float(temperature), n, A,
                          self.all_policy_probs, A, self.row_columns, self._status, s)
        self.lib.ope_reduce(self.episode_offsets, self.episodes, n, self.row_columns, self.all_rewards, self.all_returns,
                            float(discount_factor), self.episode_columns, self._result, s)
        self._result_host.copy_(self._result)                       # the one device-to-host copy (synchronises)
        host = self._result_host.numpy()
        if int(host[OUT:].view(np.int32)[0]):
            self._status.zero_()                                    # (zero since allocation until a launch sets it)
            raise ValueError("the evaluation set holds an action outside [0, %d)" % A)
        self.sum_of_weights = float(host[5])
        return OpeEstimation(*[float(x) for x in host[:5]])

    # the columns by the reference's names
    @property
    def rho_all_dataset(self):
        return self.row_columns[_rlx.CONSTANTS["RLX_OPE_COL_RHO"]]

    @property
    def all_v_values_q_model_based(self):
        return self.row_columns[_rlx.CONSTANTS["RLX_OPE_COL_V"]]

    @property
    def per_episode_seq_dr(self):
        return self.episode_columns[_rlx.CONSTANTS["RLX_OPE_EP_SEQ_DR"]]

    @property
    def per_episode_w_i(self):
        return self.episode_columns[_rlx.CONSTANTS["RLX_OPE_EP_W"]]
