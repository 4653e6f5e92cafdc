"""Wolpertinger on one MI355X — host-side mirror of rl_coach/agents/wolpertinger_agent.py (parameter classes :33-65,
WolpertingerAgent.learn_from_batch :72-85, choose_action :90-109, get_initialized_knn :116-128) and of the
WolpertingerActorHead (architectures/tensorflow_components/heads/wolpertinger_actor_head.py:27-56).  Dulac-Arnold et al.
2015, "Deep Reinforcement Learning in Large Discrete Action Spaces", https://arxiv.org/abs/1512.07679.

DDPG over a discretised box: the agent's action space is the DiscreteActionSpace a BoxDiscretization output filter makes
of the environment's box.  Per step the online actor gives a proto-action (its head: tanh times the box's max_abs_range),
AdditiveNoise adds absolute Gaussian noise (host draws at the stream positions the reference's get_action makes them),
the k nearest of the n actions' embeddings are looked up (rlx_knn_topk: exact and ordered, where the reference queries
an approximate Annoy forest on the host), the online critic scores the k candidates and the best one's INDEX is the
action: it is what the replay stores and the `actions` signal records; the environment receives
target_actions[action].  Per update the batch's discrete actions become box points (rlx_discrete_to_box, inside the
captured update) and DDPG's update runs unchanged.

Two tables, both built once on the host with the reference's numpy expressions and uploaded as fp32:
  keys            expand_dims((arange(n) / (n - 1) - 0.5) * 2, 1) * max_abs_range     wolpertinger_agent.py:122
  target_actions  BoxDiscretization's product of np.linspace(low, high, bins)          filters/action.py
They are different expressions and may differ in the last bit; the lookup and the critic's acting input use the keys,
the environment and the update the target actions, as in the reference.
"""
from collections import OrderedDict

import numpy as np
import torch

from .. import _rlx
from ..architectures.head_parameters import WolpertingerActorHeadParameters
from ..exploration_policies.additive_noise import AdditiveNoiseParameters
from ..filters.action import BoxDiscretization
from ..memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters
from .ddpg_agent import (DDPGActorNetworkParameters, DDPGAgent, DDPGAlgorithmParameters,
                         DDPGCriticNetworkParameters)


class WolpertingerCriticNetworkParameters(DDPGCriticNetworkParameters):      # wolpertinger_agent.py:33-35
    def __init__(self, use_batchnorm=False):
        super().__init__(use_batchnorm=use_batchnorm)


class WolpertingerActorNetworkParameters(DDPGActorNetworkParameters):        # wolpertinger_agent.py:38-41
    def __init__(self, use_batchnorm=False):
        super().__init__()                   # (the reference passes use_batchnorm to the head alone)
        self.heads_parameters = [WolpertingerActorHeadParameters(batchnorm=use_batchnorm)]


class WolpertingerAlgorithmParameters(DDPGAlgorithmParameters):              # wolpertinger_agent.py:44-48
    def __init__(self):
        super().__init__()
        self.action_embedding_width = 1
        self.k = 1


class WolpertingerAgentParameters(object):                                   # wolpertinger_agent.py:51-65
    def __init__(self, use_batchnorm=False):
        self.algorithm = WolpertingerAlgorithmParameters()
        self.exploration = AdditiveNoiseParameters()
        self.exploration.noise_as_percentage_from_action_space = False
        self.memory = EpisodicExperienceReplayParameters()
        self.network_wrappers = OrderedDict([("actor", WolpertingerActorNetworkParameters(use_batchnorm=use_batchnorm)),
                                             ("critic", WolpertingerCriticNetworkParameters(use_batchnorm=use_batchnorm))])
        self.output_filter = None            # presets set an OutputFilter holding one BoxDiscretization
        self.seed = 0

    @property
    def path(self):
        return 'coach_amd.agents.wolpertinger_agent:WolpertingerAgent'


def knn_keys(num_actions, max_abs_range):
    """get_initialized_knn's keys (wolpertinger_agent.py:118-122), fp64 [n][len(max_abs_range)]; Annoy stores them as fp32"""
    return np.expand_dims((np.arange(num_actions) / (num_actions - 1) - 0.5) * 2, 1) * max_abs_range


def discretization_of(agent_parameters):
    """the BoxDiscretization of the agent's output filter, or None"""
    flt = getattr(agent_parameters, "output_filter", None)
    filters = list(getattr(flt, "action_filters", {}).values()) if flt is not None else []
    return filters[0] if len(filters) == 1 and isinstance(filters[0], BoxDiscretization) else None


class WolpertingerAgent(DDPGAgent):
    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        ep, alg = environment.p, agent_parameters.algorithm
        disc = discretization_of(agent_parameters)
        if ep.kind == "image":
            raise ValueError("WolpertingerAgent works only for vector observations (DDPG's networks)")
        if disc is None or getattr(ep, "action_dim", None) is None:
            # the agent's own action space must be the DiscreteActionSpace an output filter makes of a box
            raise ValueError("WolpertingerAgent works only for discrete control problems")     # wolpertinger_agent.py:91-92
        if alg.action_embedding_width != 1 or int(ep.action_dim) != 1:
            # get_initialized_knn's keys are [n][box dimensions] while the Annoy index and the actor's head are
            # action_embedding_width wide: only 1 and 1 agree
            raise ValueError("WolpertingerAgent needs action_embedding_width = 1 and a one-dimensional box (got width {} "
                             "and {} dimensions): the reference's own key table has another shape otherwise"
                             .format(alg.action_embedding_width, ep.action_dim))
        low = np.broadcast_to(np.asarray(ep.action_low, dtype=np.float32), (int(ep.action_dim),))
        high = np.broadcast_to(np.asarray(ep.action_high, dtype=np.float32), (int(ep.action_dim),))
        self.n_actions = int(disc.get_unfiltered_action_space(low, high))
        self.k = int(alg.k)
        if self.n_actions < 2:
            raise ValueError("WolpertingerAgent needs at least 2 discrete actions (the keys divide by n - 1), got {}"
                             .format(self.n_actions))
        if not 1 <= self.k <= min(self.n_actions, 64):
            raise ValueError("WolpertingerAgent: k = {} outside [1, min(number of actions = {}, 64)]"
                             .format(self.k, self.n_actions))
        self.discretization = disc
        self.keys = knn_keys(self.n_actions, np.maximum(np.abs(low), np.abs(high)))
        super().__init__(agent_parameters, environment, device, dist, use_graphs)
        dev, n, k, W = self.device, self.n_env, self.k, self._actor_outputs()
        self.d_keys = torch.from_numpy(self.keys.astype(np.float32)).to(dev)
        self.d_target_actions = torch.from_numpy(disc.target_actions.astype(np.float32)).to(dev)
        self.actions = torch.zeros(n, dtype=torch.int32, device=dev)                 # the discrete actions: stored, logged
        self.env_actions = torch.zeros(n, self.A, dtype=torch.float32, device=dev)   # target_actions[actions]: executed
        self.proto = torch.zeros(n, W, dtype=torch.float32, device=dev)              # the noisy proto-actions
        self.nn_idx = torch.zeros(n, k, dtype=torch.int32, device=dev)
        self.cand_obs = torch.zeros(n * k, self.obs_dim, dtype=torch.float32, device=dev)
        self.cand_act = torch.zeros(n * k, W, dtype=torch.float32, device=dev)
        self.cand_q = None                                                           # [n * k] once the critic ran
        self.box_actions = torch.zeros(self.batch_size, self.A, dtype=torch.float32, device=dev)
        self.convert_status = torch.zeros(1, dtype=torch.int32, device=dev)
        import ctypes
        nbytes = ctypes.c_longlong()
        self.lib.knn_topk_scratch_bytes(n, self.n_actions, k, ctypes.byref(nbytes))
        self._knn_scratch_bytes = int(nbytes.value)
        self.knn_scratch = torch.zeros(max(1, self._knn_scratch_bytes // 8), dtype=torch.int64, device=dev)

    def _actor_outputs(self):
        return int(self.ap.algorithm.action_embedding_width)

    def _replay_action_dim(self):
        return None                          # the replay holds the discrete action (wolpertinger_agent.py:73-77)

    # --------------------------------------------------------------------------------- acting
    def random_actions(self):
        """DiscreteActionSpace.sample (spaces.py:406-407): np.random.choice(actions) per env, as the DQN agents draw it"""
        a = np.array([np.random.choice(self.n_actions) for _ in range(self.n_env)], dtype=np.int32)
        self.actions.copy_(self._to_device("rand_act", a, torch.int32))
        self._to_box(self.actions, self.n_env, self.env_actions)
        return self.actions

    def choose_action(self, states):
        """wolpertinger_agent.py:90-109.  use_target_network_for_evaluation plays no part: both networks are the online
        ones."""
        self.exploration_policy.phase = self.phase
        self._run(("mu", False), lambda: self._mu_forward(states, False))
        self.exploration_policy.get_action(self._mu_act, self.proto)
        self._run(("rank",), lambda: self._rank(states))
        if self.signal_stats is not None:
            self.signal_stats.accumulate({"actions": self.actions.to(torch.float32)})
        return self.actions

    def _rank(self, states):
        """proto-actions -> their k nearest keys -> the online critic on the n_env * k candidates -> the best index"""
        s, n, k, W = _rlx.current_stream(), self.n_env, self.k, self._actor_outputs()
        self.lib.knn_topk(self.proto, W, n, W, self.d_keys, W, self.n_actions, k, self.nn_idx, None, self.knn_scratch,
                          self._knn_scratch_bytes, s)
        self.lib.wolpertinger_candidates(self.nn_idx, self.d_keys, W, self.n_actions, W, states, self.obs_dim,
                                         self.obs_dim, n, k, self.cand_obs, self.obs_dim, self.cand_act, W, s)
        q, _ = self.networks["critic"].forward(self.cand_obs, self.cand_act, n * k, tag="rank")
        self.cand_q = q[0]
        self.lib.wolpertinger_select(self.cand_q, 1, self.nn_idx, n, k, self.d_target_actions, self.A, self.n_actions,
                                     self.A, self.actions, self.env_actions, self.A, s)

    def _env_actions(self, actions):
        return self.env_actions

    # ------------------------------------------------------------------------------- training
    def _to_box(self, actions, rows, out):
        self.lib.discrete_to_box(actions, rows, self.d_target_actions, self.A, self.n_actions, self.A, out, self.A,
                                 self.convert_status, _rlx.current_stream())

    def _batch_actions(self, b):
        """the output filter on every action of the batch (wolpertinger_agent.py:79-83): one launch of the update"""
        self._to_box(b.actions(), self.batch_size, self.box_actions)
        return self.box_actions

    def check_status(self):
        super().check_status()
        if int(self.convert_status.item()) != 0:
            raise RuntimeError("WolpertingerAgent: a stored action lies outside the {} discrete actions"
                               .format(self.n_actions))
