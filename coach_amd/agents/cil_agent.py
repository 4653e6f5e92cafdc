"""Conditional Imitation Learning on one MI355X — host-side mirror of rl_coach/agents/cil_agent.py (parameter classes
:28-59, CILAgent :63-87).  Codevilla et al. 2017, https://arxiv.org/abs/1710.02410.

The network is nn.networks.CILNet: a vector embedder and an FC middleware under one RegressionHead copy per high-level
command (G.BranchStack, csrc/cil.hip).  The command is a width-1 slice of the environment's observation vector, named by
algorithm.state_key_with_the_class_index; the other columns are what the embedder reads.  The replay stores the whole
observation row, so the command and the float action are replay columns; rlx_cil_split_observation makes the embedder's
input and the int32 commands from a batch of rows (or from the current state) in one launch.

Acting (:68-73 + ImitationAgent.choose_action): the clean prediction of the row's own branch (rlx_cil_branches_forward
with the commands), then the exploration policy FORCED into RunPhase.TEST — AdditiveNoise adds nothing there.
learn_from_batch (:75-87): the reference's predict, target assembly and training pass are CILNet.learn_from_batch, one
captured graph per batch size; each replay draws new dropout masks.

Memory: BalancedExperienceReplay; the host learns each stored row's class from the state the agent acted on.

Served: vector observations with a slice table, a Box action space, AdditiveNoiseParameters, one environment, one GPU.
Refused by name before anything touches the device: image observations, discrete actions, ParameterNoise and every
other exploration policy, data-parallel training, load_memory_from_file_path (a pickled replay buffer or a CSV file).
"""
import numpy as np
import torch

from ..architectures.head_parameters import RegressionHeadParameters
from ..architectures.scheme_views import SchemeViews
from ..core_types import EnvironmentSteps, RunPhase
from ..exploration_policies.additive_noise import AdditiveNoiseParameters
from ..exploration_policies.e_greedy import EGreedyParameters
from ..exploration_policies.parameter_noise import ParameterNoiseParameters, network_is_noisy
from ..memories.non_episodic.balanced_experience_replay import (BalancedExperienceReplay,
                                                                 BalancedExperienceReplayParameters)
from ..nn.networks import CILNet, cil_net_kwargs
from .vector_agent import AlgorithmParameters, BoxActionAgent, VectorOffPolicyAgent


class CILAlgorithmParameters(AlgorithmParameters):       # cil_agent.py:28-35
    def __init__(self):
        super().__init__()
        self.state_key_with_the_class_index = 'high_level_command'


class CILNetworkParameters(SchemeViews):                 # cil_agent.py:38-47 + NetworkParameters defaults
    def __init__(self):
        self.activation_function = 'relu'
        self.embedder_scheme = 'Medium'
        self.middleware_scheme = 'Medium'
        self.heads_parameters = [RegressionHeadParameters()]
        self.optimizer_type = 'Adam'
        self.batch_size = 32
        self.replace_mse_with_huber_loss = False
        self.create_target_network = False
        self.learning_rate = 0.00025
        self.adam_optimizer_beta1 = 0.9
        self.adam_optimizer_beta2 = 0.99
        self.optimizer_epsilon = 0.0001
        self.scale_down_gradients_by_number_of_workers_for_sync_training = True
        self.clip_gradients = None


class CILAgentParameters(object):                        # cil_agent.py:50-59
    def __init__(self):
        self.algorithm = CILAlgorithmParameters()
        self.exploration = EGreedyParameters()           # the reference's default; CARLA_CIL sets AdditiveNoiseParameters
        self.memory = BalancedExperienceReplayParameters()
        self.network_wrappers = {"main": CILNetworkParameters()}
        self.seed = 0

    @property
    def path(self):
        return 'coach_amd.agents.cil_agent:CILAgent'


def check_cil_parameters(ap, ep, dist=None):
    """what CILAgent refuses, before anything touches the device -> (class column, embedder width, action dimension)"""
    from ..core_types import PickledReplayBuffer
    if dist is not None and getattr(dist, "enabled", True):
        raise ValueError("data-parallel training is not served by CILAgent")
    if getattr(ep, "kind", "vector") == "image":
        raise ValueError("CILAgent serves vector observations, not image observations")
    if getattr(ep, "action_dim", None) is None:
        raise ValueError("CILAgent serves a Box action space, not discrete actions (its heads regress the action)")
    net = ap.network_wrappers["main"]
    if isinstance(ap.exploration, ParameterNoiseParameters) or network_is_noisy(net):
        raise ValueError("the ParameterNoise exploration policy (noisy dense layers) is not implemented for CILAgent")
    if not isinstance(ap.exploration, AdditiveNoiseParameters):
        raise ValueError("CILAgent acts under AdditiveNoiseParameters (as CARLA_CIL sets it), not %s"
                         % type(ap.exploration).__name__)
    if not isinstance(ap.memory, BalancedExperienceReplayParameters):
        raise ValueError("CILAgent's memory is a BalancedExperienceReplay, not %s" % type(ap.memory).__name__)
    dataset = getattr(ap.memory, "load_memory_from_file_path", None)
    if isinstance(dataset, PickledReplayBuffer):
        raise ValueError("Loading a pickled replay buffer ({}) is not served: a pickle of the reference's Transition "
                         "objects is bound to its classes".format(dataset.filepath))
    if dataset:
        raise ValueError("load_memory_from_file_path ({}) is not served by CILAgent: a BalancedExperienceReplay is "
                         "filled through store()".format(dataset))
    if int(getattr(ep, "num_envs", 1)) != 1:
        raise ValueError("CILAgent steps one environment (num_envs = 1), got %d" % ep.num_envs)
    key = ap.algorithm.state_key_with_the_class_index
    slices = dict(getattr(ep, "observation_slices", None) or {})
    if key not in slices or slices[key][1] - slices[key][0] != 1:
        raise ValueError("CILAgent: the environment's observation has no width-1 slice named {!r} "
                         "(state_key_with_the_class_index); its slices: {}".format(key, sorted(slices) or "(none)"))
    if ap.memory.state_key_with_the_class_index != key:                   # balanced_experience_replay.py:82-84
        raise ValueError("The class index was not present in the state of the transition under the given key ({})"
                         .format(ap.memory.state_key_with_the_class_index))
    names = getattr(net, "input_embedder_names", None)
    rest = tuple(sorted((k for k in slices if k != key), key=lambda k: slices[k][0]))
    if names is not None and (tuple(names) != tuple(sorted(rest)) or tuple(names) != rest):
        raise ValueError("the input embedders {} do not match the environment's observation slices {} without {!r}"
                         .format(list(names), list(rest), key))
    heads = list(net.heads_parameters)
    if len(heads) == 1 and isinstance(heads[0], RegressionHeadParameters) and \
            heads[0].num_output_head_copies != ap.memory.num_classes:
        raise ValueError("CILAgent: num_output_head_copies = {} regression heads for memory.num_classes = {} commands"
                         .format(heads[0].num_output_head_copies, ap.memory.num_classes))
    return int(slices[key][0]), int(ep.observation_shape[0]) - 1, int(ep.action_dim)


class CILAgent(BoxActionAgent):
    imitation = True
    is_on_policy = False

    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        ap, ep = agent_parameters, environment.p
        self.class_column, self.embedder_dim, _ = check_cil_parameters(ap, ep, dist)
        VectorOffPolicyAgent.__init__(self, ap, environment, device, None, use_graphs)
        net, mp = ap.network_wrappers["main"], ap.memory
        self.obs_dim = int(ep.observation_shape[0])
        self._set_action_bounds(ep)
        self.batch_size = net.batch_size
        self.networks = {"main": CILNet(self.device, (self.embedder_dim,), self.A, **cil_net_kwargs(net, ap.seed or 0))}
        self.memory = BalancedExperienceReplay(
            mp.max_size, mp.allow_duplicates_in_batch_sampling, mp.num_classes, mp.state_key_with_the_class_index,
            class_column=self.class_column, device=self.device, n_env=self.n_env,
            observation_shape=ep.observation_shape, action_dim=self.A)
        self.exploration_policy = self._make_exploration()
        self.actions = torch.zeros(self.n_env, self.A, dtype=torch.float32, device=self.device)
        self._views = {}
        self._finish_init()

    def _check_input_embedder_names(self, ep):
        """(check_cil_parameters: the embedders' names are the environment's slices WITHOUT the class slice)"""

    def _split(self, obs, B, tag):
        """stored observation rows -> (the embedder's input [B, D - 1], commands int32 [B]); static buffers per tag"""
        if (tag, B) not in self._views:
            self._views[(tag, B)] = (torch.zeros(B, self.embedder_dim, dtype=torch.float32, device=self.device),
                                     torch.zeros(B, dtype=torch.int32, device=self.device))
        x, commands = self._views[(tag, B)]
        self.lib.cil_split_observation(obs, self.obs_dim, B, self.obs_dim, self.class_column, x, self.embedder_dim,
                                       commands, self.networks["main"].ctx.stream)
        return x, commands

    # --------------------------------------------------------------------------------- acting
    def _act_forward(self, states):
        """choose_action :68-70 + extract_action_values :72-73: each row's output of its command's head"""
        x, commands = self._split(states, self.n_env, "act")
        self._values = self.networks["main"].action_values(x, self.n_env, commands)

    def choose_action(self, states):
        self.exploration_policy.phase = RunPhase.TEST              # imitation_agent.py:47, whatever the agent's own phase
        self._run(("act", self.n_env), lambda: self._act_forward(states))
        return self.exploration_policy.get_action(self._values, self.actions)

    def _store_extra_host(self, dones_host, record):
        """the class of the state this step acted on (the memory's current state until store() advances it)"""
        if not record:
            return {}
        v = self.memory.cur_state[:, self.class_column].cpu().numpy()
        if not (np.isfinite(v).all() and (v >= 0).all() and (v == np.trunc(v)).all()):
            raise ValueError("The class index under the key ({}) is not a non-negative integer: {}"
                             .format(self.ap.algorithm.state_key_with_the_class_index, v.tolist()))
        return {"classes_host": v.astype(np.int64)}

    # ------------------------------------------------------------------------------- training
    def _training_phases_due(self):
        """num_consecutive_playing_steps = EnvironmentSteps(0) (CARLA_CIL): every train() call is one training phase
        on what the memory holds; otherwise the off-policy schedule"""
        playing = self.ap.algorithm.num_consecutive_playing_steps
        if isinstance(playing, EnvironmentSteps) and playing.num_steps == 0:
            return 1 if self.memory.num_transitions() > 0 else 0
        return super()._training_phases_due()

    def _learn_device(self, batch, B):
        x, commands = self._split(batch._states["observation"], B, "train")
        self.networks["main"].learn_from_batch(x, B, commands, batch.actions(), grad_scale=self._grad_scale())

    def learn_from_batch(self, batch):
        """CILAgent.learn_from_batch (:75-87); one captured graph per batch size"""
        B = batch.size
        self._run(("cil_learn", B), lambda: self._learn_device(batch, B))
        net = self.networks["main"]
        self.signals = {"Loss": net.loss[0], "Grads (unclipped)": net.norm}
        return net.loss[0]
