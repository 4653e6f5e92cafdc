"""Direct Future Prediction (DFP) on one MI355X — host-side mirror of rl_coach/agents/dfp_agent.py (parameter classes
:37-134, DFPAgent :138-255) and of the MeasurementsPredictionHead
(architectures/tensorflow_components/heads/measurements_prediction_head.py:26-62).  Dosovitskiy & Koltun 2017,
"Learning to Act by Predicting the Future".

Vector observations and discrete actions.  The measurements are the agent's own: with
use_accumulated_reward_as_measurement the running sum of shaped rewards is THE measurement (the device environments
supply none), with the reference's one-step lag (agent.py:920-925 injects the sum before :958 adds the step's reward;
rlx_dfp_accumulated_reward_step).
Per step: the current states, their measurements and the goal -> DFPNet -> rlx_dfp_egreedy (the merge of the two
streams, the fp64 score of every action over the last len(future_measurements_weights) steps, the epsilon-greedy choice).
Per finished episode: the episodic replay writes every transition's future-measurement targets from the episode's own
future (rlx_dfp_future_measurements; NaN or the last state past the end).
Per update: ONE forward pass -> rlx_dfp_head_loss (the targets are the prediction but for the taken action's row; NaN
targets ignored; loss and the gradients of the two stream outputs) -> backward -> TF1 Adam (beta1 0.95).  No target
network.

Not served: image observations (the Doom presets), measurements an environment supplies, goals that change during a
run, shared_memory across workers, ParameterNoise (the noisy dense launch has no leaky_relu)."""
from enum import Enum

import numpy as np
import torch

from .. import _rlx
from ..architectures.head_parameters import MeasurementsPredictionHeadParameters
from ..architectures.layers import scheme_to_native
from ..core_types import EnvironmentSteps
from ..exploration_policies.e_greedy import EGreedyParameters
from ..exploration_policies.parameter_noise import ParameterNoiseParameters
from ..memories.episodic.episodic_experience_replay import (EpisodicExperienceReplay,
                                                            EpisodicExperienceReplayParameters)
from ..memories.memory import MemoryGranularity
from ..nn.networks import DFPNet, dfp_net_kwargs
from .dqn_agent import DQNAgent
from .vector_agent import AlgorithmParameters, VectorOffPolicyAgent


class HandlingTargetsAfterEpisodeEnd(Enum):                     # dfp_agent.py:37-39
    LastStep = 0
    NAN = 1


class _EmbedderRecord(object):
    """input_embedders_parameters[name] of a preset text: `.scheme` (an EmbedderScheme member, its name or a list of
    Dense layers) and `.activation_function`, live views onto the network parameters' per-embedder tables."""

    def __init__(self, owner, name):
        object.__setattr__(self, "_owner", owner)
        object.__setattr__(self, "_name", name)

    @property
    def scheme(self):
        return self._owner.embedder_schemes[self._name]

    @scheme.setter
    def scheme(self, value):
        self._owner.embedder_schemes[self._name] = scheme_to_native(value, False)

    @property
    def activation_function(self):
        return self._owner.embedder_activations[self._name]

    @activation_function.setter
    def activation_function(self, value):
        self._owner.embedder_activations[self._name] = value

    def __setattr__(self, name, value):
        if name in ("scheme", "activation_function"):
            object.__setattr__(self, name, value)
        else:                                                    # dropout_rate, ...: remembered, not used
            self._owner.__dict__.setdefault("_view_extras", {}).setdefault(self._name, {})[name] = value


class _EmptyMiddleware(object):
    """middleware_parameters of DFPNetworkParameters: FCMiddlewareParameters(scheme=MiddlewareScheme.Empty); anything
    else has no device network."""
    activation_function = 'leaky_relu'

    @property
    def scheme(self):
        return "Empty"

    @scheme.setter
    def scheme(self, value):
        if scheme_to_native(value, False) not in ("Empty", []):
            raise ValueError("the DFP network has no middleware (MiddlewareScheme.Empty); got {}".format(value))


class DFPNetworkParameters(object):                              # dfp_agent.py:42-73 + NetworkParameters defaults
    def __init__(self):
        self.embedder_schemes = {"observation": "Medium", "measurements": [128, 128, 128], "goal": [128, 128, 128]}
        self.embedder_activations = {k: 'leaky_relu' for k in self.embedder_schemes}
        self.middleware_parameters = _EmptyMiddleware()
        self.heads_parameters = [MeasurementsPredictionHeadParameters(activation_function='leaky_relu')]
        self.optimizer_type = 'Adam'
        self.async_training = False
        self.batch_size = 64
        self.create_target_network = False
        self.learning_rate = 0.00025
        self.adam_optimizer_beta1 = 0.95
        self.adam_optimizer_beta2 = 0.99
        self.optimizer_epsilon = 0.0001
        self.scale_down_gradients_by_number_of_workers_for_sync_training = True
        self.clip_gradients = None

    @property
    def input_embedders_parameters(self):
        return {k: _EmbedderRecord(self, k) for k in self.embedder_schemes}


class DFPMemoryParameters(EpisodicExperienceReplayParameters):   # dfp_agent.py:76-80
    def __init__(self):
        super().__init__()
        # 20000 transitions: "a very small ER keeping only recent samples" (dfp_agent.py:146).  The reference assigns it
        # (and shared_memory = True) BEFORE its base class's __init__, which puts its own defaults back, so the reference
        # itself runs with a million and no shared memory (tests/golden/dfp.npz records that); the stated size is kept
        # here, and shared_memory across workers is not served
        self.max_size = (MemoryGranularity.Transitions, 20000)
        self.shared_memory = False


class DFPAlgorithmParameters(AlgorithmParameters):              # dfp_agent.py:83-122
    def __init__(self):
        super().__init__()
        self.num_predicted_steps_ahead = 6                       # the steps t + 2^i, i < 6
        self.goal_vector = [1.0, 1.0]
        self.future_measurements_weights = [0.5, 0.5, 1.0]       # the LAST len(...) predicted steps count
        self.use_accumulated_reward_as_measurement = False
        self.handling_targets_after_episode_end = HandlingTargetsAfterEpisodeEnd.NAN
        self.scale_measurements_targets = {}
        self.num_consecutive_playing_steps = EnvironmentSteps(8)


class DFPAgentParameters(object):                                # dfp_agent.py:125-134
    def __init__(self):
        self.algorithm = DFPAlgorithmParameters()
        self.exploration = EGreedyParameters()
        self.memory = DFPMemoryParameters()
        self.network_wrappers = {"main": DFPNetworkParameters()}
        self.seed = 0

    @property
    def path(self):
        return 'coach_amd.agents.dfp_agent:DFPAgent'


class DFPAgent(DQNAgent):
    """On DQNAgent's acting skeleton (host epsilon-greedy draws, the staged choice) with its own network, memory columns,
    acting launch and update."""
    SIGNAL_NAMES = VectorOffPolicyAgent.SIGNAL_NAMES             # (no 'Q': the reference's DFPAgent is a plain Agent)
    parameter_noise = False
    is_on_policy = True                                          # dfp_agent.py:144-148 ("approximately")

    @staticmethod
    def check_parameters(ap, ep):
        """What the agent refuses, before anything touches the device (ap: DFPAgentParameters, ep: the environment's
        parameters) -> (measurement names, scale factors fp64 [M], goal, weights).  The measurements space is agent.py:311-316's,
        the scale factors and their check dfp_agent.py:201-226's."""
        alg = ap.algorithm
        if getattr(ep, "kind", "vector") == "image" or len(tuple(ep.observation_shape)) != 1:
            raise ValueError("DFPAgent: image observations are not served (vector observations only; the Doom presets "
                             "and simulators that supply their own measurements stay out)")
        if getattr(ep, "num_actions", None) is None:
            raise ValueError("DFPAgent: a Box action space is not served (the head predicts per discrete action)")
        if isinstance(ap.exploration, ParameterNoiseParameters):
            raise ValueError("DFPAgent: ParameterNoise is not served (the noisy dense launch has no leaky_relu)")
        names = list(getattr(ep, "measurements_names", None) or [])
        if names:
            raise ValueError("DFPAgent: measurements supplied by the environment are not served")
        if alg.use_accumulated_reward_as_measurement:
            names.append('accumulated_reward')
        if not names:
            raise ValueError("Measurements are not present: the environment supplies none, so "
                             "use_accumulated_reward_as_measurement must be set")
        scales = alg.scale_measurements_targets
        if set(names).intersection(scales.keys()) != set(scales.keys()):
            raise ValueError("Some of the keys in parameter scale_measurements_targets ({})  are not defined in "
                             "the measurements space {}".format(scales.keys(), names))
        factors = np.array([scales.get(n, 1) for n in names], dtype=np.float64)
        goal = [float(g) for g in alg.goal_vector]
        if len(goal) != len(names):
            raise ValueError("the goal vector {} weights {} values, the measurements are {}"
                             .format(alg.goal_vector, len(goal), names))
        weights = [float(w) for w in alg.future_measurements_weights]
        if not 1 <= len(weights) <= int(alg.num_predicted_steps_ahead):
            raise ValueError("future_measurements_weights weights the last {} of {} predicted steps"
                             .format(len(weights), alg.num_predicted_steps_ahead))
        if not isinstance(alg.handling_targets_after_episode_end, HandlingTargetsAfterEpisodeEnd):
            raise ValueError("handling_targets_after_episode_end is a HandlingTargetsAfterEpisodeEnd")
        if not isinstance(ap.memory, EpisodicExperienceReplayParameters):
            raise ValueError("DFPAgent: the targets come from an episode's own future, so the memory is an "
                             "EpisodicExperienceReplay")
        if getattr(ap.memory, "shared_memory", False):
            raise ValueError("DFPAgent: shared_memory across workers is not served")
        return names, factors, goal, weights

    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        names, factors, goal, weights = self.check_parameters(agent_parameters, environment.p)
        VectorOffPolicyAgent.__init__(self, agent_parameters, environment, device, dist, use_graphs)
        ep, net, alg = environment.p, self.ap.network_wrappers["main"], self.ap.algorithm
        self.A = int(ep.num_actions)
        self.batch_size = net.batch_size
        self.measurements_names, self.M = names, len(names)
        self.target_measurements_scale_factors, self.current_goal = factors, goal
        self.S = int(alg.num_predicted_steps_ahead)
        dev, n = self.device, self.n_env
        self.goal_dev = torch.tensor(self.current_goal, dtype=torch.float64, device=dev)
        self.weights_dev = torch.tensor(weights, dtype=torch.float64, device=dev)
        self._goal_rows_cache = {}
        self.networks = {"main": DFPNet(dev, int(ep.observation_shape[0]), self.M, self.A, self.S,
                                        **dfp_net_kwargs(net, self.ap.seed or 0))}
        self.memory = self._make_memory()
        self.exploration_policy = self._make_exploration_policy()
        self.actions = torch.zeros(n, dtype=torch.int32, device=dev)
        self.td_errors = None
        # the running sum of shaped rewards per env, the CURRENT states' measurements (fp64 and the network's fp32 twin)
        # and the measurements of the states the last step was taken in (what the replay stores)
        self.accumulated_reward = torch.zeros(n, dtype=torch.float64, device=dev)
        self.cur_measurements = torch.zeros(n, self.M, dtype=torch.float64, device=dev)
        self.cur_measurements32 = torch.zeros(n, self.M, dtype=torch.float32, device=dev)
        self._state_measurements = torch.zeros(n, self.M, dtype=torch.float64, device=dev)
        self._finish_init()

    def _make_memory(self, action_dim=None):
        mp, ep, alg = self.ap.memory, self.env.p, self.ap.algorithm
        last = alg.handling_targets_after_episode_end == HandlingTargetsAfterEpisodeEnd.LastStep
        return EpisodicExperienceReplay(
            mp.max_size, mp.allow_duplicates_in_batch_sampling, n_step=getattr(mp, "n_step", -1), discount=alg.discount,
            max_episode_length=self.L, measurements_dim=self.M,
            future_measurements=(self.S, self.target_measurements_scale_factors, last), device=self.device,
            n_env=self.n_env, observation_shape=ep.observation_shape, stack=None, action_dim=None,
            min_episode_length=getattr(ep, "min_episode_length", self.L))

    def _step_graph_ok(self):
        return False                                   # (DQN's one-record step is the uniform replay's)

    # -------------------------------------------------------------------- the accumulated reward
    def _restart_measurements(self):
        """reset_internal_state (agent.py:614): every env starts an episode, its sum and its first state's measurement 0"""
        self.accumulated_reward.zero_()
        self.cur_measurements.zero_()
        self.cur_measurements32.zero_()

    def reset_internal_state(self):
        first = super().reset_internal_state()
        self._restart_measurements()
        return first

    def evaluate_episodes(self, episodes_per_env=1):
        try:
            return super().evaluate_episodes(episodes_per_env)
        finally:
            self._restart_measurements()               # training resumes from a fresh reset

    def _stored_game_over(self, game_over):
        self._step_game_over = game_over
        return game_over

    def _store_extra_host(self, dones_host, record):
        """after the reward filter, before the rows are written: the stored states' measurements, the next states' and
        the sums (one launch); evaluation steps advance them too (the network reads them), but store nothing."""
        self.lib.dfp_accumulated_reward_step(self.filtered_reward, self._step_game_over, self.accumulated_reward,
                                             self.cur_measurements, self.cur_measurements32,
                                             self._state_measurements if record else None, self.n_env, self.M,
                                             self.M - 1, _rlx.current_stream())
        return {"measurements": self._state_measurements} if record else {}

    # --------------------------------------------------------------------------------- acting
    def _goal_rows(self, rows):
        """np.repeat(np.expand_dims(current_goal, 0), rows, axis=0) as a static fp32 device buffer"""
        g = self._goal_rows_cache.get(rows)
        if g is None:
            g = self._goal_rows_cache[rows] = torch.tensor([self.current_goal] * rows, dtype=torch.float32,
                                                           device=self.device)
        return g

    def _q_buf(self):
        """the fp64 action values of the last acting step [n_env, A], written by the acting launch."""
        if getattr(self, "_q_act", None) is None:
            self._q_act = torch.zeros(self.n_env, self.A, dtype=torch.float64, device=self.device)
        return self._q_act

    def _q_forward(self, states):
        ins = {"observation": states, "measurements": self.cur_measurements32, "goal": self._goal_rows(self.n_env)}
        self._streams_act = self.networks["main"].streams(ins, self.n_env, tag="act")

    def choose_action(self, states):
        """DFPAgent.choose_action (dfp_agent.py:169-199): one forward pass on the current states, then the acting launch."""
        pol = self.exploration_policy
        pol.phase = self.phase
        draws = pol.draw()                                           # host RNG, per env, in order
        self._goal_rows(self.n_env)                                  # (allocated outside a capture)
        self._run(("q", self.n_env), lambda: self._q_forward(states))
        eps, d = pol.stage(draws)
        self._select_actions(d["u"], d["ra"], d["tie"], eps)
        return self.actions

    def _select_actions(self, u, ra, tie, eps):
        net = self.networks["main"]
        e, x = self._streams_act
        self.lib.dfp_egreedy(e, net.K, x, net.A * net.K, self.goal_dev, self.weights_dev, self.S, self.M,
                             self.weights_dev.numel(), u, ra, tie, float(eps), self.n_env, self.A, self._q_buf(),
                             self.actions, _rlx.current_stream())

    # ------------------------------------------------------------------------------- training
    def _learn_device(self, b, weights=None, per_ride=None):
        B = self.batch_size
        ins = {"observation": b._states["observation"], "measurements": b._states["measurements"],
               "goal": self._goal_rows(B)}
        self.networks["main"].learn_from_batch(ins, B, b.actions(), b.info("future_measurements"),
                                               grad_scale=self._grad_scale(), sync=self if self.dist is not None else None)

    def learn_from_batch(self, batch):
        """DFPAgent.learn_from_batch (dfp_agent.py:150-167)."""
        self._goal_rows(self.batch_size)
        self._run(("learn",), lambda: self._learn_device(batch))
        return self._loss_signals()
