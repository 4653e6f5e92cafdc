"""Rainbow DQN on one MI355X — host-side mirror of rl_coach/agents/rainbow_dqn_agent.py (parameter classes :32-72,
RainbowDQNAgent :84-137) and of the RainbowQHead (architectures/tensorflow_components/heads/rainbow_q_head.py:25-70).

The import layer (coach_amd.compat) serves the reference's module path rl_coach.agents.rainbow_dqn_agent from this module;
coach_amd/agents/rainbow_dqn_agent.py keeps the refusing class that existing tests pin.

The six ingredients and where they live here:
  1. NoisyNets          ParameterNoise (the default exploration): every dense layer is an nn.graph.NoisyDense
  2. C51                the support, softmax, expectations and projection of csrc/categorical_head.hpp
  3. Prioritized ER     memories/non_episodic/nstep_prioritized_experience_replay.py over csrc/sumtree.hip
  4. Double DQN         the online network on s' picks the action whose target distribution is projected
  5. Dueling            the head's two streams, merged per atom
  6. n-step returns     whole episodes reach the replay when they end, next states redirected n steps ahead
                        (csrc/nstep_store.hip)
Per step: the online network's two stream outputs -> rlx_rainbow_argmax (ParameterNoise: the first maximum of the fp64
expectations, no host draw) or rlx_rainbow_egreedy (an EGreedy policy over a plain network).
Per update: online(s'), target(s'), online(s) -> rlx_rainbow_head_loss -> backward through both streams -> TF1 Adam.  The
projection shifts the support by n_step_discounted_rewards and scales it by discount ** n_step where
should_bootstrap_next_state is set; game_over is not read.  As for C51 the head's loss_type is empty, so the importance
weights are read and have no effect; the new priorities are the taken action's cross entropy (:133-135).

Refused: n_step < 2 (the reference never sets should_bootstrap_next_state then and fails with a KeyError in
learn_from_batch), a memory other than the n-step prioritized replay, image observations (the n-step next state in the
frame-dedup ring is not built: Atari_Rainbow builds its parameters, not its agent).
"""
from .. import _rlx
from ..architectures.head_parameters import RainbowQHeadParameters
from ..exploration_policies.parameter_noise import ParameterNoiseParameters
from ..memories.non_episodic.nstep_prioritized_experience_replay import NStepPrioritizedExperienceReplay
from ..memories.non_episodic.prioritized_experience_replay import PrioritizedExperienceReplayParameters
from ..nn.networks import RainbowNet
from .categorical_dqn_agent import (CategoricalDQNAgent, CategoricalDQNAgentParameters,
                                    CategoricalDQNAlgorithmParameters)
from .dqn_agent import DQNNetworkParameters


class RainbowDQNNetworkParameters(DQNNetworkParameters):                # rainbow_dqn_agent.py:32-36
    def __init__(self):
        super().__init__()
        self.heads_parameters = [RainbowQHeadParameters()]
        self.middleware_scheme = 'Empty'


class RainbowDQNAlgorithmParameters(CategoricalDQNAlgorithmParameters):   # rainbow_dqn_agent.py:39-56
    def __init__(self):
        super().__init__()
        self.n_step = 3                  # rewards summed before the target bootstraps from the network's prediction
        # an episode's transitions reach the memory when it ends, after the n-step processing of the whole episode
        self.store_transitions_only_when_episodes_are_terminated = True


class RainbowDQNAgentParameters(CategoricalDQNAgentParameters):           # rainbow_dqn_agent.py:59-72
    def __init__(self):
        super().__init__()
        self.algorithm = RainbowDQNAlgorithmParameters()
        # ParameterNoiseParameters marks the network wrappers: they are set first
        self.network_wrappers = {"main": RainbowDQNNetworkParameters()}
        self.exploration = ParameterNoiseParameters(self)
        self.memory = PrioritizedExperienceReplayParameters()

    @property
    def path(self):
        return 'coach_amd.agents.rainbow_agent:RainbowDQNAgent'


class RainbowDQNAgent(CategoricalDQNAgent):
    NET = RainbowNet              # (its loss kernel's per-row error: the taken action's cross entropy)

    def _check_parameters(self):
        super()._check_parameters()
        alg = self.ap.algorithm
        if self.image:
            raise ValueError("Rainbow DQN on image observations is not built: n-step next states in the frame-dedup "
                             "ring are not built")
        if not isinstance(alg.n_step, int) or alg.n_step < 2:
            raise ValueError("Rainbow DQN needs n_step >= 2 (got %r): with n_step = 1 the reference never sets "
                             "should_bootstrap_next_state and its learn_from_batch fails with a KeyError" % (alg.n_step,))

    def _check_memory(self):
        super()._check_memory()
        if not isinstance(self.memory, NStepPrioritizedExperienceReplay):
            raise ValueError("Rainbow DQN needs the n-step prioritized replay (PrioritizedExperienceReplayParameters "
                             "with algorithm.store_transitions_only_when_episodes_are_terminated), not %s"
                             % type(self.memory).__name__)

    # --------------------------------------------------------------------------------- acting
    def _q_forward(self, states):
        v, x = self.networks["main"].head_streams(states, self.n_env, tag="act")
        self._head_v, self._head_x = v.data.view(self.n_env, self.N), x.data.view(self.n_env, self.A * self.N)

    def _select_actions(self, u, ra, tie, eps):
        self.lib.rainbow_egreedy(self._head_v, self.N, self._head_x, self.A * self.N, self.networks["main"].z, self.N,
                                 u, ra, tie, float(eps), self.n_env, self.A, self._q_buf(), self.actions,
                                 _rlx.current_stream())

    def _argmax_actions(self):
        self.lib.rainbow_argmax(self._head_v, self.N, self._head_x, self.A * self.N, self.networks["main"].z, self.N,
                                self.n_env, self.A, self._q_buf(), self.actions, _rlx.current_stream())

    # ------------------------------------------------------------------------------- training
    def _learn_device(self, b, weights, per_ride=None):
        alg = self.ap.algorithm
        self.networks["main"].learn_from_batch(
            b._states["observation"], b._next_states["observation"], self.batch_size, b.actions(),
            b.info("n_step_discounted_rewards"), b.info("should_bootstrap_next_state"), alg.discount ** alg.n_step,
            grad_scale=self._grad_scale(), sync=self if self.dist is not None else None, per_errors=self.td_errors)
