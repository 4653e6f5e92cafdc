"""Persistent Advantage Learning (PAL) on one MI355X — host-side mirror of rl_coach/agents/pal_agent.py (parameter
classes :26-55, PALAgent.learn_from_batch :70-111).  Bellemare et al. 2016, https://arxiv.org/abs/1512.04860.

A DQN-family agent whose TD target is the Double-DQN target minus alpha times the action gap of the target network —
max Q_target(s) - Q_target(s, a), or in the persistent form the smaller of it and the gap at s' — mixed at rate
monte_carlo_mixing_rate with the transition's Monte Carlo return (the episodic replay's n_step_discounted_rewards
column, n_step = -1: the discounted return to the episode's end).
Per step: DQN's acting (online Q values, epsilon-greedy).
Per update: online(s') (the selector), target(s), target(s'), online(s) -> rlx_mixed_target_head_loss (targets, loss,
dQ: csrc/pal.hip) -> backward -> TF1 Adam.

MixedTargetDQNAgent is the part PALAgent shares with MixedMonteCarloAgent (mmc_agent.py): the network, the memory's
type, what an update passes to the launch.
"""
from ..exploration_policies.parameter_noise import ParameterNoiseParameters, network_is_noisy
from ..memories.episodic.episodic_experience_replay import EpisodicExperienceReplay, EpisodicExperienceReplayParameters
from ..nn.networks import MixedTargetDQNNet
from .dqn_agent import DQNAgent, DQNAgentParameters, DQNAlgorithmParameters


class PALAlgorithmParameters(DQNAlgorithmParameters):                    # pal_agent.py:26-44
    def __init__(self):
        super().__init__()
        self.pal_alpha = 0.9
        self.persistent_advantage_learning = False
        self.monte_carlo_mixing_rate = 0.1


class PALAgentParameters(DQNAgentParameters):                            # pal_agent.py:47-55
    def __init__(self):
        super().__init__()
        self.algorithm = PALAlgorithmParameters()
        self.memory = EpisodicExperienceReplayParameters()

    @property
    def path(self):
        return 'coach_amd.agents.pal_agent:PALAgent'


class MixedTargetDQNAgent(DQNAgent):
    MODE = None              # MixedTargetDQNNet.learn_from_batch's mode

    NET = MixedTargetDQNNet

    def _check_parameters(self):
        name = type(self).__name__
        if isinstance(self.ap.exploration, ParameterNoiseParameters) or \
                network_is_noisy(self.ap.network_wrappers["main"]):
            raise ValueError("the ParameterNoise exploration policy (noisy dense layers) is not implemented for %s"
                             % name)
        if not isinstance(self.ap.memory, EpisodicExperienceReplayParameters):
            raise ValueError("%s mixes the Monte Carlo return into its targets, and only the episodic replay computes "
                             "one (n_step_discounted_rewards): use EpisodicExperienceReplayParameters, not %s"
                             % (name, type(self.ap.memory).__name__))
        from ..memories.episodic.episodic_hindsight_experience_replay import EpisodicHindsightExperienceReplayParameters
        if isinstance(self.ap.memory, EpisodicHindsightExperienceReplayParameters):
            raise ValueError("%s reads the transitions' Monte Carlo returns (n_step_discounted_rewards), which the "
                             "hindsight replay does not provide: use EpisodicExperienceReplayParameters" % name)
        self.parameter_noise = False

    def _check_memory(self):                                        # (image observations: refused by the memory)
        assert isinstance(self.memory, EpisodicExperienceReplay)

    def _has_td_errors(self):
        return False

    def _step_graph_ok(self):
        """the one-graph-per-env-step path of DQNAgent is declined: it draws from the flat replay and its update is
        DQN's"""
        return False

    def _target_parameters(self):
        """-> (pal_alpha, persistent, mixing_rate) of the launch"""
        raise NotImplementedError

    def _learn_device(self, b, weights=None, per_ride=None):
        alpha, persistent, rate = self._target_parameters()
        self.networks["main"].learn_from_batch(
            b._states["observation"], b._next_states["observation"], self.batch_size, b.actions(), b.rewards(),
            b.game_overs(), b.info("n_step_discounted_rewards"), self.ap.algorithm.discount, pal_alpha=alpha,
            persistent=persistent, mixing_rate=rate, mode=self.MODE, grad_scale=self._grad_scale(),
            sync=self if self.dist is not None else None, states_pair=b._info.get("states_pair"))


class PALAgent(MixedTargetDQNAgent):
    MODE = "pal"

    def _target_parameters(self):
        alg = self.ap.algorithm
        return alg.pal_alpha, alg.persistent_advantage_learning, alg.monte_carlo_mixing_rate
