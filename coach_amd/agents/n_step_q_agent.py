"""N-step Q on one MI355X — host-side mirror of rl_coach/agents/n_step_q_agent.py (parameter classes :34-84,
NStepQAgent :88-153) over the on-policy base (agents/policy_optimization_agent.py): a Q head with a target network,
trained from t_max windows of the running episode.

Per vector step: states -> the online network's Q values -> rlx_egreedy on the staged host draws (the DQN agent's
acting; in the reference choose_action is ValueOptimizationAgent's, so there are no 'Entropy' samples) -> env.step ->
reward filter -> the env's episode row, with its game-over byte and the observation before the reset.
Per train() call: first the target-copy check of the off-policy agents (_should_update_online_weights_to_target,
:142-153), then the base's train(): gate, window, pointer, accumulation and apply cadence are untouched.
Per update window: the online network forward on the window's T states, the TARGET network forward on the state behind
the window ('N-Step': one row) or on the T next states ('1-Step'; in place while the episode runs, the last one staged
from the observation before the reset behind a finished episode); ONE launch, rlx_nstep_q_window_loss
(csrc/n_step_q.hip), restates learn_from_batch :99-140 — R = 0 on a game over or the target row's maximum, the reverse
recurrence or the per-row 1-step target in the reference's order and rounding, the Q head's loss on the taken action
and its gradient; backward; accumulated += gradients.  The target rows are always forwarded: whether the last
transition is a game over is a device fact the launch reads.  The target network's values do not leave the device.
"""
import torch

from .. import _rlx
from ..architectures.head_parameters import QHeadParameters
from ..architectures.scheme_views import SchemeViews
from ..core_types import EnvironmentSteps, RunPhase
from ..exploration_policies.e_greedy import EGreedy, EGreedyParameters
from ..memories.episodic.single_episode_buffer import SingleEpisodeBufferParameters
from ..nn.networks import NStepQNet, n_step_q_net_kwargs
from .policy_optimization_agent import PolicyOptimizationAgent
from .vector_agent import AlgorithmParameters


class NStepQNetworkParameters(SchemeViews):              # n_step_q_agent.py:34-43 + NetworkParameters defaults
    def __init__(self):
        self.activation_function = 'relu'
        self.embedder_scheme = 'Medium'
        self.middleware_scheme = 'Medium'
        self.heads_parameters = [QHeadParameters()]
        self.optimizer_type = 'Adam'
        self.async_training = True
        self.shared_optimizer = True
        self.create_target_network = True
        self.batch_size = 32
        self.replace_mse_with_huber_loss = False
        self.learning_rate = 0.00025
        self.adam_optimizer_beta1 = 0.9
        self.adam_optimizer_beta2 = 0.99
        self.optimizer_epsilon = 0.0001
        self.scale_down_gradients_by_number_of_workers_for_sync_training = True
        self.clip_gradients = None                       # ClipByGlobalNorm threshold (base_parameters.py)


class NStepQAlgorithmParameters(AlgorithmParameters):    # n_step_q_agent.py:46-72
    def __init__(self):
        super().__init__()
        self.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(10000)
        self.apply_gradients_every_x_episodes = 1
        self.num_steps_between_gradient_updates = 5      # this is called t_max in all the papers
        self.targets_horizon = 'N-Step'


class NStepQAgentParameters(object):                     # n_step_q_agent.py:75-84
    def __init__(self):
        self.algorithm = NStepQAlgorithmParameters()
        self.exploration = EGreedyParameters()
        self.memory = SingleEpisodeBufferParameters()
        self.network_wrappers = {"main": NStepQNetworkParameters()}
        self.seed = 0

    @property
    def path(self):
        return 'coach_amd.agents.n_step_q_agent:NStepQAgent'


class NStepQAgent(PolicyOptimizationAgent):
    # the reference's registration order: PolicyOptimizationAgent's 'Entropy' (never sampled here),
    # ValueOptimizationAgent's 'Q', then :92-93
    SIGNAL_NAMES = PolicyOptimizationAgent.SIGNAL_NAMES + ["Q", "Q Values", "Value Loss"]

    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        horizon = agent_parameters.algorithm.targets_horizon
        if horizon not in _rlx.NSTEPQ_HORIZON:
            # the reference's `assert True, ...` (:128) lets an unknown horizon through and trains on the online
            # prediction itself; here the launch has no such branch
            raise ValueError("The available values for targets_horizon are: {} (got {!r})"
                             .format(", ".join(sorted(_rlx.NSTEPQ_HORIZON)), horizon))
        self.horizon = _rlx.NSTEPQ_HORIZON[horizon]
        super().__init__(agent_parameters, environment, device, dist, use_graphs)
        dev, L = self.device, self.L
        self.targets = torch.zeros(L, dtype=torch.float32, device=dev)           # the taken actions' targets of the window
        self.returns = torch.zeros(L, dtype=torch.float64, device=dev)           # a finished episode's discounted returns
        self.target_copies = 0           # how often train() copied the online weights to the target network
        self.debug_targets = None        # tests set this to a list: (Q, target Q, targets, game over) clones per window

    @property
    def is_on_policy(self):
        return False                                     # :95-97

    def _make_network(self, obs_shape, wrapper):
        return NStepQNet(self.device, obs_shape, self.A, **n_step_q_net_kwargs(wrapper, self.ap.seed or 0))

    def _make_exploration_policy(self):
        return EGreedy(self.A, self.n_env, self.device, self.ap.exploration)

    # --------------------------------------------------------------------------------- acting
    def _act_device(self, states, draws):
        q = self.networks["main"].q_values(states, self.n_env, tag="act")
        eps, d = draws
        self.lib.egreedy(q.data, self.A, d["u"], d["ra"], d["tie"], float(eps), self.n_env, self.A, self.actions,
                         _rlx.current_stream())

    def choose_action(self, states):
        pol = self.exploration_policy
        pol.phase = self.phase
        staged = pol.stage(pol.draw())                               # host RNG, per env, in order
        self._run(("act", states.data_ptr()), lambda: self._act_device(states, staged))
        return self.actions

    # ------------------------------------------------------------------------------- training
    def train(self):
        """:142-153: the target-copy check, then PolicyOptimizationAgent.train"""
        if self.phase == RunPhase.TRAIN and self._should_update_online_weights_to_target():
            self.update_target_networks(self.ap.algorithm.rate_for_copying_weights_to_target)
            self._target_updated_since_log = True                    # the 'Update Target Network' column
            self.target_copies += 1
        return super().train()

    def _window_device(self, env, start, end, complete):
        """learn_from_batch (:99-140) on steps [start, end) of env's episode"""
        alg, net, T = self.ap.algorithm, self.networks["main"], end - start
        obs, actions, rewards = self.memory.episode_rows(env, start, end)
        rows, last_next_state, game_over = self.memory.bootstrap_rows(env, start, end, complete)
        if self.horizon == _rlx.NSTEPQ_HORIZON["N-Step"]:
            target_obs, rows_t = last_next_state.view(1, -1), 1      # last_sample(batch.next_states) (:121)
        elif rows is not None:
            target_obs, rows_t = rows[1:], T                         # the T next states, in place
        else:                                                        # the reset overwrote the state behind the episode
            target_obs, rows_t = net.stage_rows(obs[1:], last_next_state), T
        loss = net.accumulate_window(obs, T, actions, self.targets, target_obs, rows_t, rewards[start:end], game_over,
                                     alg.discount, self.horizon)
        self.signals = {"Loss": net.loss, "Grads (unclipped)": net.norm, "Q Values": net.td_targets.view(-1),
                        "Value Loss": net.loss}
        if complete:                                     # handle_episode_ended: a sample per transition (agent.py:569-570)
            self.lib.episode_nstep_returns(rewards, None, self.returns, 0, end, 0, 1, end, float(alg.discount), -1,
                                           _rlx.current_stream())
            self.signals["Discounted Return"] = self.returns[:end]
        if self.debug_targets is not None:
            self.debug_targets.append((net.q_online.clone(), net.q_target.clone(), self.targets[:T].clone(),
                                       actions.clone(), game_over.clone()))
        return loss

    def check_status(self):
        super().check_status()
        self.networks["main"].check_status()
