"""The imitation agents' base — host-side mirror of rl_coach/agents/imitation_agent.py (ImitationAgent :29-69).

An imitation agent fits the logged actions of a dataset instead of maximising a return; it is off-policy and sets
``imitation = True``.  Acting is the network's prediction (the action probabilities) followed by the exploration
policy, which choose_action FORCES into RunPhase.TEST at every call (:47) — so it is evaluation_epsilon that applies,
also while the agent trains, and the epsilon schedule is never stepped.  On the device that is the DQN family's acting
loop with probabilities in the place of Q values: the host draws of EGreedy in the reference's order, rlx_egreedy over
the probabilities.  learn_from_batch is abstract here, with the reference's text; BCAgent (bc_agent.py) is the subclass.

Served: vector observations, discrete actions, one GPU.  Refused by name before anything touches the device: image
observations, box action spaces, the ParameterNoise exploration policy, data-parallel training.
"""
import torch

from ..core_types import RunPhase
from ..exploration_policies.e_greedy import EGreedy
from ..exploration_policies.parameter_noise import ParameterNoiseParameters, network_is_noisy
from .dqn_agent import DQNAgent, check_load_memory_from_file_path
from .vector_agent import VectorOffPolicyAgent


class ImitationAgent(DQNAgent):
    """What the DQN family's stepping machinery needs from an imitation agent: `_build_network(obs_shape, wrapper)` and
    `_predict(states, n)` -> device fp32 [n, A] action probabilities."""
    imitation = True
    is_on_policy = False
    SIGNAL_NAMES = VectorOffPolicyAgent.SIGNAL_NAMES

    def __init__(self, agent_parameters, environment, device=None, dist=None, use_graphs=None):
        ap, ep, name = agent_parameters, environment.p, type(self).__name__
        if dist is not None and getattr(dist, "enabled", True):
            raise ValueError("data-parallel training is not served by %s" % name)
        if getattr(ep, "kind", "vector") == "image":
            raise ValueError("%s serves vector observations, not image observations" % name)
        if getattr(ep, "action_dim", None) is not None or not getattr(ep, "num_actions", None):
            raise ValueError("%s serves discrete action spaces, not a Box action space (the continuous PolicyHead is "
                             "not served)" % name)
        if isinstance(ap.exploration, ParameterNoiseParameters) or network_is_noisy(ap.network_wrappers["main"]):
            raise ValueError("the ParameterNoise exploration policy (noisy dense layers) is not implemented for %s" % name)
        dataset = check_load_memory_from_file_path(ap)
        VectorOffPolicyAgent.__init__(self, ap, environment, device, None, use_graphs)
        self.parameter_noise = False
        net = self.ap.network_wrappers["main"]
        self.A = int(ep.num_actions)
        self.batch_size = net.batch_size
        self.networks = {"main": self._build_network(tuple(ep.observation_shape), net)}
        self.memory = self._make_memory(action_dim=None)
        self.exploration_policy = EGreedy(self.A, self.n_env, self.device, self.ap.exploration)
        self.actions = torch.zeros(self.n_env, dtype=torch.int32, device=self.device)
        self.td_errors = None
        self._finish_init()
        if dataset is not None:                        # agent.py:262-263: the memory starts as the file
            self.load_memory_from_file()

    def _build_network(self, obs_shape, wrapper):
        raise NotImplementedError

    def _predict(self, states, n):
        raise NotImplementedError

    def _step_graph_ok(self):
        return False

    def _has_td_errors(self):
        return False

    # --------------------------------------------------------------------------------- acting
    def _q_forward(self, states):
        """extract_action_values(prediction) (:38-39): the action values ARE the predicted probabilities"""
        self._q_act = self._predict(states, self.n_env)

    def choose_action(self, states):
        self.exploration_policy.phase = RunPhase.TEST              # :47, whatever the agent's own phase
        draws = self.exploration_policy.draw()                     # host RNG, per env, in order
        self._run(("predict", self.n_env), lambda: self._q_forward(states))
        eps, d = self.exploration_policy.stage(draws)
        self._select_actions(d["u"], d["ra"], d["tie"], eps)
        return self.actions

    # ------------------------------------------------------------------------------- training
    def learn_from_batch(self, batch):
        raise NotImplementedError("ImitationAgent is an abstract agent. Not to be used directly.")
