"""`Architecture` on librlx for the two network families of the BASELINE configs C1-C3, i.e. what
GeneralTensorFlowNetwork builds (architectures/tensorflow_components/general_network.py:228-405) behind
the calls of architecture.py:26-237 and tensorflow_components/architecture.py:312-385, 469-521, 598-607:
  * DQN / DDQN: embedder -> FC middleware -> QHead or DuelingQHead, MSE / Huber regression against
    explicit [B, A] targets (`DQNNetworkParameters`);
  * Clipped PPO: two separate embedder + middleware copies, head 0 = VHead, head 1 = PPOHead, fed the way
    ClippedPPOAgent.train_network feeds it (clipped_ppo_agent.py:226-266): inputs 'observation',
    'output_1_0' = actions, 'output_1_1' [, 'output_1_2'] = old policy distribution, the last
    'output_1_n' = clip_param_rescaler; targets [value targets, advantages]; additional_fetches taken
    from `online_network.output_heads[1]` (`ClippedPPONetworkParameters`);
  * DDPG / TD3 actor (`*ActorNetworkParameters`): predict -> actions; predict(outputs=
    weighted_gradients[0], initial_feed_dict={gradients_weights_ph[0]: w}) -> d sum(actions * w)/d theta
    (ddpg_agent.py:183-193);
  * DDPG / TD3 critic (`*CriticNetworkParameters`, inputs 'observation' + 'action'): predict ->
    [Q, mean Q] or [Q1, Q2, min(Q1, Q2), mean Q1]; predict(outputs=gradients_wrt_inputs[k]['action']) with
    k = the mean output -> d mean(Q1)/d action (ddpg_agent.py:169-173, td3_agent.py:194-198);
    accumulate_gradients(inputs, TD targets) for the loss sum_i mean((y - Q_i)^2);
  * SAC (soft_actor_critic_agent.py:168-280): the policy network (`SACPolicyNetworkParameters`: predict ->
    [mu, log_std, raw actions, actions, logprob, mean logprob] with a FRESH noise draw per call, like
    every sess.run of the TF graph; weighted_gradients[5] / [3] with gradients_weights_ph[5] / [3]), the
    twin-Q network (`SACCriticNetworkParameters`, inputs 'observation' + 'output_0_0': predict ->
    [min(Q1, Q2), its mean], outputs=[q_head.q1_output, q_head.q2_output],
    gradients_wrt_inputs[1]['output_0_0'], train_on_batch with q1_loss / q2_loss fetches) and the value
    network (`SACValueNetworkParameters`).  Gradients of the policy network are handed out as a list of
    per-variable tensors, because the agent text combines them variable by variable;
  * Policy Gradients (`PolicyGradientNetworkParameters`): embedder -> FC middleware -> discrete PolicyHead, fed the way
    PolicyGradientsAgent.learn_from_batch feeds it (policy_gradients_agent.py:128-130): inputs 'observation' and
    'output_0_0' = actions, targets = the rescaled returns; predict -> the action probabilities;
  * Actor-Critic (`ActorCriticNetworkParameters`): embedder -> FC middleware -> VHead + discrete PolicyHead, fed the way
    ActorCriticAgent.learn_from_batch feeds it (actor_critic_agent.py:175-177): inputs 'observation' and 'output_1_0' =
    actions, targets = [value targets, advantages]; predict -> [V, the action probabilities];
  * N-step Q (`NStepQNetworkParameters`): embedder -> FC middleware -> QHead with a target copy, fed the way
    NStepQAgent.learn_from_batch feeds it (n_step_q_agent.py:134): targets = [the full target matrix]; predict -> Q;
  * ACER (`ACERNetworkParameters`): embedder -> FC middleware -> QHead + ACERPolicyHead with a target copy (the average
    policy network), fed the way ACERAgent._learn_from_batch feeds it (acer_agent.py:157-165): 'output_1_0' ...
    'output_1_5' and targets = [the aliased Q matrix, the state values]; predict -> [Q, the action probabilities].

One device network (`coach_amd.nn.networks.DQNNet`) holds the online and the target weights in one
allocation; the `…/online` and `…/target` HipArchitecture objects of a NetworkWrapper are two views of
it.  Inputs are numpy arrays (or device tensors) owned by the caller, outputs fresh numpy arrays, as in
the reference; `get_weights()` hands out a backend-native handle that is only good for `set_weights`
of a sibling network (network_wrapper.py:109-125).  `accumulated_gradients` is one flat device buffer
instead of a list of per-variable arrays.
"""
import numpy as np
import torch

from .. import _rlx
from ..nn.actor_critic_nets import ActorNet, CriticNet, SACPolicyNet, SACQNet, SACValueNet
from ..nn.networks import (ACERNet, ActorCriticNet, ClippedPPONet, DFPNet, DQNNet, NStepQNet, PPOActorNet, PPOCriticNet,
                           PolicyGradientNet,
                           acer_net_kwargs, actor_critic_net_kwargs, common_net_kwargs, dfp_net_kwargs, dqn_net_kwargs,
                           n_step_q_net_kwargs, policy_gradient_net_kwargs)
from .architecture import Architecture


def squeeze_list(var):
    """utils.py squeeze_list: a one-element list is returned as its element."""
    return var[0] if isinstance(var, (list, tuple)) and len(var) == 1 else var


class _HeadFetches(object):
    """`online_network.output_heads[i].<name>`: the handles agents put into additional_fetches."""

    def __init__(self, head_idx, names):
        for n in names:
            setattr(self, n, "output_heads/%d/%s" % (head_idx, n))


def _adam_args(np_):
    return (np_.learning_rate, np_.adam_optimizer_beta1, np_.adam_optimizer_beta2, np_.optimizer_epsilon)


def _obs_shape(spaces):
    return tuple(int(x) for x in spaces.state['observation'].shape)


def _discrete_actions(spaces, refusal):
    """the number of actions of a discrete action space; any other space is refused with the family's own text"""
    if not hasattr(spaces.action, "actions"):
        raise ValueError(refusal)
    return len(spaces.action.actions)


def _fetched(table, additional_fetches):
    """table: {fetch handle: a function that returns its value} -> the values of additional_fetches, in their order"""
    if any(f not in table for f in additional_fetches):
        raise ValueError("unknown fetch in {}".format(additional_fetches))
    return [table[f]() for f in additional_fetches]


def _with_entropy_regulariser(losses, net, mean_entropy):
    """the heads' losses and, where beta_entropy is set, the regulariser as a loss of its own (policy_head.py:77-79,
    acer_policy_head.py:56-58)"""
    if net.beta_entropy:
        losses.append(float(-np.float32(net.beta_entropy) * mean_entropy))
    return losses


class HipArchitecture(Architecture):
    """Common part of every network family: device plumbing, the online / target views of one device
    network, gradient accumulation and application, weights, variables, savers.  `construct` picks
    the family from the class of the network parameters (the role `GeneralTensorFlowNetwork` plays for
    the TF backend); the families below add what their heads need."""

    inputs = ['observation']

    @staticmethod
    def construct(variable_scope, devices, *args, **kwargs):
        """devices: [torch.device | 'cuda:N'] — the first entry is used (one process per GPU)."""
        agent_parameters = kwargs["agent_parameters"] if "agent_parameters" in kwargs else args[0]
        name = kwargs["name"] if "name" in kwargs else (args[2] if len(args) > 2 else "")
        cls = _family_of(agent_parameters.network_wrappers[name.split('/')[0]])
        return cls(*args, device=devices[0] if devices else None, variable_scope=variable_scope, **kwargs)

    def __init__(self, agent_parameters, spaces, name="", global_network=None, network_is_local=True,
                 network_is_trainable=True, device=None, variable_scope="", shared_with=None):
        super().__init__(agent_parameters, spaces, name)
        if type(self) is HipArchitecture:
            raise TypeError("use HipArchitecture.construct(...): the family is chosen from the network parameters")
        if global_network is not None:
            raise NotImplementedError("parameter-server (global network) mode is replaced by the gradient "
                                      "all-reduce of coach_amd.distributed.GradientSync")
        if not torch.cuda.is_available():
            raise _rlx.RlxUnavailable("HipArchitecture needs a GPU: the HIP path has no CPU fallback")
        self.variable_scope = variable_scope
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.network_is_local, self.network_is_trainable = network_is_local, network_is_trainable
        self.is_target = shared_with is not None
        if shared_with is None:
            self.net = self._build(agent_parameters, spaces, self.network_parameters,
                                   getattr(agent_parameters, "seed", 0) or 0)
        else:
            self.net = shared_with.net                    # the target view of the same device network
        self._handles()
        self.accumulated_gradients = None
        self.sess = None
        self.current_learning_rate = self.learning_rate

    # ---- what a family provides ------------------------------------------------------------
    def _build(self, agent_parameters, spaces, np_, seed):
        raise NotImplementedError

    def _handles(self):
        """Fetch / placeholder handles (output_heads, gradients_wrt_inputs, ...) and input names."""

    def _queue(self, inputs, tag):
        """Queue the forward pass on the device stream; returns whatever _fetch needs."""
        raise NotImplementedError

    def _fetch(self, queued):
        """-> the list of numpy outputs of predict()."""
        return [t.cpu().numpy() for t in queued]

    def _predict_fetch(self, inputs, outputs, feed):
        raise NotImplementedError("outputs={} is not a fetch of this network".format(outputs))

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        """Forward + loss + backward into params.grads (+ self.net.norm); returns
        (total_loss, losses, norm_unclipped_grads, fetched)."""
        raise NotImplementedError

    # ------------------------------------------------------------------------------ plumbing
    def _weights_buffer(self):
        return self.net.target if self.is_target else self.net.params.weights

    def _to_device(self, array, dtype=None):
        if isinstance(array, torch.Tensor):
            t = array.to(self.device)
        else:
            t = torch.from_numpy(np.ascontiguousarray(array)).to(self.device)
        return t if dtype is None or t.dtype == dtype else t.to(dtype)

    def _observation(self, inputs):
        for k in inputs:
            if isinstance(k, str) and k not in self.inputs:
                raise ValueError('input name {} was provided to create a feed dictionary, but there is no '
                                 'placeholder with that name. placeholder names available include: {}'
                                 .format(k, ', '.join(self.inputs)))
        obs = inputs['observation']
        B = int(obs.shape[0])
        obs = self._to_device(obs, torch.uint8 if self.net.image else torch.float32).contiguous()
        shape = tuple(getattr(self.net, "obs_shape", None) or (self.net.obs_dim,))
        if tuple(obs.shape[1:]) != shape:
            raise ValueError("observation shape {} does not match the network input {}"
                             .format(tuple(obs.shape[1:]), shape))
        return obs, B

    def _action(self, inputs, B, key='action'):
        if key not in inputs:
            raise ValueError("the critic needs the input {}".format(key))
        a = self._to_device(inputs[key], torch.float32).contiguous()
        if tuple(a.shape) != (B, self.net.A):
            raise ValueError("action shape {} does not match {}".format(tuple(a.shape), (B, self.net.A)))
        return a

    def _per_sample(self, array, B, what):
        t = self._to_device(array[0] if isinstance(array, (list, tuple)) else array, torch.float32)
        t = t.reshape(-1).contiguous()
        if t.numel() != B:
            raise ValueError("{} must hold one value per sample".format(what))
        return t

    def _action_column(self, inputs, key, B):
        """the discrete policy head's actions, inputs[key], as int32 [B]  (_action is the critics' fp32 [B, A] matrix)"""
        if key not in inputs:
            raise ValueError("the policy head needs the input {} (the actions)".format(key))
        actions = self._to_device(inputs[key], torch.int32).reshape(-1).contiguous()
        if actions.numel() != B:
            raise ValueError("{} must hold one action per sample".format(key))
        return actions

    def _softmax(self, logits, B):
        """logits [B, A] (a device buffer) -> the action probabilities in a fresh [B, A] tensor"""
        net = self.net
        probs = torch.empty(B, net.A, dtype=torch.float32, device=self.device)
        net.lib.softmax(logits, net.A, B, net.A, probs, net.A, _rlx.current_stream())
        return probs

    # ------------------------------------------------------------------------------ inference
    def predict(self, inputs, outputs=None, squeeze_output=True, initial_feed_dict=None):
        """One entry per head output (general_network.py outputs), fresh numpy arrays; `outputs` selects
        one of the family's fetch handles instead."""
        if outputs is not None:
            return self._predict_fetch(inputs, outputs, initial_feed_dict or {})
        out = self._fetch(self._queue(inputs, "predict"))
        return squeeze_list(out) if squeeze_output else out

    @staticmethod
    def parallel_predict(sess, network_input_tuples):
        """The reference runs the listed networks in one session.run; here every forward pass is queued
        on the device stream back to back and the results are fetched afterwards."""
        queued = [(net, net._queue(inputs, "pp%d" % i)) for i, (net, inputs) in enumerate(network_input_tuples)]
        return tuple(squeeze_list(net._fetch(q)) for net, q in queued)

    # ------------------------------------------------------------------------------- training
    def reset_accumulated_gradients(self):
        if self.accumulated_gradients is None:
            self.accumulated_gradients = torch.zeros_like(self.net.params.grads)
        else:
            self.accumulated_gradients.zero_()

    def accumulate_gradients(self, inputs, targets, additional_fetches=None, importance_weights=None,
                             no_accumulation=False):
        if not self.network_is_trainable or self.is_target:
            raise ValueError("{} is not trainable".format(self.name))
        if self.accumulated_gradients is None:
            self.reset_accumulated_gradients()
        result = self._accumulate_impl(inputs, targets, additional_fetches or [], importance_weights)
        net = self.net
        lib, s, n = net.lib, _rlx.current_stream(), net.params.size
        if no_accumulation:
            lib.axpby(self.accumulated_gradients, 1.0, net.params.grads, 0.0, None, n, s)
        else:
            lib.axpby(self.accumulated_gradients, 1.0, self.accumulated_gradients, 1.0, net.params.grads, n, s)
        return result

    def apply_gradients(self, gradients, scaler=1.):
        """The gradients are MULTIPLIED by scaler (tensorflow_components/architecture.py:469-521)."""
        p = self.net.params
        if isinstance(gradients, (list, tuple)):
            # per-variable tensors (the SAC policy text combines gradients variable by variable)
            if len(gradients) != len(p.entries) or any(e[2] != 1 for e in p.entries.values()):
                raise ValueError("a gradient list must hold one tensor per variable of a single-tower network")
            for name, g in zip(p.entries, gradients):
                dst = p.g(name)
                dst.copy_(self._to_device(g, torch.float32).reshape(dst.shape))
            gradients = p.grads
        if not isinstance(gradients, torch.Tensor) or gradients.numel() != p.size:
            raise ValueError("gradients must be the accumulated_gradients buffer of an identical network")
        self.net.adam.step(float(scaler), lr=self.current_learning_rate, grads=gradients)

    def apply_and_reset_gradients(self, gradients, scaler=1.):
        self.apply_gradients(gradients, scaler)
        self.reset_accumulated_gradients()

    def train_on_batch(self, inputs, targets, scaler=1., additional_fetches=None, importance_weights=None):
        result = self.accumulate_gradients(inputs, targets, additional_fetches, importance_weights)
        self.apply_and_reset_gradients(self.accumulated_gradients, scaler)
        return result

    # -------------------------------------------------------------------------------- weights
    def get_weights(self):
        return self._weights_buffer()

    def set_weights(self, weights, rate=1.0):
        """new = rate * given + (1 - rate) * old (architecture.py:598-607)."""
        own = self._weights_buffer()
        if not isinstance(weights, torch.Tensor) or weights.numel() != own.numel():
            raise ValueError("weights must come from get_weights() of an identical network")
        self.net.lib.mix_weights(own, weights, own.numel(), float(rate), _rlx.current_stream())

    def get_variable_value(self, variable):
        """variable: 'learning_rate' or a parameter name ('main/q_head/dense/kernel'; tower 0)."""
        if variable == 'learning_rate':
            return np.float32(self.current_learning_rate)
        return self.net.params.w(variable, 0, self._weights_buffer()).cpu().numpy()

    def set_variable_value(self, assign_op, value, placeholder=None):
        if assign_op == 'learning_rate':
            self.current_learning_rate = float(value)
            return
        dst = self.net.params.w(assign_op, 0, self._weights_buffer())
        dst.copy_(self._to_device(np.asarray(value, dtype=np.float32)).view_as(dst))

    def collect_savers(self, parent_path_suffix):
        from ..checkpoint import NetworkSaver
        return [NetworkSaver("%s.%s" % (parent_path_suffix, self.name.replace('/', '.')), self.net)]

    # ---- de-facto members the reference agents touch
    def set_session(self, sess):
        self.sess = sess

    def set_is_training(self, state):
        self.is_training = bool(state)

    def reset_internal_memory(self):
        pass


# ================================================================================ DQN / DDQN
class QArchitecture(HipArchitecture):
    """embedder -> FC middleware -> QHead | DuelingQHead; regression against explicit [B, A] targets."""

    def _build(self, agent_parameters, spaces, np_, seed):
        return DQNNet(self.device, _obs_shape(spaces), len(spaces.action.actions), **dqn_net_kwargs(np_, seed))

    def _queue(self, inputs, tag):
        obs, B = self._observation(inputs)
        net = self.net
        return [net.q_values(obs, B, use_target=self.is_target, tag="%s_%d" % (tag, B)).data.view(B, net.A)]

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        net = self.net
        obs, B = self._observation(inputs)
        target = targets[0] if isinstance(targets, (list, tuple)) else targets
        target = self._to_device(target, torch.float32).contiguous()
        if tuple(target.shape) != (B, net.A):
            raise ValueError("targets shape {} does not match the head output {}"
                             .format(tuple(target.shape), (B, net.A)))
        w = importance_weights[0] if isinstance(importance_weights, (list, tuple)) else importance_weights
        if w is not None:
            w = self._per_sample(np.asarray(w) if not isinstance(w, torch.Tensor) else w, B, "importance_weights")
        net.accumulate_regression(obs, B, target, w)
        total_loss = float(net.loss.item())
        net.check_status()
        return total_loss, [total_loss], float(net.norm.item()), []


# =============================================================================== Clipped PPO
class PPOArchitecture(HipArchitecture):
    """Two embedder + middleware copies, head 0 = VHead, head 1 = PPOHead (discrete or continuous)."""

    def _build(self, agent_parameters, spaces, np_, seed):
        alg = agent_parameters.algorithm
        continuous = not hasattr(spaces.action, "actions")
        n_act = int(spaces.action.shape[0]) if continuous else len(spaces.action.actions)
        return ClippedPPONet(self.device, _obs_shape(spaces), n_act,
                             clip_likelihood_ratio_using_epsilon=alg.clip_likelihood_ratio_using_epsilon,
                             beta_entropy=alg.beta_entropy, continuous=continuous, **common_net_kwargs(np_, seed))

    def _handles(self):
        self.n_dist = 2 if self.net.continuous else 1           # old policy: [probs] or [mean, std]
        self.inputs = ['observation'] + ['output_1_%d' % i for i in range(self.n_dist + 2)]
        self.output_heads = [_HeadFetches(0, ['output']),
                             _HeadFetches(1, ['kl_divergence', 'entropy', 'likelihood_ratio',
                                              'clipped_likelihood_ratio', 'output'])]

    def _queue(self, inputs, tag):
        """[V (B, 1), policy probabilities (B, A)] or [V, policy_mean, policy_std]."""
        obs, B = self._observation(inputs)
        net, tag = self.net, "%s_%d" % (tag, B)
        w = net.target if self.is_target else None
        acts = net.torso.forward(net.ctx, net.obs_tensor(obs, B), tag=tag + "v", weights=w, t0=0, nt=1)
        v = net.v_head.forward(net.ctx, acts[-1], tag=tag + "v", weights=w).data.view(B, 1)
        if net.continuous:
            mean, std = net.policy_mean_std(obs, B, use_target=self.is_target, tag=tag)
            return [v, mean, std]
        return [v, net.policy_probs(obs, B, use_target=self.is_target, tag=tag)]

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        """The feed of ClippedPPOAgent.train_network (clipped_ppo_agent.py:226-266)."""
        net, n_dist = self.net, self.n_dist
        obs, B = self._observation(inputs)
        for k in ['output_1_%d' % i for i in range(n_dist + 1)]:
            if k not in inputs:
                raise ValueError("the PPO head needs the input {}".format(k))
        if not isinstance(targets, (list, tuple)) or len(targets) != 2:
            raise ValueError("targets must be [value targets, advantages]")
        f32 = torch.float32
        actions = self._to_device(inputs['output_1_0'], f32 if net.continuous else torch.int32).contiguous()
        old = [self._to_device(inputs['output_1_%d' % (i + 1)], f32).contiguous() for i in range(n_dist)]
        rescaler = float(np.asarray(inputs.get('output_1_%d' % (n_dist + 1), 1.0)).reshape(-1)[0])
        value_targets = self._per_sample(targets[0], B, "value targets")
        advantages = self._per_sample(targets[1], B, "advantages")
        if actions.shape[0] != B or any(tuple(o.shape) != (B, net.A) for o in old):
            raise ValueError("head inputs do not match the batch size {}".format(B))
        ratio = torch.empty(B, dtype=f32, device=self.device)
        clipped = torch.empty(B, dtype=f32, device=self.device)
        net.forward_backward(obs, B, actions, advantages, value_targets, tuple(old) if net.continuous else old[0],
                             rescaler, ratio, clipped)
        net.grad_norm()
        sc = net.scalars.cpu().numpy()      # [surrogate, entropy, kl, policy-head total, value loss, grad norm]
        net.check_status()
        head = self.output_heads[1]
        table = {head.kl_divergence: lambda: sc[2], head.entropy: lambda: sc[1],
                 head.likelihood_ratio: lambda: ratio.cpu().numpy(),
                 head.clipped_likelihood_ratio: lambda: clipped.cpu().numpy()}
        losses = [float(sc[4]), float(sc[3])]                   # head 0 (V), head 1 (PPO)
        return float(sc[4] + sc[3]), losses, float(sc[5]), _fetched(table, additional_fetches)


# ================================================================================ DDPG / TD3
def _no_batchnorm(np_):
    if getattr(np_, "batchnorm", False):
        # the moving averages step on the batch fed WITH apply_gradients (additional_inputs, ddpg_agent.py:178-193); this
        # interface keeps no such pass — coach_amd.agents.ddpg_agent.DDPGAgent runs the batch-normalised networks
        raise NotImplementedError("batch-normalised DDPG networks are driven by coach_amd.agents.ddpg_agent.DDPGAgent, "
                                  "not through the Architecture plug-in interface")


class ActorArchitecture(HipArchitecture):
    def _build(self, agent_parameters, spaces, np_, seed):
        scale = float(np.maximum(np.abs(spaces.action.low), np.abs(spaces.action.high)).max())
        _no_batchnorm(np_)
        return ActorNet(self.device, int(spaces.state['observation'].shape[0]), int(spaces.action.shape[0]), scale,
                        np_.observation_embedder_scheme, np_.middleware_scheme, np_.activation_function,
                        *_adam_args(np_), seed)

    def _handles(self):
        self.gradients_weights_ph = ["gradients_weights_ph/0"]
        self.weighted_gradients = ["weighted_gradients/0"]

    def _queue(self, inputs, tag):
        obs, B = self._observation(inputs)
        return [self.net.forward(obs, B, use_target=self.is_target, tag="%s_%d" % (tag, B))[0]]

    def _predict_fetch(self, inputs, outputs, feed):
        """weighted_gradients[0]: d sum(actions * w) / d theta with w = feed[gradients_weights_ph[0]]."""
        if squeeze_list(outputs) != self.weighted_gradients[0]:
            return super()._predict_fetch(inputs, outputs, feed)
        net = self.net
        obs, B = self._observation(inputs)
        if self.is_target or self.gradients_weights_ph[0] not in feed:
            raise ValueError("weighted_gradients needs initial_feed_dict[gradients_weights_ph[0]] on the "
                             "online actor")
        w = self._to_device(np.asarray(feed[self.gradients_weights_ph[0]], dtype=np.float32)).contiguous()
        if tuple(w.shape) != (B, net.A):
            raise ValueError("gradient weights shape {} does not match {}".format(tuple(w.shape), (B, net.A)))
        _, saved = net.forward(obs, B, tag="wgrad")
        net.backward(saved, w, B)
        return net.params.grads.clone()

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        raise NotImplementedError("the actor has no loss head: its gradients come from "
                                  "predict(outputs=weighted_gradients[0])")


class CriticArchitecture(HipArchitecture):
    """DDPG critic (one stream: outputs [Q, mean Q]) / TD3 twin critic ([Q1, Q2, min, mean Q1])."""

    def _build(self, agent_parameters, spaces, np_, seed):          # the agents seed the critic with seed + 1
        _no_batchnorm(np_)
        return CriticNet(self.device, int(spaces.state['observation'].shape[0]), int(spaces.action.shape[0]),
                         np_.observation_embedder_scheme, np_.middleware_scheme, np_.num_streams,
                         np_.activation_function, np_.head_initializer, *_adam_args(np_), seed + 1)

    def _handles(self):
        self.inputs = ['observation', 'action']
        n_out = 2 if self.net.T == 1 else 4
        self.gradients_wrt_inputs = [{k: "gradients_wrt_inputs/%d/%s" % (i, k) for k in self.inputs}
                                     for i in range(n_out)]

    def _queue(self, inputs, tag):
        obs, B = self._observation(inputs)
        q, _ = self.net.forward(obs, self._action(inputs, B), B, use_target=self.is_target, tag="%s_%d" % (tag, B))
        return q, B

    def _fetch(self, queued):
        q, B = queued
        q = q.cpu().numpy()                                         # [T, B]
        if self.net.T == 1:
            return [q[0].reshape(B, 1), q[0].mean()]
        return [q[0].reshape(B, 1), q[1].reshape(B, 1), np.minimum(q[0], q[1]).reshape(B, 1), q[0].mean()]

    def _predict_fetch(self, inputs, outputs, feed):
        """gradients_wrt_inputs[mean output]['action'] = d mean(Q1) / d action."""
        mean_output = len(self.gradients_wrt_inputs) - 1
        if squeeze_list(outputs) != self.gradients_wrt_inputs[mean_output]['action'] or self.is_target:
            raise NotImplementedError("only gradients_wrt_inputs[{}]['action'] of the online critic is "
                                      "available (d mean(Q1) / d action)".format(mean_output))
        net = self.net
        obs, B = self._observation(inputs)
        _, saved = net.forward(obs, self._action(inputs, B), B, tag="agrad")
        g = torch.empty(B, net.A, dtype=torch.float32, device=self.device)
        net.action_gradient(saved, B, g, scale=1.0)
        return g.cpu().numpy()

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        net = self.net
        obs, B = self._observation(inputs)
        actions = self._action(inputs, B)
        target = self._per_sample(targets, B, "TD targets")
        _, saved = net.forward(obs, actions, B, tag="train")
        net.train_backward(saved, target, B)
        net.grad_norm()
        losses = [float(x) for x in net.loss[:net.T].cpu().numpy()]
        return float(sum(losses)), losses, float(net.norm.item()), []


# ======================================================================================= SAC
class SACPolicyArchitecture(HipArchitecture):
    """predict -> [mu, log_std, raw actions, actions, logprob, mean logprob]; every call draws fresh
    N(0, 1) noise from np.random, like every sess.run of the TF graph's sampling op."""

    def _build(self, agent_parameters, spaces, np_, seed):
        return SACPolicyNet(self.device, int(spaces.state['observation'].shape[0]), int(spaces.action.shape[0]),
                            np_.embedder_scheme, np_.middleware_scheme, *_adam_args(np_), seed=seed)

    def _handles(self):
        self.gradients_weights_ph = ["gradients_weights_ph/%d" % i for i in range(6)]
        self.weighted_gradients = ["weighted_gradients/%d" % i for i in range(6)]

    def _sample(self, inputs, tag):
        obs, B = self._observation(inputs)
        normals = self._to_device(np.random.standard_normal((B, self.net.A)), torch.float64).contiguous()
        return self.net.forward(obs, B, normals, tag=tag), B

    def _queue(self, inputs, tag):
        (o, _), B = self._sample(inputs, tag)
        return o

    def _fetch(self, o):
        lp = o["logprob"].cpu().numpy()
        return [o["mean"].cpu().numpy(), o["log_std"].cpu().numpy(), o["raw_actions"].cpu().numpy(),
                o["actions"].cpu().numpy(), lp, lp.mean()]

    def _grad_list(self):
        """params.grads as a list of per-variable tensors (views of one fresh flat copy)."""
        p = self.net.params
        flat = p.grads.clone()
        return [p.view(flat, name) for name in p.entries]

    def _predict_fetch(self, inputs, outputs, feed):
        fetch = squeeze_list(outputs)
        if fetch not in (self.weighted_gradients[5], self.weighted_gradients[3]):
            raise NotImplementedError("only weighted_gradients[5] (mean log-prob) and [3] (actions) exist")
        idx = 5 if fetch == self.weighted_gradients[5] else 3
        if self.gradients_weights_ph[idx] not in feed:
            raise ValueError("weighted_gradients[{0}] needs initial_feed_dict[gradients_weights_ph[{0}]]".format(idx))
        w = feed[self.gradients_weights_ph[idx]]
        net = self.net
        (_, saved), B = self._sample(inputs, "wgrad")
        if idx == 5:
            net.backward(saved, B, logprob_mean_weight=float(np.asarray(w)))
        else:
            wd = self._to_device(np.asarray(w, dtype=np.float32)).contiguous()
            if tuple(wd.shape) != (B, net.A):
                raise ValueError("gradient weights shape {} does not match {}".format(tuple(wd.shape), (B, net.A)))
            net.backward(saved, B, action_weights=wd)
        return self._grad_list()

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        raise NotImplementedError("the SAC policy has no loss head: its gradients come from "
                                  "predict(outputs=weighted_gradients[k])")


class SACQArchitecture(HipArchitecture):
    """Twin Q head: predict -> [min(Q1, Q2), its mean]; inputs 'observation' + 'output_0_0' (actions)."""

    def _build(self, agent_parameters, spaces, np_, seed):          # the agent's seeds: policy, q + 1, v + 2
        return SACQNet(self.device, int(spaces.state['observation'].shape[0]), int(spaces.action.shape[0]),
                       np_.network_layers_sizes, *_adam_args(np_), seed=seed + 1)

    def _handles(self):
        self.inputs = ['observation', 'output_0_0']
        self.output_heads = [_HeadFetches(0, ['q1_output', 'q2_output', 'q1_loss', 'q2_loss', 'q_output'])]
        self.gradients_wrt_inputs = [{k: "gradients_wrt_inputs/%d/%s" % (i, k) for k in self.inputs}
                                     for i in range(2)]           # outputs: [q_output, q_output_mean]

    def _queue(self, inputs, tag):
        obs, B = self._observation(inputs)
        q, saved = self.net.forward(obs, self._action(inputs, B, 'output_0_0'), B, tag="%s_%d" % (tag, B))
        return q, saved, B

    def _fetch(self, queued):
        q, _, B = queued
        q = q.cpu().numpy()
        qmin = np.minimum(q[0], q[1])
        return [qmin.reshape(B, 1), qmin.mean()]

    def _predict_fetch(self, inputs, outputs, feed):
        net, head = self.net, self.output_heads[0]
        if isinstance(outputs, (list, tuple)):
            q, _, B = self._queue(inputs, "predict")
            q = q.cpu().numpy()
            table = {head.q1_output: q[0].reshape(B, 1), head.q2_output: q[1].reshape(B, 1),
                     head.q_output: np.minimum(q[0], q[1]).reshape(B, 1)}
            if any(f not in table for f in outputs):
                raise NotImplementedError("unknown fetch in {}".format(outputs))
            return [table[f] for f in outputs]
        if outputs != self.gradients_wrt_inputs[1]['output_0_0']:
            raise NotImplementedError("only gradients_wrt_inputs[1]['output_0_0'] (d mean(min Q) / d action) exists")
        _, saved, B = self._queue(inputs, "agrad")
        g = torch.empty(B, net.A, dtype=torch.float32, device=self.device)
        net.action_gradient(saved, B, g)
        return g.cpu().numpy()

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        net, head = self.net, self.output_heads[0]
        obs, B = self._observation(inputs)
        target = self._per_sample(targets, B, "targets")
        _, saved = net.forward(obs, self._action(inputs, B, 'output_0_0'), B, tag="train")
        net.train_backward(saved, target, B)
        net.grad_norm()
        loss = net.loss.cpu().numpy()
        table = {head.q1_loss: lambda: loss[0], head.q2_loss: lambda: loss[1]}
        total = float(loss[:2].sum())
        return total, [total], float(net.norm.item()), _fetched(table, additional_fetches)


class SACValueArchitecture(HipArchitecture):
    def _build(self, agent_parameters, spaces, np_, seed):
        return SACValueNet(self.device, int(spaces.state['observation'].shape[0]), np_.embedder_scheme,
                           np_.middleware_scheme, *_adam_args(np_), seed=seed + 2)

    def _queue(self, inputs, tag):
        obs, B = self._observation(inputs)
        return [self.net.forward(obs, B, use_target=self.is_target, tag="%s_%d" % (tag, B))[0].view(B, 1)]

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        net = self.net
        obs, B = self._observation(inputs)
        target = self._per_sample(targets, B, "targets")
        _, saved = net.forward(obs, B, tag="train")
        net.train_backward(saved, target, B)
        net.grad_norm()
        total = float(net.loss.sum().item())
        return total, [total], float(net.norm.item()), []


# ========================================================================== Policy Gradients
class PolicyGradientArchitecture(HipArchitecture):
    """embedder -> FC middleware -> discrete PolicyHead, fed the way PolicyGradientsAgent.learn_from_batch feeds it
    (policy_gradients_agent.py:128-130): inputs 'observation' and 'output_0_0' = actions, targets = the rescaled
    returns (the head's `advantages` placeholder, fp32).  predict -> [action probabilities (B, A)]."""

    def _build(self, agent_parameters, spaces, np_, seed):
        A = _discrete_actions(spaces, "the continuous PolicyHead (a Box action space) is not served: the policy-gradient "
                                      "network has the discrete head only")
        return PolicyGradientNet(self.device, _obs_shape(spaces), A,
                                 **policy_gradient_net_kwargs(np_, agent_parameters.algorithm, seed))

    def _handles(self):
        self.inputs = ['observation', 'output_0_0']
        self.output_heads = [_HeadFetches(0, ['entropy', 'output'])]

    def _queue(self, inputs, tag):
        obs, B = self._observation(inputs)
        net = self.net
        return [self._softmax(net.policy_values(obs, B, tag="%s_%d" % (tag, B)).data.view(B, net.A), B)]

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        net = self.net
        obs, B = self._observation(inputs)
        actions = self._action_column(inputs, 'output_0_0', B)
        advantages = self._per_sample(targets, B, "targets (the rescaled returns)")
        net.window_gradients(obs, B, actions, advantages)
        sc = net.scalars.cpu().numpy()
        net.check_status()
        fetched = _fetched({self.output_heads[0].entropy: lambda: sc[1]}, additional_fetches)
        return float(sc[0]), [float(sc[0])], float(net.norm.item()), fetched


# ============================================================= Classification (imitation models)
class ClassificationArchitecture(HipArchitecture):
    """embedder -> FC middleware -> ClassificationHead, fed the way DDQNBCQAgent.improve_reward_model feeds the imitation
    model (ddqn_bcq_agent.py:168-171): inputs 'observation', targets = the one-hot (or any dense) [B, A] label matrix.
    predict -> [class probabilities (B, A)].  The loss is the softmax cross entropy SUMMED over the batch
    (rlx_classification_head_loss)."""

    def _build(self, agent_parameters, spaces, np_, seed):
        from ..nn.networks import ClassificationNet, classification_net_kwargs
        A = _discrete_actions(spaces, "the ClassificationHead over a Box action space (one output) is not served")
        return ClassificationNet(self.device, _obs_shape(spaces), A, **classification_net_kwargs(np_, seed))

    def _handles(self):
        self.output_heads = [_HeadFetches(0, ['output'])]

    def _queue(self, inputs, tag):
        obs, B = self._observation(inputs)
        return [self.net.predict(obs, B, tag="%s_%d" % (tag, B))]

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        net = self.net
        obs, B = self._observation(inputs)
        target = targets[0] if isinstance(targets, (list, tuple)) else targets
        target = self._to_device(target, torch.float32).contiguous()
        if tuple(target.shape) != (B, net.A):
            raise ValueError("targets shape {} does not match the head output {}".format(tuple(target.shape), (B, net.A)))
        if importance_weights is not None:
            raise ValueError("the ClassificationHead takes no importance weights")
        net.accumulate_gradients(obs, B, labels=target)
        total_loss = float(net.loss.item())
        net.check_status()
        return total_loss, [total_loss], float(net.norm.item()), _fetched({}, additional_fetches)


# ========================================================================== Actor-Critic
class ActorCriticArchitecture(HipArchitecture):
    """embedder -> FC middleware -> VHead (head 0) + discrete PolicyHead (head 1), fed the way
    ActorCriticAgent.learn_from_batch feeds it (actor_critic_agent.py:175-177): inputs 'observation' and 'output_1_0' =
    actions, targets = [value targets (B, 1), advantages (B,)], fp64, rounded to fp32 once at the heads' placeholders
    (rlx_a3c_window_loss with RLX_A3C_TARGETS_GIVEN).  predict -> [V (B, 1), action probabilities (B, A)];
    accumulate_gradients -> total loss, [value loss, policy loss, the entropy regulariser], the gradients' norm."""

    def _build(self, agent_parameters, spaces, np_, seed):
        A = _discrete_actions(spaces, "the continuous PolicyHead (a Box action space) is not served: the actor-critic "
                                      "network has the discrete head only")
        return ActorCriticNet(self.device, _obs_shape(spaces), A,
                              **actor_critic_net_kwargs(np_, agent_parameters.algorithm, seed))

    def _handles(self):
        self.inputs = ['observation', 'output_1_0']
        self.output_heads = [_HeadFetches(0, ['output']), _HeadFetches(1, ['entropy', 'output'])]

    def _queue(self, inputs, tag):
        obs, B = self._observation(inputs)
        net = self.net
        v, z = net.predict(obs, B, tag="%s_%d" % (tag, B))
        return [v.view(B, 1), self._softmax(z, B)]

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        net = self.net
        obs, B = self._observation(inputs)
        actions = self._action_column(inputs, 'output_1_0', B)
        if not isinstance(targets, (list, tuple)) or len(targets) != 2:
            raise ValueError("targets must be [the V head's targets, the policy head's advantages]")
        value_targets, advantages = (self._to_device(t, torch.float64).reshape(-1).contiguous() for t in targets)
        if value_targets.numel() != B or advantages.numel() != B:
            raise ValueError("the value targets and the advantages must hold one value per sample")
        net.window_gradients(obs, B, False, actions, value_targets, advantages)
        sc = net.scalars.cpu().numpy()
        net.check_status()
        fetched = _fetched({self.output_heads[1].entropy: lambda: sc[3]}, additional_fetches)
        losses = _with_entropy_regulariser([float(sc[1]), float(sc[2])], net, sc[3])
        return float(sc[0]), losses, float(net.norm.item()), fetched


# =============================================================================== N-step Q
class NStepQArchitecture(HipArchitecture):
    """embedder -> FC middleware -> QHead with a target copy, fed the way NStepQAgent.learn_from_batch feeds it
    (n_step_q_agent.py:134): input 'observation', targets = [state_value_head_targets (B, A)], the online prediction with
    the taken actions' columns replaced.  A full target matrix is the head's regression against every column
    (rlx_regression_loss; the untouched columns give exactly zero).  predict -> Q (B, A), of the online or the target
    view; accumulate_gradients -> total loss, [the Q head's loss], the gradients' norm."""

    def _build(self, agent_parameters, spaces, np_, seed):
        A = _discrete_actions(spaces, "a Box action space is not served: the N-step Q network has the discrete QHead only")
        return NStepQNet(self.device, _obs_shape(spaces), A, **n_step_q_net_kwargs(np_, seed))

    def _queue(self, inputs, tag):
        obs, B = self._observation(inputs)
        net, tag = self.net, "%s_%d" % (tag, B)
        q = net.target_q_values(obs, B, tag=tag + "_t") if self.is_target else net.q_values(obs, B, tag=tag)
        return [q.data.view(B, net.A)]

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        net = self.net
        obs, B = self._observation(inputs)
        target = targets[0] if isinstance(targets, (list, tuple)) else targets
        target = self._to_device(target, torch.float32).contiguous()
        if tuple(target.shape) != (B, net.A):
            raise ValueError("targets shape {} does not match the head output {}".format(tuple(target.shape), (B, net.A)))
        if importance_weights is not None:
            raise ValueError("the N-step Q head takes no importance weights")
        _fetched({}, additional_fetches)                 # (the head offers none)
        net.window_gradients(obs, B, None, None, target_matrix=target)
        total_loss = float(net.loss.item())
        return total_loss, [total_loss], float(net.norm.item()), []


# =================================================================================== ACER
class ACERArchitecture(HipArchitecture):
    """embedder -> FC middleware -> QHead (head 0) + ACERPolicyHead (head 1) with a target copy (the average policy
    network), fed the way ACERAgent._learn_from_batch feeds it (acer_agent.py:157-165): inputs 'observation',
    'output_1_0' = actions, 'output_1_1' = rho (B, A), 'output_1_2' = rho_i (B,), 'output_1_3' = the aliased Q values
    (B, A), 'output_1_4' = Q_retrace (B,), 'output_1_5' = the average policy (B, A); targets = [the Q head's target
    matrix (B, A), the state values (B,)] (rlx_acer_window_loss with RLX_ACER_TARGETS_GIVEN).  predict -> [Q (B, A),
    action probabilities (B, A)], of the online or the target view; accumulate_gradients -> total loss, [Q loss, policy
    loss (, the entropy regulariser)], the gradients' norm; fetches: probability_loss, bias_correction_loss,
    kl_divergence of head 1."""

    def _build(self, agent_parameters, spaces, np_, seed):
        A = _discrete_actions(spaces, "only discrete action spaces are supported for ACER")
        return ACERNet(self.device, _obs_shape(spaces), A, **acer_net_kwargs(np_, agent_parameters.algorithm, seed))

    def _handles(self):
        self.inputs = ['observation'] + ['output_1_%d' % i for i in range(6)]
        self.output_heads = [_HeadFetches(0, ['output']),
                             _HeadFetches(1, ['probability_loss', 'bias_correction_loss', 'kl_divergence', 'output'])]

    def _queue(self, inputs, tag):
        obs, B = self._observation(inputs)
        tag = "%s_%d%s" % (tag, B, "_t" if self.is_target else "")
        q, z = self.net.predict(obs, B, tag=tag, use_target=self.is_target)
        return [q, self._softmax(z, B)]

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        net = self.net
        obs, B = self._observation(inputs)
        missing = [n for n in self.inputs[1:] if n not in inputs]
        if missing:
            raise ValueError("the ACER policy head needs the inputs {}".format(missing))
        if not isinstance(targets, (list, tuple)) or len(targets) != 2:
            raise ValueError("targets must be [the Q head's target matrix, the state values]")
        f32 = lambda v, shape: self._to_device(v, torch.float32).reshape(shape).contiguous()
        actions = self._action_column(inputs, 'output_1_0', B)
        A = net.A
        try:
            given = dict(rho=f32(inputs['output_1_1'], (B, A)), rho_i=f32(inputs['output_1_2'], (B,)),
                         td_targets=f32(inputs['output_1_3'], (B, A)), q_retrace=f32(inputs['output_1_4'], (B,)),
                         avg_policy=f32(inputs['output_1_5'], (B, A)), V=f32(targets[1], (B,)))
            q_targets = f32(targets[0], (B, A))
        except RuntimeError as e:
            raise ValueError("an ACER input does not have its shape for a batch of {}: {}".format(B, e))
        # the reference hands ONE array as 'output_1_3' and as the Q head's target; the launch reads it once
        if not torch.equal(q_targets, given["td_targets"]):
            raise ValueError("the Q head's targets must be the matrix handed in as output_1_3 (the reference aliases them)")
        net.window_gradients(obs, B, False, actions, given=given)
        sc = net.scalars.cpu().numpy()
        net.check_status()
        head = self.output_heads[1]
        table = {head.probability_loss: lambda: sc[3], head.bias_correction_loss: lambda: sc[4],
                 head.kl_divergence: lambda: sc[5]}
        fetched = _fetched(table, additional_fetches)
        losses = _with_entropy_regulariser([float(sc[1]), float(sc[2])], net, sc[6])
        return float(sc[0]), losses, float(net.norm.item()), fetched


# ================================================================================ PPO (KL penalty)
class PPOActorArchitecture(HipArchitecture):
    """embedder -> FC middleware -> PPOHead without a clip range and with the KL penalty, fed the way
    PPOAgent.train_policy_network feeds it (ppo_agent.py:278-288): inputs 'observation', 'output_0_0' = actions,
    'output_0_1' (, 'output_0_2') = the old policy's probabilities (mean, std); targets = [advantages].  predict -> the
    action probabilities, or [mean, std].  The head's kl_coefficient is readable / assignable through
    get_variable_value / set_variable_value (ppo_agent.py:336-351)."""

    def _build(self, agent_parameters, spaces, np_, seed):
        alg = agent_parameters.algorithm
        if alg.clip_likelihood_ratio_using_epsilon is not None:
            raise ValueError("clip_likelihood_ratio_using_epsilon is not None: that is the Clipped PPO network")
        continuous = not hasattr(spaces.action, "actions")
        n_act = int(spaces.action.shape[0]) if continuous else len(spaces.action.actions)
        return PPOActorNet(self.device, _obs_shape(spaces), n_act,
                           beta_entropy=alg.beta_entropy, target_kl_divergence=alg.target_kl_divergence,
                           initial_kl_coefficient=alg.initial_kl_coefficient,
                           high_kl_penalty_coefficient=alg.high_kl_penalty_coefficient,
                           use_kl_regularization=alg.use_kl_regularization, continuous=continuous,
                           **common_net_kwargs(np_, seed))

    def _handles(self):
        self.n_dist = 2 if self.net.continuous else 1
        self.inputs = ['observation'] + ['output_0_%d' % i for i in range(self.n_dist + 1)]
        self.output_heads = [_HeadFetches(0, ['kl_divergence', 'entropy', 'likelihood_ratio', 'output', 'kl_coefficient',
                                              'assign_kl_coefficient', 'kl_coefficient_ph'])]

    def _queue(self, inputs, tag):
        obs, B = self._observation(inputs)
        net, tag = self.net, "%s_%d" % (tag, B)
        if net.continuous:
            return list(net.policy_mean_std(obs, B, use_target=self.is_target, tag=tag))
        return [net.policy_probs(obs, B, use_target=self.is_target, tag=tag)]

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        net, n_dist = self.net, self.n_dist
        obs, B = self._observation(inputs)
        for k in self.inputs[1:]:
            if k not in inputs:
                raise ValueError("the PPO head needs the input {}".format(k))
        f32 = torch.float32
        actions = self._to_device(inputs['output_0_0'], f32 if net.continuous else torch.int32).contiguous()
        old = [self._to_device(inputs['output_0_%d' % (i + 1)], f32).contiguous() for i in range(n_dist)]
        advantages = self._per_sample(targets, B, "targets ([advantages])")
        if actions.shape[0] != B or any(tuple(o.shape) != (B, net.A) for o in old):
            raise ValueError("head inputs do not match the batch size {}".format(B))
        ratio = torch.empty(B, dtype=f32, device=self.device)
        net.forward_backward(obs, B, actions, advantages, tuple(old) if net.continuous else old[0], ratio,
                             accumulate=False)
        net.grad_norm()
        sc = net.scalars.cpu().numpy()      # [surrogate, entropy, kl, total, penalty factor]
        net.check_status()
        head = self.output_heads[0]
        table = {head.kl_divergence: lambda: sc[2], head.entropy: lambda: sc[1],
                 head.likelihood_ratio: lambda: ratio.cpu().numpy()}
        return float(sc[3]), [float(sc[0])], float(net.norm.item()), _fetched(table, additional_fetches)

    def get_variable_value(self, variable):
        if variable == self.output_heads[0].kl_coefficient:
            return np.float32(self.net.kl_coefficient.item())
        return super().get_variable_value(variable)

    def set_variable_value(self, assign_op, value, placeholder=None):
        if assign_op == self.output_heads[0].assign_kl_coefficient:
            self.net.kl_coefficient.fill_(float(np.float32(value)))
            return
        super().set_variable_value(assign_op, value, placeholder)


class PPOCriticArchitecture(HipArchitecture):
    """embedder -> FC middleware -> the plain VHead (MSE), fed the way PPOAgent.train_value_network feeds it
    (ppo_agent.py:227-233): inputs 'observation', targets = the returns (B, 1).  predict -> V (B, 1)."""

    def _build(self, agent_parameters, spaces, np_, seed):
        return PPOCriticNet(self.device, _obs_shape(spaces), **common_net_kwargs(np_, seed))

    def _handles(self):
        self.inputs = ['observation']
        self.output_heads = [_HeadFetches(0, ['output'])]

    def _queue(self, inputs, tag):
        obs, B = self._observation(inputs)
        return [self.net.values(obs, B, use_target=self.is_target, tag="%s_%d" % (tag, B)).view(B, 1)]

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        net = self.net
        obs, B = self._observation(inputs)
        _fetched({}, additional_fetches)                 # (the head offers none)
        net.forward_backward(obs, B, self._per_sample(targets, B, "targets (the returns)"))
        net.grad_norm()
        loss = float(net.loss.item())
        return loss, [loss], float(net.norm.item()), []


# ==================================================================================== DFP
class DFPArchitecture(HipArchitecture):
    """goal / measurements / observation embedders -> concatenation -> MeasurementsPredictionHead, no target network, fed
    the way DFPAgent feeds it (dfp_agent.py:150-167, :172-174): inputs 'observation' (B, D), 'measurements' (B, M) and
    'goal' (B, M) — a missing or an extra key is refused; targets = the prediction with the taken actions' rows replaced
    by the stored future measurements (B, A, K), NaN where a step lies past the episode's end.  predict -> the prediction
    (B, A, K).  A full target tensor is the head's loss against every entry: the entries that equal the prediction and
    the NaN entries give exactly zero, so the row with the differing entries is the taken action's
    (rlx_dfp_head_loss; more than one differing row per sample is refused).  accumulate_gradients -> total loss, [the
    head's loss], the gradients' norm."""

    def _build(self, agent_parameters, spaces, np_, seed):
        A = _discrete_actions(spaces, "a Box action space is not served: the DFP network predicts measurements per discrete "
                                      "action")
        if len(spaces.state['observation'].shape) != 1:
            raise ValueError("image observations are not served: the DFP network has vector embedders only")
        return DFPNet(self.device, int(spaces.state['observation'].shape[0]), int(spaces.state['measurements'].shape[0]),
                      A, int(agent_parameters.algorithm.num_predicted_steps_ahead),
                      **dfp_net_kwargs(np_, seed))

    def _handles(self):
        self.inputs = list(DFPNet.INPUTS)
        self.output_heads = [_HeadFetches(0, ['output'])]

    def _inputs(self, inputs):
        if sorted(inputs) != sorted(self.inputs):
            raise ValueError('the DFP network takes the inputs {}, got {}'.format(self.inputs, sorted(inputs)))
        net = self.net
        B = int(np.asarray(inputs['observation']).shape[0]) if not isinstance(inputs['observation'], torch.Tensor) \
            else int(inputs['observation'].shape[0])
        out = {}
        for k in self.inputs:
            t = self._to_device(inputs[k], torch.float32).contiguous()
            if tuple(t.shape) != (B, net.dims[k]):
                raise ValueError("input {} has shape {}, the network takes {}".format(k, tuple(t.shape), (B, net.dims[k])))
            out[k] = t
        return out, B

    def _merged(self, e, x, B):
        """the head's output from the two stream outputs: rlx_dfp_head_loss's y_out with no valid target (all NaN)."""
        net = self.net
        y = torch.empty(B, net.A, net.K, dtype=torch.float32, device=self.device)
        nan = torch.full((B, net.K), float("nan"), dtype=torch.float32, device=self.device)
        zero = torch.zeros(B, dtype=torch.int32, device=self.device)
        de = torch.empty(B, net.K, dtype=torch.float32, device=self.device)           # (all zero: nothing to learn from)
        dx = torch.empty(B, net.A * net.K, dtype=torch.float32, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        net.lib.dfp_head_loss(e, net.K, x, net.A * net.K, zero, nan, net.A, net.K, B, 1.0, de, net.K, dx, net.A * net.K,
                              net.loss_ws, net.ticket, loss, net.status, y, None, _rlx.current_stream())
        return y

    def _queue(self, inputs, tag):
        ins, B = self._inputs(inputs)
        if B > 256:
            raise ValueError("the DFP head's launches take at most 256 rows")
        e, x = self.net.streams(ins, B, tag="%s_%d" % (tag, B))
        return [self._merged(e, x, B)]

    def _accumulate_impl(self, inputs, targets, additional_fetches, importance_weights):
        net = self.net
        ins, B = self._inputs(inputs)
        if importance_weights is not None:
            raise ValueError("the measurements prediction head takes no importance weights")
        _fetched({}, additional_fetches)                 # (the head offers none)
        target = targets[0] if isinstance(targets, (list, tuple)) else targets
        target = self._to_device(target, torch.float32).contiguous()
        if tuple(target.shape) != (B, net.A, net.K):
            raise ValueError("targets shape {} does not match the head output {}"
                             .format(tuple(target.shape), (B, net.A, net.K)))
        # which row of every sample differs from the prediction?  (NaN entries differ from everything: they count, so an
        # all-NaN row is found as well; its loss and gradient are zero either way)
        e, x = net.streams(ins, B, tag="targets_%d" % B)
        y = self._merged(e, x, B)
        differs = ((target != y) | torch.isnan(target)).any(dim=2)
        if int((differs.sum(dim=1) > 1).sum().item()):
            raise ValueError("the targets differ from the prediction in more than one action's row of a sample")
        actions = differs.int().argmax(dim=1).int().contiguous()
        future = target[torch.arange(B, device=self.device), actions.long()].contiguous()
        net.accumulate(ins, B, actions, future)
        net.grad_norm()
        total_loss = float(net.loss.item())
        net.check_status()
        return total_loss, [total_loss], float(net.norm.item()), []


_BY_PARAMETER_CLASS = {"PolicyGradientNetworkParameters": PolicyGradientArchitecture,
                       "BCNetworkParameters": PolicyGradientArchitecture,          # a discrete PolicyHead, targets of ones
                       "DFPNetworkParameters": DFPArchitecture,
                       "PPOActorNetworkParameters": PPOActorArchitecture,
                       "PPOCriticNetworkParameters": PPOCriticArchitecture,
                       "ACERNetworkParameters": ACERArchitecture,
                       "ActorCriticNetworkParameters": ActorCriticArchitecture,
                       "NStepQNetworkParameters": NStepQArchitecture,
                       "SACPolicyNetworkParameters": SACPolicyArchitecture,
                       "SACCriticNetworkParameters": SACQArchitecture,
                       "SACValueNetworkParameters": SACValueArchitecture,
                       "ClippedPPONetworkParameters": PPOArchitecture}


def _family_of(network_parameters):
    """The family is decided by the class of `agent_parameters.network_wrappers[name]`, as
    GeneralTensorFlowNetwork decides by the head parameter classes it is given."""
    from .head_parameters import ClassificationHeadParameters
    heads = list(getattr(network_parameters, "heads_parameters", ()) or ())
    if len(heads) == 1 and isinstance(heads[0], ClassificationHeadParameters):
        return ClassificationArchitecture               # a wrapper of any class under a ClassificationHead
    for cls in type(network_parameters).__mro__:
        if cls.__name__ in _BY_PARAMETER_CLASS:
            return _BY_PARAMETER_CLASS[cls.__name__]
        if "Actor" in cls.__name__:
            return ActorArchitecture
        if "Critic" in cls.__name__:
            return CriticArchitecture
    return QArchitecture
