"""Device-resident networks of the hot-path agents, assembled from nn.graph layers.

Topologies follow rl_coach/architectures/tensorflow_components:
  embedders/image_embedder.py:57-63   Medium = conv 32x8x8/4, 64x4x4/2, 64x3x3/1
  embedders/vector_embedder.py:51-60  Medium = Dense 256, Shallow = Dense 128
  middlewares/fc_middleware.py:40-52  Medium = Dense 512, Shallow = Dense 64
  heads/q_head.py, v_head.py:43-48 (normalized-columns init, std 1.0), ppo_head.py:100-116
and the per-agent network parameters (agents/dqn_agent.py:43-56, clipped_ppo_agent.py:41-58).
"""
import numpy as np
import torch

from .. import _rlx
from ..architectures.head_parameters import DuelingQHeadParameters
from . import graph as G

IMAGE_EMBEDDER = {"Medium": [(32, 8, 4), (64, 4, 2), (64, 3, 1)], "Shallow": [(32, 3, 1)]}
VECTOR_EMBEDDER = {"Medium": [256], "Shallow": [128], "Empty": []}
FC_MIDDLEWARE = {"Medium": [512], "Shallow": [64], "Empty": []}


def build_torso(params, prefix, obs_shape, activation, towers, embedder="Medium", middleware="Medium", noisy=False):
    """input embedder + FC middleware.  obs_shape (H, W, C) -> image embedder on uint8 frames
    (input / 255, embedder_parameters.py:33-36), (D,) -> vector embedder.
    noisy: every dense layer is a factorised NoisyNet layer (G.NoisyDense; the convolutions stay)."""
    layers = []
    Dense = G.NoisyDense if noisy else G.Dense
    if len(obs_shape) == 3:
        hwc = tuple(obs_shape)
        convs = IMAGE_EMBEDDER[embedder] if isinstance(embedder, str) else embedder
        for i, (f, k, s) in enumerate(convs):
            c = G.Conv2d(params, "%s/embedder/conv%d" % (prefix, i), hwc, f, k, s, activation, towers)
            layers.append(c)
            hwc = c.out_hwc
        feat = hwc[0] * hwc[1] * hwc[2]
    else:
        feat = int(obs_shape[0])
        dense = VECTOR_EMBEDDER[embedder] if isinstance(embedder, str) else embedder
        for i, u in enumerate(dense):
            layers.append(Dense(params, "%s/embedder/dense%d" % (prefix, i), feat, u, activation, towers))
            feat = u
    mids = FC_MIDDLEWARE[middleware] if isinstance(middleware, str) else middleware
    for i, u in enumerate(mids):
        layers.append(Dense(params, "%s/middleware/dense%d" % (prefix, i), feat, u, activation, towers))
        feat = u
    return G.Sequential(layers), feat


class _NetBase:
    def _finish(self, device, seed, lr, beta1, beta2, eps, has_target=True):
        self.device = device
        self.params.finalize(device)
        rng = np.random.RandomState(seed)
        for m in self.modules:
            m.initialize(rng)
        self.ctx = G.Context(device)
        self.lib = self.ctx.lib
        self.adam = G.AdamState(self.params, lr, beta1, beta2, eps)
        if has_target:
            self.target = self.params.target_weights
            self.target.copy_(self.params.weights)
        else:
            self.target = None
        self.norm = torch.zeros(1, dtype=torch.float32, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)

    def obs_tensor(self, obs, B):
        if self.image:
            return G.input_tensor(obs, B, int(np.prod(self.obs_shape)), u8=True, div=255.0)
        return G.input_tensor(obs, B, int(self.obs_shape[0]))

    # ---- the single-tower networks: one embedder + FC middleware trunk under one or more Dense heads -------------
    def _build_trunk(self, obs_shape, activation, embedder, middleware):
        """the constructor's prologue: the observation's shape, the flat parameters and the one-tower torso -> the width
        of the torso's output, which the heads read"""
        self.obs_shape, self.image = tuple(obs_shape), len(obs_shape) == 3
        self.params = G.FlatParams()
        self.torso, feat = build_torso(self.params, "main", obs_shape, activation, 1, embedder, middleware)
        return feat

    def trunk_forward(self, obs, B, tag, weights=None):
        """the torso on obs -> its activations; the heads read the last one"""
        return self.torso.forward(self.ctx, self.obs_tensor(obs, B), tag=tag, weights=weights)

    def _fork(self, feat, heads, tag):
        """a training pass's [(head layer, the Tensor it reads)]: the first head reads feat, every other head a Tensor
        on the same data whose gradient is a buffer of its own (_heads_backward adds them onto feat.grad)"""
        feat.ensure_grad()
        pairs = [(heads[0], feat)]
        for l in heads[1:]:
            side = G.Tensor(feat.data, feat.rows, feat.cols, 1, act=feat.act)
            side.grad = self.ctx.buffer(l.name + "/input:grad", tuple(feat.data.shape), tag=tag)
            pairs.append((l, side))
        return pairs

    def _heads_forward(self, pairs, tag, weights=None):
        """[(head layer, input Tensor)] -> [output Tensor]: the layers the narrow-dense kernels serve in ONE launch
        (where there is more than one), the others as launches of their own"""
        narrow = [p for p in pairs if p[0].N <= G.SMALL_N]
        out = {}
        if len(narrow) > 1:
            ys = G.small_dense_forward_multi(self.ctx, narrow, tag=tag, weights=weights)
            out = {l: y for (l, _), y in zip(narrow, ys)}
        return [out[l] if l in out else l.forward(self.ctx, x, tag=tag, weights=weights) for l, x in pairs]

    def _heads_backward(self, feat, pairs, outs):
        """the heads' backward pass behind _fork and _heads_forward (every output's .grad is set): the narrow layers in
        ONE launch where it takes their rows, the others as launches of their own; then the side gradients are added
        onto feat.grad in head order"""
        items = [(l, x, y) for (l, x), y in zip(pairs, outs)]
        narrow = [it for it in items if it[0].N <= G.SMALL_N and feat.rows * it[0].N <= 1024]
        together = set()
        if len(narrow) > 1:
            G.small_dense_backward_multi(self.ctx, narrow)
            together = {l for l, _, _ in narrow}
        for l, x, y in items:
            if l not in together:
                l.backward(self.ctx, x, y)
        g = feat.grad
        for _, x in pairs[1:]:
            self.lib.axpby(g, 1.0, g, 1.0, x.grad, g.numel(), self.ctx.stream)
        feat.grad_is_dz = all(x.grad_is_dz for _, x in pairs)

    def update_target(self, rate=1.0):
        """NetworkWrapper.update_target_network (network_wrapper.py:109-116): w_t <- rate*w_o + (1-rate)*w_t."""
        self.lib.mix_weights(self.target, self.params.weights, self.params.size, float(rate), self.ctx.stream)

    def grad_norm(self):
        self.lib.global_norm(self.params.grads, self.params.size, self.norm, self.ctx.ws.small,
                             self.ctx.ws.small.numel(), self.ctx.stream)
        return self.norm

    def apply_gradients(self, grad_scale=1.0, with_norm=False, acc=None, mix_rate=None):
        """Adam; with_norm also refreshes self.norm = tf.global_norm(grads) in the same pass; mix_rate (a soft
        target update is due right after this step): the target weights are mixed in the same pass."""
        kw = {}
        if mix_rate is not None and self.target is not None and self.adam.one_launch:
            kw = dict(mix_target=self.target, mix_rate=float(mix_rate))
        elif mix_rate is not None and self.target is not None:
            kw = {}
        if with_norm:
            self.adam.step(grad_scale, norm_out=self.norm, workspace=self.ctx.ws.small, acc=acc, **kw)
        else:
            self.adam.step(grad_scale, **kw)
        if mix_rate is not None and self.target is not None and not kw:
            self.update_target(mix_rate)
        for bn in getattr(self, "bn_layers", ()):          # UPDATE_OPS of apply_gradients (architecture.py:273-277)
            bn.commit(self.ctx)

    def set_is_training(self, state):
        """NetworkWrapper.set_is_training (network_wrapper.py:215-224): batch-norm layers use batch statistics."""
        self.ctx.bn_training = bool(state)

    clip_gradients = None

    def clip_by_global_norm(self):
        """clip_gradients (ClipByGlobalNorm, architecture.py:196-200): self.norm <- tf.global_norm of
        the raw gradients, then the gradient buffer is rescaled in place.  False when clipping is off."""
        if not self.clip_gradients:
            return False
        self.grad_norm()
        self.lib.clip_by_global_norm(self.params.grads, self.params.size, self.norm,
                                     float(self.clip_gradients), self.ctx.stream)
        return True

    def check_status(self):
        s = int(self.status.item())
        if s:
            self.status.zero_()
            raise ValueError("device kernel reported invalid input (status bits %d)" % s)


class ClippedPPONet(_NetBase):
    """ClippedPPONetworkParameters (agents/clipped_ppo_agent.py:41-58): two full copies of
    embedder + middleware (use_separate_networks_per_head), head 0 = VHead, head 1 = PPOHead
    (discrete).  tower 0 = value, tower 1 = policy."""
    HEADS_LOSS_BACKWARD_ONE_LAUNCH = True     # discrete heads: losses + heads' backward as one launch (tests flip it)
    HEADS_FORWARD_WITH_TORSO = True           # the heads' forward inside the last dense layer's split-K reduction (tests flip it)
    # the last dense layer of both towers + heads forward + both losses + heads backward as ONE launch (rlx_ppo_fc_heads,
    # csrc/ppo_fc_fused.hip) where the shape allows it (discrete heads, minibatch <= 64 rows).  OFF: measured on C2 it is
    # 34.8 us against 11.0 + 8.0 + 11.2 us for the three launches it replaces (1 MB of split-K partials instead of 6.5 MB, 10
    # launches per update instead of 12) and the update comes out 198.1 us against 193.8 us (same box, bench.py --fc-heads
    # 1 / 0, profiles/r06_ab_fc_heads.txt): its three in-launch hand-offs (8 K splits -> tile, 16 tiles -> tower, dy back to
    # the tiles) each cost a write-through + read round trip, which is what a launch boundary costs here.  Entry point,
    # parity test (tests/test_ppo_fc_fused.py) and A/B flag stay.
    FC_HEADS_ONE_LAUNCH = False
    # discrete heads, minibatch <= 256 rows: what of the heads' losses and backward pass is LOCAL TO A ROW (heads forward, the
    # row's loss terms, dV / dlogits, dz of the last dense layer) runs in the workgroup that finishes that row of the dense
    # layer's K-split reduction (rlx_ppo_fc_rows), and the rest — dW / db of the heads, the loss scalars, which nobody reads
    # before the Adam step — as extra workgroups of the backward pass's deferred-reduction launch
    # (rlx_splitk_reduce_jobs_ppo_tail): the heads' launch (11.3 us of the C2 update, tens of workgroups) disappears from
    # the chain.  Bit-identical to the three-launch path (tests/test_ppo_fc_rows.py); tests and bench.py --heads-row-local flip it.
    HEADS_ROW_LOCAL = True

    def __init__(self, device, obs_shape, n_actions, activation="tanh", embedder="Medium",
                 middleware="Medium", learning_rate=2.5e-4, adam_beta1=0.9, adam_beta2=0.99,
                 optimizer_epsilon=1e-4, clip_likelihood_ratio_using_epsilon=0.2, beta_entropy=0.01,
                 seed=0, continuous=False):
        """continuous: n_actions is the action dimension; the head is ppo_head.py:118-144 (policy_mean
        Dense with normalized-columns(0.01) init + one state-independent policy_log_std vector)."""
        self.obs_shape, self.image, self.A = tuple(obs_shape), len(obs_shape) == 3, n_actions
        self.clip_eps, self.beta = clip_likelihood_ratio_using_epsilon, beta_entropy
        self._clip_scale_dev, self._clip_scale_value = None, None
        self.continuous = continuous
        # (heads forward / losses / heads backward as ONE launch was tried twice and lost to these three small grids:
        # profiles/r02_ab_fused_heads.txt)
        self.params = G.FlatParams()
        self.torso, feat = build_torso(self.params, "main", obs_shape, activation, 2, embedder, middleware)
        self.v_head = G.Dense(self.params, "main/v_head/dense", feat, 1, None, 1,
                              init=G.normalized_columns(1.0))                   # v_head.py:43-48
        if continuous:
            self.pi_head = G.Dense(self.params, "main/ppo_head/policy_mean", feat, n_actions, None, 1,
                                   init=G.normalized_columns(0.01))
            self.params.add_group([("main/ppo_head/policy_log_std", (n_actions,))])   # zeros (:133-137)
        else:
            self.pi_head = G.Dense(self.params, "main/ppo_head/policy_fc", feat, n_actions, None, 1)
        self.modules = [self.torso, self.v_head, self.pi_head]
        self._finish(device, seed, learning_rate, adam_beta1, adam_beta2, optimizer_epsilon)
        # [surrogate, entropy, kl, policy-head total, value loss, grad norm]: one contiguous record
        self.scalars = torch.zeros(8, dtype=torch.float32, device=device)
        self.norm = self.scalars[5:6]

    # ---- inference -------------------------------------------------------------------------
    def policy_probs(self, obs, B, use_target=False, tag="act", out=None, sample=None):
        """softmax(policy_fc(policy tower(obs)))  — target weights = the frozen 'old policy'.
        sample=(uniforms [B] fp64, actions [B] int32 out): draw the actions in the same launch and return None."""
        w = self.target if use_target else None
        if self.HEADS_FORWARD_WITH_TORSO and self.pi_head.N <= G.SMALL_N and self.torso.layers[-1].N > G.SMALL_N:
            acts, (logits,) = self.torso.forward(self.ctx, self.obs_tensor(obs, B), tag=tag, weights=w, t0=1, nt=1,
                                                 row_heads=[(self.pi_head, 0)])
        else:
            acts = self.torso.forward(self.ctx, self.obs_tensor(obs, B), tag=tag, weights=w, t0=1, nt=1)
            logits = self.pi_head.forward(self.ctx, acts[-1], tag=tag, weights=w)
        if sample is not None:
            # acting: the categorical draw in the softmax launch (rlx_softmax_categorical_sample); the probabilities
            # themselves are not needed by anyone
            uniforms, actions = sample
            self.lib.softmax_categorical_sample(logits.data, self.A, uniforms, B, self.A, None, 0, actions, self.ctx.stream)
            return None
        probs = out if out is not None else self.ctx.buffer("probs", (B, self.A), tag=tag)
        self.lib.softmax(logits.data, self.A, B, self.A, probs, self.A, self.ctx.stream)
        return probs

    def act_and_record(self, obs, B, uniforms, actions, value_out, probs_out, tag="actrec"):
        """One acting step of the discrete agent that also leaves what the training phase needs from these states:
        BOTH towers run (the forward of forward_backward, launch for launch), the categorical draw happens in the softmax
        launch as in policy_probs(sample=...), V(s) goes to value_out [B] and the action probabilities to probs_out
        [B, A] — rows of the rollout's own columns.  The weights do not change between a rollout's steps and its training
        phase, and the old policy of that phase IS the acting policy (networks['main'].sync() at its start,
        clipped_ppo_agent.py:326), so fill_advantages' pass over the whole dataset (:161-170) and the old-policy pass
        (:238-241) recompute exactly these numbers: with them recorded here both passes disappear."""
        ctx = self.ctx
        fused_heads = self.pi_head.N <= G.SMALL_N and B * self.pi_head.N <= 1024
        if fused_heads and self.HEADS_FORWARD_WITH_TORSO and self.torso.layers[-1].N > G.SMALL_N:
            acts, (v, logits) = self.torso.forward(ctx, self.obs_tensor(obs, B), tag=tag,
                                                   row_heads=[(self.v_head, 0, value_out), (self.pi_head, 1)])
        else:
            acts = self.torso.forward(ctx, self.obs_tensor(obs, B), tag=tag)
            mid = acts[-1]
            if fused_heads:
                v, logits = G.small_dense_forward_multi(ctx, [(self.v_head, mid.tower_view(0)), (self.pi_head, mid.tower_view(1))], tag=tag)
            else:
                v = self.v_head.forward(ctx, mid.tower_view(0), tag=tag)
                logits = self.pi_head.forward(ctx, mid.tower_view(1), tag=tag)
            value_out.copy_(v.data.view(-1))
        self.lib.softmax_categorical_sample(logits.data, self.A, uniforms, B, self.A, probs_out, self.A, actions, ctx.stream)

    def policy_mean_std(self, obs, B, use_target=False, tag="act", out_mean=None, out_std=None):
        """Continuous head outputs [policy_mean, policy_std] (ppo_head.py:139-144): std = exp(log_std)
        tiled over the batch (the +eps is added where the distribution is built)."""
        w = self.target if use_target else None
        acts = self.torso.forward(self.ctx, self.obs_tensor(obs, B), tag=tag, weights=w, t0=1, nt=1)
        mean = self.pi_head.forward(self.ctx, acts[-1], tag=tag, weights=w).data.view(B, self.A)
        std = out_std if out_std is not None else self.ctx.buffer("policy_std", (B, self.A), tag=tag)
        ls = self.params.w("main/ppo_head/policy_log_std", 0, w)
        self.lib.exp_rows(ls, std, B, self.A, self.ctx.stream)
        if out_mean is not None:
            out_mean.copy_(mean)
            mean = out_mean
        return mean, std

    def values(self, obs, B, tag="val", out=None):
        """V(s) from the value tower of the online network (fill_advantages :161-170)."""
        if self.HEADS_FORWARD_WITH_TORSO and self.torso.layers[-1].N > G.SMALL_N:
            acts, (v,) = self.torso.forward(self.ctx, self.obs_tensor(obs, B), tag=tag, t0=0, nt=1,
                                            row_heads=[(self.v_head, 0)])
        else:
            acts = self.torso.forward(self.ctx, self.obs_tensor(obs, B), tag=tag, t0=0, nt=1)
            v = self.v_head.forward(self.ctx, acts[-1], tag=tag)
        if out is not None:
            out.copy_(v.data.view(-1))
            return out
        return v.data.view(-1)

    # ---- one minibatch of ClippedPPOAgent.train_network (:226-266) ---------------------------
    def late_gradient_offset(self):
        """Offset in the flat buffers where the parameters whose gradients are produced FIRST in the
        backward pass start (FC middleware + heads: 95 % of the bytes).  [offset, size) can be
        all-reduced while the convolution gradients [0, offset) are still being computed."""
        return self.params.entries[self.torso.layers[self._split_layer()].kname][0]

    def _split_layer(self):
        from .graph import Conv2d
        for i, l in enumerate(self.torso.layers):
            if not isinstance(l, Conv2d):
                return i
        return 0

    def set_clip_rescaler(self, value):
        """clip_param_rescaler (clipped_ppo_agent.py:266-268) as a DEVICE scalar: forward_backward(clip_rescaler=None)
        then multiplies the clip range by it inside the loss kernel, so a captured graph serves every value of a
        decaying clipping_decay_schedule."""
        if self._clip_scale_dev is None:
            self._clip_scale_dev = torch.ones(1, dtype=torch.float32, device=self.device)
        if self._clip_scale_value != float(value):
            self._clip_scale_dev.fill_(float(value))
            self._clip_scale_value = float(value)

    def forward_backward(self, obs, B, actions, advantages, value_targets, old_probs,
                         clip_rescaler=1.0, ratio_out=None, clipped_out=None, stop_after_dense=False):
        """accumulate_gradients (tensorflow_components/architecture.py:312-385): forward both towers,
        head losses, backward; leaves d total_loss / d theta in params.grads.
        stop_after_dense: stop once the dense layers' gradients are final (backward_rest() resumes).
        clip_rescaler None: the device scalar of set_clip_rescaler."""
        ctx = self.ctx
        clip_dev = self._clip_scale_dev if clip_rescaler is None else None
        if clip_rescaler is None:
            assert clip_dev is not None, "set_clip_rescaler first"
            clip_rescaler = 1.0
        fused_heads = self.pi_head.N <= G.SMALL_N and B * self.pi_head.N <= 1024
        heads_with_torso = fused_heads and self.HEADS_FORWARD_WITH_TORSO and self.torso.layers[-1].N > G.SMALL_N
        discrete_fused = heads_with_torso and not self.continuous and self.HEADS_LOSS_BACKWARD_ONE_LAUNCH
        if (self.FC_HEADS_ONE_LAUNCH or (self.HEADS_ROW_LOCAL and B <= 256)) and discrete_fused:
            acts = self.torso.forward(ctx, self.obs_tensor(obs, B), tag="train", skip_last=True)
            if self.HEADS_ROW_LOCAL and B <= 256 and not self.FC_HEADS_ONE_LAUNCH and len(acts) == len(self.torso.layers):
                res = G.ppo_fc_rows(ctx, self.torso.layers[-1], acts[-1], self.v_head, self.pi_head, value_targets, actions,
                                    advantages, old_probs, self.A, self.clip_eps * clip_rescaler, clip_dev, self.beta,
                                    self.scalars, ratio_out, clipped_out, self.status, tag="train",
                                    tail_now=stop_after_dense)
                if res is not None:
                    acts.append(res[0])
                    return self._backward_torso(acts, stop_after_dense)
            if self.FC_HEADS_ONE_LAUNCH and len(acts) == len(self.torso.layers) and \
                    G.ppo_fc_heads_supported(ctx, self.torso.layers[-1], acts[-1], self.v_head, self.pi_head):
                mid, v, logits = G.ppo_fc_heads(ctx, self.torso.layers[-1], acts[-1], self.v_head, self.pi_head, value_targets,
                                                actions, advantages, old_probs, self.A, self.clip_eps * clip_rescaler, clip_dev,
                                                self.beta, self.scalars, ratio_out, clipped_out, self.status, tag="train")
                acts.append(mid)
                return self._backward_torso(acts, stop_after_dense)
            # (not this shape: the layer-by-layer path below recomputes nothing — acts holds the layers in front of the last)
            last = self.torso.layers[-1]
            if heads_with_torso:
                y, (v, logits) = last.forward(ctx, acts[-1], tag="train", row_heads=[(self.v_head, 0), (self.pi_head, 1)])
            else:
                y = last.forward(ctx, acts[-1], tag="train")
            acts.append(y)
        elif heads_with_torso:   # the heads' forward rides on the last dense layer's launch (rlx_gemm_desc.row_heads)
            acts, (v, logits) = self.torso.forward(ctx, self.obs_tensor(obs, B), tag="train",
                                                   row_heads=[(self.v_head, 0), (self.pi_head, 1)])
        else:
            acts = self.torso.forward(ctx, self.obs_tensor(obs, B), tag="train")
        mid = acts[-1]
        mid.ensure_grad()
        xv, xp = mid.tower(0), mid.tower(1)
        if heads_with_torso:
            pass
        elif fused_heads:      # value + policy head in one launch (forward here, backward below)
            v, logits = G.small_dense_forward_multi(ctx, [(self.v_head, xv), (self.pi_head, xp)], tag="train")
        else:
            v = self.v_head.forward(ctx, xv, tag="train")
            logits = self.pi_head.forward(ctx, xp, tag="train")
        one_launch = fused_heads and not self.continuous and B <= 256 and self.HEADS_LOSS_BACKWARD_ONE_LAUNCH
        if one_launch:         # both head losses + the heads' backward pass: rlx_ppo_heads_loss_backward
            G.ppo_heads_loss_backward(ctx, (self.v_head, xv, v), (self.pi_head, xp, logits), value_targets, actions,
                                      advantages, old_probs, self.A, self.clip_eps * clip_rescaler, clip_dev, self.beta,
                                      self.scalars, ratio_out, clipped_out, self.status)
        dv, dlogits = v.ensure_grad(), logits.ensure_grad()
        # head 0: VHead, MSE(target, V), loss weight 1 (head.py:172-181)
        if one_launch:
            pass                                                   # (done above)
        elif not self.continuous:
            # ... and head 1, the discrete PPOHead clipped surrogate (+ entropy bonus), in one launch
            self.lib.ppo_discrete_value_losses(logits.data, self.A, actions, advantages, old_probs, self.A, B,
                                               self.A, self.clip_eps * clip_rescaler, self.beta, 1.0, dlogits,
                                               self.A, self.scalars[0:4], ratio_out, clipped_out, self.status,
                                               v.data, value_targets, dv, self.scalars[4:5], clip_dev, ctx.stream)
        else:
            self.lib.regression_loss(v.data, 1, value_targets, 1, None, B, 1, 0, 1.0, 1.0, dv, 1,
                                     self.scalars[4:5], ctx.stream)
        # head 1: PPOHead clipped surrogate (+ entropy bonus)
        if self.continuous:
            old_mean, old_std = old_probs                          # [policy_mean, policy_std] of the old policy
            self.lib.ppo_continuous_loss(logits.data, self.A, self.params.w("main/ppo_head/policy_log_std"),
                                         actions, advantages, old_mean, old_std, self.A, B, self.A,
                                         self.clip_eps * clip_rescaler, self.beta, 1.0, dlogits, self.A,
                                         self.params.g("main/ppo_head/policy_log_std"), self.scalars[0:4],
                                         ratio_out, clipped_out, clip_dev, ctx.stream)

        if one_launch:
            pass
        elif fused_heads:
            G.small_dense_backward_multi(ctx, [(self.v_head, xv, v), (self.pi_head, xp, logits)])
        else:
            self.v_head.backward(ctx, xv, v)
            self.pi_head.backward(ctx, xp, logits)
        mid.grad_is_dz = xv.grad_is_dz and xp.grad_is_dz     # the heads wrote dz of the middleware
        self._backward_torso(acts, stop_after_dense)

    def _backward_torso(self, acts, stop_after_dense):
        ctx = self.ctx
        if stop_after_dense:
            k = self._split_layer()
            self.torso.backward(ctx, acts, layers=(k, len(self.torso.layers)))
            self._resume = (acts, k)
        else:
            self.torso.backward(ctx, acts)
        ctx.flush_ppo_tail()        # (no deferred-reduction launch took the heads' all-rows part along)

    def backward_rest(self):
        acts, k = self._resume
        if k > 0:
            self.torso.backward(self.ctx, acts, layers=(0, k))

    # ---- the Adam step of the dense torso layers under the convolution weight-gradient launch (G.EarlyAdam) ----
    def early_adam_ranges(self):
        """the flat-buffer ranges whose gradients are final before the convolution weight-gradient launch: the dense
        layers of an image torso (both towers' kernel and bias: one contiguous group each)"""
        if not self.image:
            return []
        return [l.group_range() for l in self.torso.layers if type(l) is G.Dense]

    def prepare_early_adam(self):
        """the split's device lists (call outside a stream capture) -> True if there is something to run early"""
        ranges = self.early_adam_ranges()
        return bool(ranges) and self.adam.prepare_early(ranges) is not None

    def arm_early_adam(self, grad_scale=1.0, prepare=True):
        """The forward_backward that follows may step the early ranges inside its convolution weight-gradient launch — it
        does if every range's product reports nothing outstanding; finish_update(grad_scale) then runs the rest.  The
        caller's decision (an agent that knows that nothing reduces or rescales the gradients in between); a
        forward_backward that nobody armed leaves every weight alone, as ever."""
        ranges = self.early_adam_ranges()
        self.ctx.early_adam = self.adam.arm_early(ranges, grad_scale, prepare=prepare) if ranges else None
        return self.ctx.early_adam is not None

    def disarm_early_adam(self):
        self.ctx.early_adam = None

    def finish_update(self, grad_scale=1.0, signal_acc=None):
        """apply_gradients (architecture.py:469-521): global norm fetch + Adam (+ the running sums of
        [surrogate, entropy, kl, policy total, value loss, grad norm] into signal_acc).  Behind an armed backward pass
        that ran the early blocks: the late launch (same result, bit for bit)."""
        acc = (self.scalars, signal_acc, 6) if signal_acc is not None else None
        ea, self.ctx.early_adam = self.ctx.early_adam, None
        if ea is not None and ea.done:
            if float(grad_scale) != ea.grad_scale:
                raise ValueError("finish_update(%r): the early part of this step ran with gradient scale %r"
                                 % (grad_scale, ea.grad_scale))
            self.adam.step_late(ea, self.norm, acc)
            return
        self.apply_gradients(grad_scale, with_norm=True, acc=acc)

    def train_minibatch(self, obs, B, actions, advantages, value_targets, old_probs,
                        clip_rescaler=1.0, grad_scale=1.0, ratio_out=None, clipped_out=None):
        self.forward_backward(obs, B, actions, advantages, value_targets, old_probs, clip_rescaler,
                              ratio_out, clipped_out)
        self.finish_update(grad_scale)
        # scalars: [surrogate, entropy, kl, policy head total, value loss]
        return self.scalars


def common_net_kwargs(np_, seed):
    """a network parameters object -> the constructor keywords every network here takes: the torso's schemes and
    activation, Adam's constants and the seed"""
    return dict(activation=np_.activation_function, embedder=np_.embedder_scheme, middleware=np_.middleware_scheme,
                learning_rate=np_.learning_rate, adam_beta1=np_.adam_optimizer_beta1, adam_beta2=np_.adam_optimizer_beta2,
                optimizer_epsilon=np_.optimizer_epsilon, seed=seed)


def discrete_policy_actions(n_actions):
    """the action count of a network under the discrete policy head, checked against what its loss launches serve"""
    A = int(n_actions)
    if not 1 <= A <= 18:
        raise ValueError("the discrete policy head serves 1 .. 18 actions (got %d)" % A)
    return A


def dqn_net_kwargs(np_, seed):
    """a DQN-family network's parameters object (DQNNetworkParameters and its subclasses) -> the keywords of DQNNet's
    constructor; `noisy` and a subclass's own arguments (atoms, heads) are the caller's."""
    head = np_.heads_parameters[0]
    return dict(common_net_kwargs(np_, seed), replace_mse_with_huber_loss=np_.replace_mse_with_huber_loss,
                dueling=isinstance(head, DuelingQHeadParameters), head_activation=head.activation_function,
                head_gradient_rescale=head.rescale_gradient_from_head_by_factor,
                clip_gradients=getattr(np_, "clip_gradients", None))


class DQNNet(_NetBase):
    """DQNNetworkParameters (agents/dqn_agent.py:43-56): embedder -> FC middleware -> QHead;
    MSE or Huber loss, importance weights from prioritized replay."""
    HEAD_FORWARD_WITH_TORSO = True     # image networks: the Q head's forward rides on the last dense layer's launch
    HEAD_LOSS_BACKWARD_ONE_LAUNCH = True   # the head's loss (TD targets, dQ) and its backward pass as one launch
    FUSED_MLP = True        # small MLPs: the whole update / the acting step as one launch (tests flip these to cross-check)
    FUSED_ACT = True

    def __init__(self, device, obs_shape, n_actions, activation="relu", embedder="Medium",
                 middleware="Medium", learning_rate=2.5e-4, adam_beta1=0.9, adam_beta2=0.99,
                 optimizer_epsilon=1e-4, replace_mse_with_huber_loss=True, seed=0, dueling=False,
                 head_activation="relu", head_gradient_rescale=1.0, clip_gradients=None, noisy=False):
        """noisy: ParameterNoise's network — every dense layer (embedder, middleware, head) is a G.NoisyDense."""
        self.obs_shape, self.image, self.A = tuple(obs_shape), len(obs_shape) == 3, n_actions
        self.huber = replace_mse_with_huber_loss
        self.dueling = dueling
        self.noisy = bool(noisy)
        self.head_gradient_rescale = float(head_gradient_rescale)
        self.clip_gradients = clip_gradients
        self.params = G.FlatParams()
        self.torso, feat = build_torso(self.params, "main", obs_shape, activation, 1, embedder, middleware,
                                       noisy=self.noisy)
        if dueling and self.noisy:
            # the same head from noisy layers: the two fc1 streams are layers of their own (a NoisyDense has one tower:
            # each stream draws its own noise), so the towers-of-one-launch and multi-problem shortcuts are declined
            hn = "main/dueling_q_values_head"
            self.v_fc = G.NoisyDense(self.params, hn + "/state_value/fc1", feat, 512, head_activation)
            self.a_fc = G.NoisyDense(self.params, hn + "/action_advantage/fc1", feat, 512, head_activation)
            self.v_out = G.NoisyDense(self.params, hn + "/state_value/fc2", 512, 1, None)
            self.a_out = G.NoisyDense(self.params, hn + "/action_advantage/fc2", 512, n_actions, None)
            self.modules = [self.torso, self.v_fc, self.a_fc, self.v_out, self.a_out]
        elif dueling:
            # DuelingQHead (heads/dueling_q_head.py:33-48): state-value and action-advantage streams,
            # each Dense(512, act) -> Dense(1 | A); the two fc1 layers are towers of one launch
            hn = "main/dueling_q_values_head"
            self.stream_fc = G.Dense(self.params, hn + "/fc1", feat, 512, head_activation, 2)
            self.v_out = G.Dense(self.params, hn + "/state_value/fc2", 512, 1, None, 1)
            self.a_out = G.Dense(self.params, hn + "/action_advantage/fc2", 512, n_actions, None, 1)
            self.modules = [self.torso, self.stream_fc, self.v_out, self.a_out]
        else:
            self.q_head = self._q_head_layer(feat, n_actions)
            self.modules = [self.torso, self.q_head]
        self._finish(device, seed, learning_rate, adam_beta1, adam_beta2, optimizer_epsilon)
        self.loss = torch.zeros(1, dtype=torch.float32, device=device)
        self.l2_norm = torch.zeros(1, dtype=torch.float32, device=device)
        mids = FC_MIDDLEWARE[middleware] if isinstance(middleware, str) else middleware
        self.embedder_layers = len(self.torso.layers) - len(mids)      # state_embedding: the output of the last of them
        self._noisy_setup()
        self._fused = self._fused_mlp_setup()
        self._act = self._act_setup()

    def _q_head_layer(self, feat, units):
        """the plain head's output layer (a subclass with its own initialisation builds its own)"""
        return (G.NoisyDense if self.noisy else G.Dense)(self.params, "main/q_head/dense", feat, units, None, 1)

    # ---------------------------------------------------------------- noisy layers (ParameterNoise)
    def _noisy_setup(self):
        """the network's noisy layers in forward order, their device counters [layer][pass] (int64, advanced by
        rlx_noisy_sample itself — part of a checkpoint) and the generator's key (the agent sets seed and rank)."""
        self.noisy_layers = [l for m in self.modules for l in (m.layers if isinstance(m, G.Sequential) else [m])
                             if isinstance(l, G.NoisyDense)]
        for i, l in enumerate(self.noisy_layers):
            l.index = i
        if len(self.noisy_layers) > _rlx.NOISY_MAX_LAYERS:      # (one sampling launch serves them all)
            raise ValueError("a noisy network may have at most %d dense layers (this one has %d)"
                             % (_rlx.NOISY_MAX_LAYERS, len(self.noisy_layers)))
        self.noise_seed, self.noise_rank = 0, 0
        self.noise_counters = torch.zeros(max(1, len(self.noisy_layers)) * _rlx.NOISY_PASSES, dtype=torch.int64,
                                          device=self.device) if self.noisy else None

    def sample_noise(self, tag, noise_pass):
        """fresh noise for the forward pass `tag` of every noisy layer: one launch; noise_pass (_rlx.NOISY_PASS) names
        the pass's own streams and counters.  No-op for a plain network."""
        if not self.noisy:
            return
        key = ("noisy_layers", tag)
        arr = self.ctx.cache.get(key)
        if arr is None:
            arr = (_rlx.NoisyLayer * len(self.noisy_layers))()
            for q, l in zip(arr, self.noisy_layers):
                q.f, q.f64, q.K, q.N, q.layer = l.noise(self.ctx, tag).data_ptr(), None, l.K, l.N, l.index
            self.ctx.cache[key] = arr
        import ctypes
        self.lib.noisy_sample(ctypes.byref(arr), len(arr), self.noise_counters, _rlx.NOISY_PASS[noise_pass],
                              self.noise_seed, self.noise_rank, self.ctx.stream)

    # ---------------------------------------------------------------- fused small-MLP update (one launch)
    def _small_mlp(self):
        """obs -> Dense(relu) -> Dense(relu) -> head (CartPole_DQN's shape), which the one-launch kernels of
        csrc/mlp_fused.hip take -> ((obs_dim, h1, h2), the six offsets of w1, b1, w2, b2, w3, b3 in the flat buffer),
        or None for any other network."""
        ls = self.torso.layers
        if self.image or self.dueling or len(ls) != 2 or \
                any(not isinstance(l, G.Dense) or l.act != "relu" or l.T != 1 for l in ls):
            return None
        offs = tuple(self.params.entries[n][0] for l in (ls[0], ls[1], self.q_head) for n in (l.kname, l.bname))
        return (ls[0].K, ls[0].N, ls[1].N), offs

    def _fused_mlp_setup(self):
        """small MLPs qualify for rlx_mlp_dqn_update: the whole learn_from_batch in ONE launch.
        DQNNet.FUSED_MLP = False keeps the layer-by-layer path (the tests cross-check the two)."""
        mlp = self._small_mlp() if self.FUSED_MLP else None
        if mlp is None or self.head_gradient_rescale != 1.0 or self.clip_gradients:
            return None
        dims, offs = mlp
        if not self.lib.rlx_mlp_dqn_supported(1, *dims, self.A):
            return None
        import ctypes
        n = ctypes.c_longlong()
        self.lib.mlp_dqn_workspace_floats(dims[1], dims[2], self.A, ctypes.byref(n))
        return dict(dims=dims, ws=torch.zeros(n.value, dtype=torch.float32, device=self.device),
                    sync=torch.zeros(4, dtype=torch.int32, device=self.device), offs=offs)

    def _act_setup(self):
        """the same network shape qualifies for rlx_mlp_q_act: Q(s) of a few envs + the epsilon-greedy choice as one
        launch (DQNNet.FUSED_ACT = False keeps the layer launches + rlx_egreedy)."""
        mlp = self._small_mlp() if self.FUSED_ACT else None
        if mlp is None or getattr(self.q_head, "act", None) is not None:
            return None
        return dict(dims=mlp[0], offs=mlp[1])

    def can_act_fused(self, n_env):
        a = self._act
        return a is not None and bool(self.lib.rlx_mlp_q_act_supported(int(n_env), *a["dims"], self.A))

    def q_act(self, states, n_env, explore_u, random_act, tie_rand, epsilon, q_out, actions, use_target=False):
        """q_out [n_env, A] = Q(states); actions = rlx_egreedy on them (actions None: values only)."""
        a = self._act
        w = self.target if use_target else self.params.weights
        self.lib.mlp_q_act(w, *a["offs"], states, int(n_env), *a["dims"], self.A, explore_u, random_act, tie_rand,
                           float(epsilon), q_out, actions, self.ctx.stream)

    def _fused_learn(self, obs, next_obs, B, actions, rewards, game_overs, discount, w, td_errors, double_dqn,
                     grad_scale):
        f = self._fused
        d = _rlx.MlpDqnDesc()
        d.weights, d.target_weights = self.params.weights.data_ptr(), self.target.data_ptr()
        d.adam_m, d.adam_v, d.adam_state = self.adam.m.data_ptr(), self.adam.v.data_ptr(), self.adam.state.data_ptr()
        d.states, d.next_states = obs.data_ptr(), next_obs.data_ptr()
        d.actions, d.rewards, d.game_overs = actions.data_ptr(), rewards.data_ptr(), game_overs.data_ptr()
        d.importance_weights = None if w is None else w.data_ptr()
        d.workspace, d.workspace_floats, d.sync_words = f["ws"].data_ptr(), f["ws"].numel(), f["sync"].data_ptr()
        d.loss_out, d.norm_out = self.loss.data_ptr(), self.norm.data_ptr()
        d.td_errors = None if td_errors is None else td_errors.data_ptr()
        d.status = self.status.data_ptr()
        d.off_w1, d.off_b1, d.off_w2, d.off_b2, d.off_w3, d.off_b3 = f["offs"]
        d.discount = float(discount)
        d.batch, (d.obs_dim, d.h1, d.h2), d.n_actions = int(B), f["dims"], self.A
        d.huber, d.double_dqn = int(self.huber), int(bool(double_dqn))
        a = self.adam
        d.learning_rate, d.beta1, d.beta2, d.epsilon, d.grad_scale = a.lr, a.beta1, a.beta2, a.eps, float(grad_scale)
        import ctypes
        self.lib.mlp_dqn_update(ctypes.byref(d), self.ctx.stream)
        return self.loss

    def _dueling_forward(self, feat, B, tag, weights=None, train=False):
        """-> (q Tensor [1, B, A], saved) ; saved = tensors the backward pass needs."""
        ctx = self.ctx
        if self.noisy:
            hv = self.v_fc.forward(ctx, feat, tag=tag, weights=weights)
            ha = self.a_fc.forward(ctx, feat, tag=tag, weights=weights)
            v = self.v_out.forward(ctx, hv, tag=tag, weights=weights)
            adv = self.a_out.forward(ctx, ha, tag=tag, weights=weights)
            qbuf = ctx.buffer("main/dueling_q_values_head/output", (1, B, self.A), tag=tag)
            self.lib.dueling_combine(v.data, adv.data, B, self.A, qbuf, ctx.stream)
            q = G.Tensor(qbuf, B, self.A, 1, grad_key=(ctx, "main/dueling_q_values_head/output", tag))
            return q, (None, None, hv, ha, v, adv)
        shared = G.Tensor(feat.data, feat.rows, feat.cols, 0, act=feat.act)      # one input, two streams
        h = self.stream_fc.forward(ctx, shared, tag=tag, weights=weights)
        hv, ha = (h.tower(0), h.tower(1)) if train else (h.tower_view(0), h.tower_view(1))
        if self.A <= G.SMALL_N:
            v, adv = G.small_dense_forward_multi(ctx, [(self.v_out, hv), (self.a_out, ha)], tag=tag,
                                                 weights=weights)
        else:
            v = self.v_out.forward(ctx, hv, tag=tag, weights=weights)
            adv = self.a_out.forward(ctx, ha, tag=tag, weights=weights)
        qbuf = ctx.buffer("main/dueling_q_values_head/output", (1, B, self.A), tag=tag)
        self.lib.dueling_combine(v.data, adv.data, B, self.A, qbuf, ctx.stream)
        q = G.Tensor(qbuf, B, self.A, 1, grad_key=(ctx, "main/dueling_q_values_head/output", tag))
        return q, (shared, h, hv, ha, v, adv)

    def _dueling_backward(self, feat, q, saved, B):
        ctx = self.ctx
        shared, h, hv, ha, v, adv = saved
        self.lib.dueling_combine_backward(q.grad, B, self.A, v.ensure_grad(), adv.ensure_grad(), ctx.stream)
        if self.noisy:
            self.v_out.backward(ctx, hv, v)
            self.a_out.backward(ctx, ha, adv)
            # the two streams' input gradients (each already times act'(feat)) add up in feat.grad
            side = G.Tensor(feat.data, feat.rows, feat.cols, 1, act=feat.act)
            side.grad = ctx.buffer("main/dueling_q_values_head/side:grad", tuple(feat.data.shape))
            self.v_fc.backward(ctx, feat, hv)
            self.a_fc.backward(ctx, side, ha)
            g = feat.grad
            self.lib.axpby(g, 1.0, g, 1.0, side.grad, g.numel(), ctx.stream)
            return
        if self.A <= G.SMALL_N and B * self.A <= 1024:
            G.small_dense_backward_multi(ctx, [(self.v_out, hv, v), (self.a_out, ha, adv)])
        else:
            self.v_out.backward(ctx, hv, v)
            self.a_out.backward(ctx, ha, adv)
        h.grad_is_dz = hv.grad_is_dz and ha.grad_is_dz
        shared.grad = feat.ensure_grad()
        self.stream_fc.backward(ctx, shared, h)
        feat.grad_is_dz = shared.grad_is_dz

    def q_values(self, obs, B, use_target=False, tag="q", noise_pass="act"):
        """noise_pass: which pass's noise a noisy network samples for this forward pass (every pass samples its own)."""
        w = self.target if use_target else None
        self.sample_noise(tag, noise_pass)
        acts = self.torso.forward(self.ctx, self.obs_tensor(obs, B), tag=tag, weights=w)
        if self.dueling:
            return self._dueling_forward(acts[-1], B, tag, w)[0]
        return self.q_head.forward(self.ctx, acts[-1], tag=tag, weights=w)

    l2_regularization = 0.0      # NetworkParameters.l2_regularization; read by _apply_update (the layer-by-layer update)

    def state_embedding(self, obs, B, tag="embed"):
        """the input embedder's output on obs, before the middleware (general_network.py's state_embedding[0]):
        fp32 [B, width] rows, valid until the next pass under the same tag"""
        acts = self.torso.forward(self.ctx, self.obs_tensor(obs, B), tag=tag)
        return acts[self.embedder_layers].data.view(B, -1)

    def _backward_from_q(self, acts, q, saved, B):
        ctx = self.ctx
        if self.dueling:
            self._dueling_backward(acts[-1], q, saved, B)
        else:
            self.q_head.backward(ctx, acts[-1], q)
        if self.head_gradient_rescale != 1.0:         # rescale_gradient_from_head_by_factor
            g = acts[-1].grad
            self.lib.axpby(g, self.head_gradient_rescale, g, 0.0, None, g.numel(), ctx.stream)
        self.torso.backward(ctx, acts)

    def accumulate_regression(self, obs, B, targets, importance_weights=None):
        """Architecture.accumulate_gradients for this network: forward, the head loss of head.py:143-186
        against explicit [B, A] targets, backward; leaves the gradients in params.grads (clipped when
        clip_gradients is set), the loss in self.loss and tf.global_norm of the raw gradients in self.norm."""
        ctx = self.ctx
        self.sample_noise("train", "online")
        acts = self.torso.forward(ctx, self.obs_tensor(obs, B), tag="train")
        saved = None
        if self.dueling:
            q, saved = self._dueling_forward(acts[-1], B, "train", train=True)
        else:
            q = self.q_head.forward(ctx, acts[-1], tag="train")
        self.lib.regression_loss(q.data, self.A, targets, self.A, importance_weights, B, self.A, int(self.huber),
                                 1.0, 1.0, q.ensure_grad(), self.A, self.loss, ctx.stream)
        self._backward_from_q(acts, q, saved, B)
        if not self.clip_by_global_norm():
            self.grad_norm()
        return self.loss

    def _online_and_target_forward(self, obs, next_obs, B, states_pair):
        """the target network on s' and the online network on s -> (acts, q, saved, q_next): the online pass as the
        backward pass needs it (saved: the dueling head's tensors, else None) and the target's head output [B, width]."""
        ctx, saved = self.ctx, None
        if states_pair is not None and not self.dueling and not self.noisy:
            # parallel_prediction (dqn_agent.py:86-89): online(s) and target(s') as two towers of the
            # same launches — the replay collates states / next_states into one [2, B, ...] buffer
            cols = int(np.prod(self.obs_shape))
            both = states_pair.view(2, B, cols)
            x = G.Tensor(both, B, cols, 2, u8=self.image, div=255.0 if self.image else 1.0)
            if self.HEAD_FORWARD_WITH_TORSO and self.A <= G.SMALL_N and self.q_head.T == 1 and \
                    self.torso.layers[-1].N > G.SMALL_N:
                # the Q head of both copies inside the last dense layer's split-K reduction (rlx_gemm_desc.row_heads)
                acts2, (q2,) = self.torso.forward(ctx, x, tag="pair", pair=True, row_heads=[(self.q_head, "pair")])
            else:
                acts2 = self.torso.forward(ctx, x, tag="pair", pair=True)
                q2 = self.q_head.forward(ctx, acts2[-1], tag="pair", pair=True)
            q_next = q2.data[1].view(B, -1)
            acts = [x.tower_view(0)] + [a.tower(0) for a in acts2[1:]]
            q = q2.tower(0)
        else:
            # (a noisy network takes this branch: the paired launches have no noisy form, and every pass samples its own
            # noise — target on s', online on s)
            q_next = self.q_values(next_obs, B, use_target=True, tag="next_t", noise_pass="target").data.view(B, -1)
            self.sample_noise("train", "online")
            acts = self.torso.forward(ctx, self.obs_tensor(obs, B), tag="train")
            if self.dueling:
                q, saved = self._dueling_forward(acts[-1], B, "train", train=True)
            else:
                q = self.q_head.forward(ctx, acts[-1], tag="train")
        return acts, q, saved, q_next

    def _apply_update(self, grad_scale, sync):
        """the gradients in params.grads -> the weights: clip, share between the workers, Adam."""
        if self.l2_regularization:
            # general_network.py:354-358: l2_regularization * sum over every weight of tf.nn.l2_loss (sum w^2 / 2) joins
            # the loss — its gradient, lambda * w, joins the flat gradient before clip and Adam; the loss signal gets the term
            lam, p = float(self.l2_regularization), self.params
            self.lib.axpby(p.grads, 1.0, p.grads, lam, p.weights, p.size, self.ctx.stream)
            self.lib.global_norm(p.weights, p.size, self.l2_norm, self.ctx.ws.small, self.ctx.ws.small.numel(),
                                 self.ctx.stream)
            self.loss.addcmul_(self.l2_norm, self.l2_norm, value=0.5 * lam)
        clipped = self.clip_by_global_norm()          # this worker's gradient, before it is shared
        if sync is not None:                          # data-parallel: ONE all-reduce of the flat buffer
            sync.all_reduce_sum(self.params.grads)
        self.apply_gradients(grad_scale, with_norm=not clipped)

    def _update(self, obs, next_obs, B, states_pair, grad_scale, sync, head_loss):
        """One update of every network of the family: the target's head output on s' and the online one on s (two towers
        of the same launches where the replay collated states_pair), head_loss(acts, q, saved, q_next, dq) — the
        class's own launch, which leaves the loss in self.loss and the head output's gradient in dq — backward, clip,
        Adam.  Passes that only the class's targets read (the online selector on s') run before this is called.
        head_loss returns true when its launch ran the head's backward pass as well (DQNNet's one-launch form)."""
        acts, q, saved, q_next = self._online_and_target_forward(obs, next_obs, B, states_pair)
        if not head_loss(acts, q, saved, q_next, q.ensure_grad()):
            self._backward_from_q(acts, q, saved, B)
        self._apply_update(grad_scale, sync)
        return self.loss

    def learn_from_batch(self, obs, next_obs, B, actions, rewards, game_overs, discount,
                         importance_weights=None, td_errors=None, double_dqn=False, grad_scale=1.0,
                         sync=None, states_pair=None, selector=None):
        """DQNAgent.learn_from_batch (agents/dqn_agent.py:81-113), all on device.
        selector: fp32 [B, A] (contiguous) whose row argmax picks the action the target network is evaluated at — the
        caller's own select_actions (DDQN-BCQ's masked online Q values, agents/ddqn_bcq_agent.py).  With it the update
        goes layer by layer (the one-launch small-MLP update computes its own selection) and double_dqn is not read."""
        ctx = self.ctx
        if selector is None and self._fused is not None and sync is None and B <= 32 and obs.is_contiguous() and \
                next_obs.is_contiguous():
            w = importance_weights
            if w is not None and w.dtype != torch.float64:
                w = w.double()
            return self._fused_learn(obs, next_obs, B, actions, rewards, game_overs, discount, w, td_errors,
                                     double_dqn, grad_scale)
        if selector is not None:
            if tuple(selector.shape) != (B, self.A) or selector.dtype != torch.float32 or not selector.is_contiguous():
                raise ValueError("selector is a contiguous fp32 [%d, %d] tensor" % (B, self.A))
            sel = selector
        else:
            sel = self.q_values(next_obs, B, tag="next_o", noise_pass="online_next").data.view(B, self.A) \
                if double_dqn else None

        def head_loss(acts, q, saved, q_next, dq):
            # TD targets, |TD errors|, QHead loss and its gradient in one launch (importance weights are
            # the fp64 weights of the prioritized replay, or fp32 -> converted, or None)
            w = importance_weights
            if w is not None and w.dtype != torch.float64:
                w = w.double()
            feat = acts[-1]
            if self.HEAD_LOSS_BACKWARD_ONE_LAUNCH and not self.dueling and self.head_gradient_rescale == 1.0 and \
                    self.q_head.T == 1 and self.A <= G.SMALL_N and B * self.A <= 1024 and B <= 256 and not feat.u8 and \
                    feat.towers == 1 and not self.noisy:
                # TD targets, |TD errors|, loss, dQ AND the Q head's backward pass (dW, db, dz of the last dense layer) in
                # one launch (rlx_dqn_head_loss_backward): what the two calls of the other branch compute, bit for bit
                import ctypes
                prob = _rlx.SmallDenseProblem()
                G._small_backward_problem(prob, self.q_head, feat, q)
                self.lib.dqn_head_loss_backward(ctypes.byref(prob), q.data, self.A, q_next, sel, self.A, actions, rewards,
                                                game_overs, w, float(discount), B, self.A, int(self.huber), 1.0, td_errors,
                                                self.loss, self.status, ctx.stream)
                self.torso.backward(ctx, acts)
                return True
            self.lib.dqn_head_loss(q.data, self.A, q_next, sel, self.A, actions, rewards, game_overs, w,
                                   float(discount), B, self.A, int(self.huber), 1.0, dq, self.A, td_errors,
                                   None, self.A, self.loss, self.status, ctx.stream)
        return self._update(obs, next_obs, B, states_pair, grad_scale, sync, head_loss)


class _OwnHeadLossDQNNet(DQNNet):
    """A DQN torso under a head with its own loss launch.  The fused small-MLP update computes DQN's targets, the fused
    acting kernel reduces DQN's head, and the head inside the torso's last launch is the plain Q head: all three are
    DQN's alone.  With these flags _fused and _act stay None and the head's forward is a launch of its own."""
    FUSED_MLP = False
    FUSED_ACT = False
    HEAD_FORWARD_WITH_TORSO = False


class DistributionalDQNNet(_OwnHeadLossDQNNet):
    """The DQN torso (vector or image) under a head that outputs N atoms per action: ONE Dense(feat, A * atoms) whose
    output column a * atoms + j is atom j of action a.  Forward and backward go through the torso's and the Dense
    layer's generic launches; what the atoms mean, and so the loss and its gradient, is the subclass's `_head_loss`
    (one launch, csrc/qr_dqn.hip or csrc/c51.hip; their shared parts: csrc/distributional_head.hpp)."""

    def __init__(self, device, obs_shape, n_actions, atoms, **kw):
        kw.pop("replace_mse_with_huber_loss", None)
        kw.pop("dueling", None)
        super().__init__(device, obs_shape, n_actions * atoms, dueling=False, **kw)
        self.A, self.N, self.AN = n_actions, int(atoms), n_actions * int(atoms)
        self.loss_ws = torch.zeros(256, dtype=torch.float32, device=device)      # per-row loss partials
        self.ticket = torch.zeros(1, dtype=torch.int32, device=device)

    def head_output(self, obs, B, use_target=False, tag="q", noise_pass="act"):
        """the head's Dense output [B, A * atoms] (a Tensor; .data is the buffer)."""
        return DQNNet.q_values(self, obs, B, use_target=use_target, tag=tag, noise_pass=noise_pass)

    def learn_from_batch(self, obs, next_obs, B, actions, rewards, game_overs, discount, grad_scale=1.0,
                         sync=None, states_pair=None, **head_outs):
        """the agents' learn_from_batch, all on device: the target's head output on s' and the online one on s (two
        towers of the same launches where the replay collated states_pair), _head_loss, backward, Adam.
        head_outs: the optional outputs of the subclass's _head_loss, by keyword."""
        def head_loss(acts, q, saved, q_next, dq):
            self._head_loss(q.data, q_next, dq, actions, rewards, game_overs, float(discount), B, **head_outs)
        return self._update(obs, next_obs, B, states_pair, grad_scale, sync, head_loss)


class QRDQNNet(DistributionalDQNNet):
    """QuantileRegressionDQNNetworkParameters (agents/qr_dqn_agent.py:28-33): a QuantileRegressionQHead
    (heads/quantile_regression_q_head.py:45-50); the quantile Huber loss and its gradient come from
    rlx_qr_dqn_head_loss (csrc/qr_dqn.hip)."""

    def __init__(self, device, obs_shape, n_actions, atoms, huber_loss_interval=1.0, **kw):
        super().__init__(device, obs_shape, n_actions, atoms, **kw)
        self.kappa = float(huber_loss_interval)

    quantiles = DistributionalDQNNet.head_output

    def _head_loss(self, q, q_next, dq, actions, rewards, game_overs, discount, B, targets_out=None, tau_out=None,
                   target_actions_out=None):
        """QuantileRegressionDQNAgent.learn_from_batch (agents/qr_dqn_agent.py:99-137): target action, TD targets,
        midpoints, loss, dtheta."""
        AN = self.AN
        self.lib.qr_dqn_head_loss(q, AN, q_next, AN, actions, rewards, game_overs, discount, self.kappa, self.N, self.A,
                                  B, 1.0, dq, AN, self.loss_ws, self.ticket, self.loss, self.status, targets_out,
                                  tau_out, target_actions_out, self.ctx.stream)


class C51Net(DistributionalDQNNet):
    """CategoricalDQNNetworkParameters (agents/categorical_dqn_agent.py:29-32): a CategoricalQHead
    (heads/categorical_q_head.py:42-47) whose outputs are logits; the softmaxes, the projection, the cross entropy and
    its gradient come from rlx_c51_head_loss (csrc/c51.hip)."""

    def __init__(self, device, obs_shape, n_actions, atoms, v_min=-10.0, v_max=10.0, **kw):
        super().__init__(device, obs_shape, n_actions, atoms, **kw)
        # the support, as the reference agent and head build it (fp64 on the host), uploaded once
        self.z_values = np.linspace(v_min, v_max, self.N)
        self.z = torch.from_numpy(self.z_values).to(device)

    distribution_logits = DistributionalDQNNet.head_output       # before the softmax

    def _head_loss(self, q, q_next, dq, actions, rewards, game_overs, discount, B, per_errors=None, m_out=None,
                   target_actions_out=None, action_losses_out=None):
        """CategoricalDQNAgent.learn_from_batch (agents/categorical_dqn_agent.py:104-167): target action, projection,
        cross entropy, dlogits, the taken action's cross entropy into per_errors."""
        AN = self.AN
        self.lib.c51_head_loss(q, AN, q_next, AN, self.z, actions, rewards, game_overs, discount, self.N, self.A, B, 1.0,
                               dq, AN, per_errors, self.loss_ws, self.ticket, self.loss, self.status, m_out,
                               target_actions_out, action_losses_out, self.ctx.stream)


class RainbowNet(_OwnHeadLossDQNNet):
    """RainbowDQNNetworkParameters (agents/rainbow_dqn_agent.py:32-36): the DQN torso under a RainbowQHead
    (heads/rainbow_q_head.py:38-70) — a state-value stream Dense(feat, 512, act) -> Dense(512, atoms) and an
    action-advantage stream Dense(feat, 512, act) -> Dense(512, A * atoms), four layers of their own (NoisyDense when the
    network is noisy: each draws its own noise).  The merge per atom, the softmaxes, the Double-DQN target action, the
    n-step projection, the cross entropy and the gradients of the two stream outputs come from rlx_rainbow_head_loss
    (csrc/rainbow.hip); acting reduces the two stream outputs with rlx_rainbow_argmax / rlx_rainbow_egreedy."""

    def __init__(self, device, obs_shape, n_actions, atoms, v_min=-10.0, v_max=10.0, **kw):
        kw.pop("replace_mse_with_huber_loss", None)
        kw.pop("dueling", None)
        self._head_shape = (int(n_actions), int(atoms), kw.get("head_activation", "relu"))
        super().__init__(device, obs_shape, n_actions * atoms, dueling=False, **kw)
        self.A, self.N, self.AN = n_actions, int(atoms), n_actions * int(atoms)
        self.loss_ws = torch.zeros(256, dtype=torch.float32, device=device)      # per-row loss partials
        self.ticket = torch.zeros(1, dtype=torch.int32, device=device)
        # the support, as the reference agent and head build it (fp64 on the host), uploaded once
        self.z_values = np.linspace(v_min, v_max, self.N)
        self.z = torch.from_numpy(self.z_values).to(device)

    def _q_head_layer(self, feat, units):
        """the head's four layers, in forward order (the constructor keeps them as one module: `q_head`)"""
        A, N, act = self._head_shape
        Dense = G.NoisyDense if self.noisy else G.Dense
        hn = "main/rainbow_q_values_head"
        self.v_fc = Dense(self.params, hn + "/state_value/fc1", feat, 512, act)
        self.v_out = Dense(self.params, hn + "/state_value/fc2", 512, N, None)
        self.a_fc = Dense(self.params, hn + "/action_advantage/fc1", feat, 512, act)
        self.a_out = Dense(self.params, hn + "/action_advantage/fc2", 512, A * N, None)
        return G.Sequential([self.v_fc, self.v_out, self.a_fc, self.a_out])

    def _streams_forward(self, feat, tag, weights=None):
        ctx = self.ctx
        hv = self.v_fc.forward(ctx, feat, tag=tag, weights=weights)
        ha = self.a_fc.forward(ctx, feat, tag=tag, weights=weights)
        return hv, ha, self.v_out.forward(ctx, hv, tag=tag, weights=weights), \
            self.a_out.forward(ctx, ha, tag=tag, weights=weights)

    def head_streams(self, obs, B, use_target=False, tag="q", noise_pass="act"):
        """-> (v, x): the two streams' Dense outputs, Tensors whose .data are [1, B, atoms] and [1, B, A * atoms]; every
        pass of a noisy network samples its own noise (noise_pass)."""
        w = self.target if use_target else None
        self.sample_noise(tag, noise_pass)
        acts = self.torso.forward(self.ctx, self.obs_tensor(obs, B), tag=tag, weights=w)
        return self._streams_forward(acts[-1], tag, w)[2:]

    def q_values(self, *args, **kw):
        raise NotImplementedError("RainbowNet has no Q-value output: head_streams and the rlx_rainbow_* reductions")

    def learn_from_batch(self, obs, next_obs, B, actions, n_step_returns, bootstrap, discount_n, grad_scale=1.0,
                         sync=None, per_errors=None, m_out=None, target_actions_out=None, action_losses_out=None,
                         merged_logits_out=None, dlogits_out=None):
        """RainbowDQNAgent.learn_from_batch (agents/rainbow_dqn_agent.py:88-137), all on device: the online network on
        s' (the Double-DQN choice), the target network on s', the online network on s, rlx_rainbow_head_loss, the
        backward pass through the four head layers into the torso, clip, Adam.  n_step_returns fp64 [B], bootstrap u8 [B]:
        the replay's two n-step columns; discount_n: the host's discount ** n_step."""
        ctx, N, AN = self.ctx, self.N, self.AN
        vn, xn = self.head_streams(next_obs, B, tag="next_o", noise_pass="online_next")
        vt, xt = self.head_streams(next_obs, B, use_target=True, tag="next_t", noise_pass="target")
        self.sample_noise("train", "online")
        acts = self.torso.forward(ctx, self.obs_tensor(obs, B), tag="train")
        feat = acts[-1]
        hv, ha, v, x = self._streams_forward(feat, "train")
        self.lib.rainbow_head_loss(v.data, N, x.data, AN, vt.data, N, xt.data, AN, vn.data, N, xn.data, AN, self.z,
                                   actions, n_step_returns, bootstrap, float(discount_n), N, self.A, B, 1.0,
                                   v.ensure_grad(), N, x.ensure_grad(), AN, per_errors, self.loss_ws, self.ticket,
                                   self.loss, self.status, m_out, target_actions_out, action_losses_out,
                                   merged_logits_out, dlogits_out, ctx.stream)
        self.v_out.backward(ctx, hv, v)
        self.a_out.backward(ctx, ha, x)
        # the two streams' input gradients (each already times act'(feat)) add up in feat.grad
        side = G.Tensor(feat.data, feat.rows, feat.cols, 1, act=feat.act)
        side.grad = ctx.buffer("main/rainbow_q_values_head/side:grad", tuple(feat.data.shape))
        self.v_fc.backward(ctx, feat, hv)
        self.a_fc.backward(ctx, side, ha)
        g = feat.grad
        self.lib.axpby(g, 1.0, g, 1.0, side.grad, g.numel(), ctx.stream)
        if self.head_gradient_rescale != 1.0:         # rescale_gradient_from_head_by_factor
            self.lib.axpby(g, self.head_gradient_rescale, g, 0.0, None, g.numel(), ctx.stream)
        self.torso.backward(ctx, acts)
        self._apply_update(grad_scale, sync)
        return self.loss


class _HeadCopiesDense(G.Dense):
    """Dense(feat, copies * units) whose column block h is copy h of a head's Dense(feat, units): every block is
    initialised as that layer of its own would be — glorot uniform with fan-out `units`, one draw per copy, in copy
    order (general_network.py builds num_output_head_copies heads, each with its own variables)."""

    def __init__(self, params, name, in_features, units, copies):
        super().__init__(params, name, in_features, units * copies, None, 1)
        self.units, self.copies = units, copies

    def initialize(self, rng):
        w = np.concatenate([G.xavier_uniform(rng, self.K, self.units, (self.K, self.units)) for _ in range(self.copies)],
                           axis=1)
        self.params.w(self.kname, 0).copy_(torch.from_numpy(np.ascontiguousarray(w)))


class BootstrappedDQNNet(_OwnHeadLossDQNNet):
    """BootstrappedDQNNetworkParameters (agents/bootstrapped_dqn_agent.py:26-30): the DQN torso under K copies of the
    QHead (num_output_head_copies), held as ONE Dense(feat, K * A) whose output column h * A + a is action a of head h;
    rescale_gradient_from_head_by_factor = 1 / K acts on what flows from the heads into the torso (the head's own
    weights get the full gradient).  Forward and backward go through the generic launches; the K masked losses and
    their gradient are one launch (rlx_bootstrapped_dqn_head_loss, csrc/bootstrapped_dqn.hip)."""
    MAX_HEADS = 32

    def __init__(self, device, obs_shape, n_actions, heads, dueling=False, noisy=False, **kw):
        if dueling or noisy:
            raise ValueError("Bootstrapped DQN has plain Q heads: the reference has neither a dueling nor a noisy form")
        heads = int(heads)
        if not 1 <= heads <= self.MAX_HEADS:
            raise ValueError("1 <= num_output_head_copies <= %d (a transition's mask is one 32-bit word), got %d"
                             % (self.MAX_HEADS, heads))
        self._heads, self._head_actions = heads, int(n_actions)
        super().__init__(device, obs_shape, n_actions * heads, dueling=False, noisy=False, **kw)
        self.A, self.K, self.KA = int(n_actions), heads, heads * int(n_actions)
        self.partials = torch.zeros(self.K * 256, dtype=torch.float32, device=device)    # per (head, row) loss terms
        self.ticket = torch.zeros(1, dtype=torch.int32, device=device)
        self.head_losses = torch.zeros(self.K, dtype=torch.float32, device=device)

    def _q_head_layer(self, feat, units):
        return _HeadCopiesDense(self.params, "main/q_head/dense", feat, self._head_actions, self._heads)

    def head_output(self, obs, B, use_target=False, tag="q"):
        """every head's Q values [B, K * A] (a Tensor; .data is the buffer)."""
        return DQNNet.q_values(self, obs, B, use_target=use_target, tag=tag)

    def learn_from_batch(self, obs, next_obs, B, actions, rewards, game_overs, masks, discount, grad_scale=1.0,
                         sync=None, states_pair=None, td_targets_out=None, target_actions_out=None):
        """BootstrappedDQNAgent.learn_from_batch (agents/bootstrapped_dqn_agent.py:57-86), all on device: online on
        s' (the selector), target on s' and online on s, the K masked head losses, backward, Adam.
        masks: int32 [B], bit h = the transition trains head h."""
        KA = self.KA
        sel = self.head_output(next_obs, B, tag="next_o").data.view(B, KA)

        def head_loss(acts, q, saved, q_next, dq):
            self.last_q, self.last_q_next, self.last_q_sel = q.data, q_next, sel     # (views of the pass's buffers)
            self.lib.bootstrapped_dqn_head_loss(q.data, KA, q_next, sel, KA, actions, rewards, game_overs, masks,
                                                float(discount), B, self.K, self.A, int(self.huber), 1.0, dq, KA,
                                                self.partials, self.ticket, self.loss, self.status, self.head_losses,
                                                td_targets_out, target_actions_out, self.ctx.stream)
        return self._update(obs, next_obs, B, states_pair, grad_scale, sync, head_loss)


class MixedTargetDQNNet(_OwnHeadLossDQNNet):
    """The DQN network (plain or dueling head) of the agents whose TD target mixes the Double-DQN target with other
    estimates: PALAgent (agents/pal_agent.py:70-111, the advantage-learning correction from the target network on s
    and the Monte Carlo return) and MixedMonteCarloAgent (agents/mmc_agent.py:57-83, the Monte Carlo return).  The
    passes are DQN's; the targets, the head's loss and its gradient are one launch (rlx_mixed_target_head_loss,
    csrc/pal.hip)."""
    MODES = ("pal", "mmc")

    def __init__(self, device, obs_shape, n_actions, noisy=False, **kw):
        if noisy:
            raise ValueError("noisy dense layers are not implemented for the PAL / Mixed Monte Carlo network")
        super().__init__(device, obs_shape, n_actions, noisy=False, **kw)

    def learn_from_batch(self, obs, next_obs, B, actions, rewards, game_overs, total_returns, discount, pal_alpha=0.9,
                         persistent=False, mixing_rate=0.1, mode="pal", grad_scale=1.0, sync=None, states_pair=None,
                         td_targets_out=None):
        """PALAgent / MixedMonteCarloAgent.learn_from_batch, all on device: online on s' (the selector), for PAL the
        target on s, target on s' and online on s, the mixed targets with loss and dQ, backward, Adam.
        total_returns: fp64 [B], the rows' n_step_discounted_rewards; td_targets_out: optional fp32 [B, A]."""
        if mode not in self.MODES:
            raise ValueError("mode is one of %s, got %r" % (self.MODES, mode))
        A = self.A
        sel = self.q_values(next_obs, B, tag="next_o", noise_pass="online_next").data.view(B, A)
        cur = self.q_values(obs, B, use_target=True, tag="cur_t", noise_pass="target").data.view(B, A) \
            if mode == "pal" else None

        def head_loss(acts, q, saved, q_next, dq):
            self.last_q, self.last_q_cur, self.last_q_next, self.last_q_sel = q.data, cur, q_next, sel    # (views)
            self.lib.mixed_target_head_loss(q.data, A, cur, q_next, sel, A, actions, rewards, game_overs, total_returns,
                                            float(discount), float(pal_alpha), int(bool(persistent)),
                                            float(mixing_rate), B, A, int(self.huber), 1.0, dq, A, td_targets_out, A,
                                            self.loss, self.status, self.ctx.stream)
        return self._update(obs, next_obs, B, states_pair, grad_scale, sync, head_loss)


class NAFNet(_NetBase):
    """NAFNetworkParameters (agents/naf_agent.py:34-43): vector embedder -> FC middleware -> NAFHead
    (heads/naf_head.py:45-86): three Dense layers on the middleware's output — V (1), mu_unscaled (A, the head's
    activation, then * output_scale) and l_vector (A(A+1)/2, a packed lower-triangular L with an exponentiated
    diagonal) — and Q = V - 1/2 ||L^T (u - mu)||^2.  The layers go through the generic launches (the multi-problem
    narrow-dense ones where their preconditions hold); the head's arithmetic, its loss and its gradient are one launch
    (rlx_naf_head_loss, csrc/naf.hip), acting and the signals use rlx_naf_head_forward."""
    MAX_ACTIONS = 32
    MAX_BATCH = 256
    HEAD = "main/naf_q_values_head"

    def __init__(self, device, obs_shape, action_dim, output_scale, activation="relu", embedder="Medium",
                 middleware="Medium", learning_rate=1e-3, adam_beta1=0.9, adam_beta2=0.99, optimizer_epsilon=1e-4,
                 replace_mse_with_huber_loss=False, head_activation="tanh", clip_gradients=None,
                 clip_by_value=False, seed=0):
        """clip_gradients with clip_by_value: GradientClippingMethod.ClipByValue (architecture.py:241-245) — every
        gradient clamped to [-clip_gradients, clip_gradients]; otherwise ClipByGlobalNorm as in the other networks."""
        if len(obs_shape) != 1:
            raise ValueError("NAF works only for continuous control problems (vector observations)")
        A = int(action_dim)
        if not 1 <= A <= self.MAX_ACTIONS:
            raise ValueError("1 <= action dimension <= %d (rlx_naf_head_loss), got %d" % (self.MAX_ACTIONS, A))
        self.A, self.NL = A, A * (A + 1) // 2
        self.huber = bool(replace_mse_with_huber_loss)
        self.clip_gradients, self.clip_value = clip_gradients, bool(clip_by_value)
        feat = self._build_trunk(obs_shape, activation, embedder, middleware)
        self.v_layer = G.Dense(self.params, self.HEAD + "/V", feat, 1, None, 1)
        self.mu_layer = G.Dense(self.params, self.HEAD + "/mu_unscaled", feat, A, head_activation, 1)
        self.l_layer = G.Dense(self.params, self.HEAD + "/l_vector", feat, self.NL, None, 1)
        self.heads = [self.v_layer, self.mu_layer, self.l_layer]
        self.modules = [self.torso] + self.heads
        self._finish(device, seed, learning_rate, adam_beta1, adam_beta2, optimizer_epsilon)
        self.scale = torch.as_tensor(np.broadcast_to(np.asarray(output_scale, dtype=np.float32), (A,)).copy(),
                                     device=device)
        self.loss = torch.zeros(1, dtype=torch.float32, device=device)
        self.partials = torch.zeros(self.MAX_BATCH, dtype=torch.float32, device=device)     # per-row loss terms
        self.ticket = torch.zeros(1, dtype=torch.int32, device=device)

    # ---------------------------------------------------------------------------------- forward
    def state_values(self, obs, B, use_target=False, tag="v"):
        """V(s) [B] (a view of the V layer's output)."""
        w = self.target if use_target else None
        acts = self.trunk_forward(obs, B, tag, w)
        return self.v_layer.forward(self.ctx, acts[-1], tag=tag, weights=w).data.view(B)

    def head_forward(self, obs, B, actions=None, use_target=False, tag="act", mu_out=None, with_signals=False):
        """-> dict(mu [B, A]) and, with_signals, Q [B], Advantage [B], L [B, A, A], V [B] of the head at `actions`
        (None: at u = mu, where Advantage = 0 and Q = V) — naf_agent.py:101-131."""
        ctx, A = self.ctx, self.A
        w = self.target if use_target else None
        acts = self.trunk_forward(obs, B, tag, w)
        v, m, l = (y.data for y in self._heads_forward([(k, acts[-1]) for k in self.heads], tag, w))
        mu = mu_out if mu_out is not None else ctx.buffer("naf/mu", (B, A), tag=tag)
        res = dict(mu=mu, V=v.view(B))
        q = adv = L = None
        if with_signals:
            q, adv = ctx.buffer("naf/q", (B,), tag=tag), ctx.buffer("naf/adv", (B,), tag=tag)
            L = ctx.buffer("naf/L", (B, A, A), tag=tag)
            res.update(Q=q, Advantage=adv, L=L)
        self.lib.naf_head_forward(v, 1, m, A, l, self.NL, self.scale, actions, A, B, A, mu, q, adv, L, ctx.stream)
        return res

    # --------------------------------------------------------------------------------- training
    def clip_by_value(self):
        """clip_gradients (ClipByValue, architecture.py:241-245): the flat gradient buffer clamped in place."""
        self.lib.clip_by_value(self.params.grads, self.params.size, float(self.clip_gradients), self.ctx.stream)

    def _apply_update(self, grad_scale, sync, mix_rate=None):
        """the gradients in params.grads -> the weights: clip, share between the workers, Adam (self.norm = the global
        norm of the unclipped gradients either way).  mix_rate: a soft target update is due right after this update —
        the Adam pass mixes the target where it can."""
        if self.clip_gradients and self.clip_value:
            self.grad_norm()
            self.clip_by_value()
            clipped = True
        else:
            clipped = self.clip_by_global_norm()
        if sync is not None:
            sync.all_reduce_sum(self.params.grads)
        self.apply_gradients(grad_scale, with_norm=not clipped, mix_rate=mix_rate)

    def learn_from_batch(self, obs, next_obs, B, actions, rewards, game_overs, discount, grad_scale=1.0, sync=None,
                         td_targets_out=None, q_out=None, adv_out=None, mix_rate=None):
        """NAFAgent.learn_from_batch (agents/naf_agent.py:80-99), all on device: the target network's V(s'), the
        online head on s, rlx_naf_head_loss (TD targets, Q, loss, dV / dmu_unscaled / dl_vector), the three layers'
        backward pass with their input gradients summed, the torso's backward pass, clip, Adam."""
        if not 1 <= B <= self.MAX_BATCH:
            raise ValueError("1 <= batch <= %d (rlx_naf_head_loss), got %d" % (self.MAX_BATCH, B))
        ctx, A, NL = self.ctx, self.A, self.NL
        v_next = self.state_values(next_obs, B, use_target=True, tag="next_t")
        acts = self.trunk_forward(obs, B, "train")
        fork = self._fork(acts[-1], self.heads, "train")
        v, m, l = outs = self._heads_forward(fork, "train")
        self.lib.naf_head_loss(v.data, 1, m.data, A, l.data, NL, self.scale, actions, A, v_next, 1, rewards, game_overs,
                               float(discount), B, A, int(self.huber), 1.0, v.ensure_grad(), 1, m.ensure_grad(), A,
                               l.ensure_grad(), NL, self.partials, self.ticket, self.loss, td_targets_out, q_out,
                               adv_out, ctx.stream)
        self._heads_backward(acts[-1], fork, outs)
        self.torso.backward(ctx, acts)
        self._apply_update(grad_scale, sync, mix_rate)
        return self.loss


def classification_net_kwargs(np_, seed):
    """a network wrapper whose single head is a ClassificationHeadParameters (Batch RL's imitation model) -> the keywords
    of ClassificationNet's constructor"""
    from ..architectures.head_parameters import ClassificationHeadParameters
    heads = list(np_.heads_parameters)
    if len(heads) != 1 or not isinstance(heads[0], ClassificationHeadParameters):
        raise ValueError("ClassificationNet serves a wrapper with exactly one ClassificationHeadParameters head, got %s"
                         % [type(h).__name__ for h in heads])
    return dict(common_net_kwargs(np_, seed), clip_gradients=getattr(np_, "clip_gradients", None),
                head_gradient_rescale=heads[0].rescale_gradient_from_head_by_factor,
                l2_regularization=float(getattr(np_, "l2_regularization", 0) or 0))


class ClassificationNet(_NetBase):
    """One embedder + FC middleware tower under a ClassificationHead (heads/classification_head.py): Dense(feat, A) named
    'output' whose values are the class logits; the head's output is their softmax.  No target copy.  The loss is the
    softmax cross entropy SUMMED over the batch (the head adds the per-row vector with tf.losses.add_loss and
    general_network.py:360 takes tf.reduce_sum), from rlx_classification_head_loss (csrc/imitation.hip); its softmax is
    the one rlx_bcq_imitation_selector applies to `logits`, so `predict` and the selector's familiarity are the same bits."""

    def __init__(self, device, obs_shape, n_actions, activation="relu", embedder="Medium", middleware="Medium",
                 learning_rate=2.5e-4, adam_beta1=0.9, adam_beta2=0.99, optimizer_epsilon=1e-4, clip_gradients=None,
                 head_gradient_rescale=1.0, l2_regularization=0.0, seed=0):
        self.A = discrete_policy_actions(n_actions)
        self.clip_gradients = clip_gradients
        self.head_gradient_rescale = float(head_gradient_rescale)
        self.l2_regularization = float(l2_regularization)
        feat = self._build_trunk(obs_shape, activation, embedder, middleware)
        self.head = G.Dense(self.params, "main/classification_head/output", feat, self.A, None, 1)
        self.modules = [self.torso, self.head]
        self._finish(device, seed, learning_rate, adam_beta1, adam_beta2, optimizer_epsilon, has_target=False)
        self.scalars = torch.zeros(2, dtype=torch.float32, device=device)     # the batch's summed loss, its correct rows
        self.loss, self.correct = self.scalars[0:1], self.scalars[1:2]
        self.l2_norm = torch.zeros(1, dtype=torch.float32, device=device)
        self._predict_scalars = torch.zeros(2, dtype=torch.float32, device=device)     # predict leaves self.loss alone
        self._probs = {}

    MAX_ROWS = 1024          # rlx_classification_head_loss: one workgroup, one row per thread

    def logits(self, obs, B, tag="logits"):
        """the head's Dense output [B, A] (a Tensor; .data is the buffer), valid until the next pass under the same tag"""
        return self.head.forward(self.ctx, self.trunk_forward(obs, B, tag)[-1], tag=tag)

    def _probs_buffer(self, B, tag):
        buf = self._probs.get((B, tag))
        if buf is None:
            buf = self._probs[(B, tag)] = torch.zeros(B, self.A, dtype=torch.float32, device=self.device)
        return buf

    def _head_loss(self, z, B, actions, labels, grad_scale, dz, probs, scalars=None):
        if (actions is None) == (labels is None):
            raise ValueError("exactly one of actions and labels is given")
        if not 1 <= B <= self.MAX_ROWS:
            raise ValueError("the classification head's loss launch serves 1 to %d rows, got %d" % (self.MAX_ROWS, B))
        if labels is not None and (tuple(labels.shape) != (B, self.A) or labels.dtype != torch.float32 or
                                   not labels.is_contiguous()):
            raise ValueError("labels is a contiguous fp32 [%d, %d] tensor" % (B, self.A))
        self.lib.classification_head_loss(z.data, self.A, actions, labels, self.A, float(grad_scale), B, self.A, dz,
                                          self.A, probs, self.A, None, self.scalars if scalars is None else scalars, self.status,
                                          self.ctx.stream)

    def predict(self, obs, B, tag="predict"):
        """the head's output: the class probabilities, fp32 [B, A] (softmax_row of the logits: the launch's probs_out)"""
        z = self.logits(obs, B, tag)
        probs = self._probs_buffer(B, tag)
        zeros = self._probs.get(B)                    # the launch wants a target: action 0 of every row, gradient scale 0
        if zeros is None:
            zeros = self._probs[B] = torch.zeros(B, dtype=torch.int32, device=self.device)
        self._head_loss(z, B, zeros, None, 0.0, z.ensure_grad(), probs, scalars=self._predict_scalars)
        return probs

    def accumulate_gradients(self, obs, B, actions=None, labels=None):
        """forward, the head loss against the actions (int32 [B]) or the dense target rows (fp32 [B, A]: the one-hot
        matrix the reference passes), backward: the gradients in params.grads (clipped when clip_gradients is set), the
        summed loss in self.loss, tf.global_norm of the raw gradients in self.norm"""
        ctx = self.ctx
        acts = self.trunk_forward(obs, B, "train")
        z = self.head.forward(ctx, acts[-1], tag="train")
        self._head_loss(z, B, actions, labels, 1.0, z.ensure_grad(), None)
        self.head.backward(ctx, acts[-1], z)
        if self.head_gradient_rescale != 1.0:         # rescale_gradient_from_head_by_factor
            g = acts[-1].grad
            self.lib.axpby(g, self.head_gradient_rescale, g, 0.0, None, g.numel(), ctx.stream)
        self.torso.backward(ctx, acts)
        if self.l2_regularization:                    # general_network.py:354-358, as DQNNet._apply_update
            lam, p = self.l2_regularization, self.params
            self.lib.axpby(p.grads, 1.0, p.grads, lam, p.weights, p.size, ctx.stream)
            self.lib.global_norm(p.weights, p.size, self.l2_norm, ctx.ws.small, ctx.ws.small.numel(), ctx.stream)
            self.loss.addcmul_(self.l2_norm, self.l2_norm, value=0.5 * lam)
        if not self.clip_by_global_norm():
            self.grad_norm()
        return self.loss

    def train_on_batch(self, obs, B, actions=None, labels=None, grad_scale=1.0, sync=None):
        """Architecture.train_on_batch: accumulate_gradients, then one Adam step"""
        self.accumulate_gradients(obs, B, actions=actions, labels=labels)
        if sync is not None:
            sync.all_reduce_sum(self.params.grads)
        self.apply_gradients(grad_scale)
        return self.loss


def policy_gradient_net_kwargs(np_, alg, seed):
    """PolicyGradientNetworkParameters + the algorithm's beta_entropy -> the keywords of PolicyGradientNet's constructor"""
    return dict(common_net_kwargs(np_, seed), clip_gradients=getattr(np_, "clip_gradients", None),
                beta_entropy=getattr(alg, "beta_entropy", 0) or 0)


class _WindowAccumulatingNet(_NetBase):
    """the on-policy networks' gradient accumulation (Architecture.accumulate_gradients / apply_and_reset_gradients): a
    subclass gives `window_gradients(...)`, which leaves one update window's gradients in params.grads and returns the
    loss; an update window's gradient is ADDED onto `accumulated`, which one Adam step consumes and clears."""

    def _finish_accumulating(self, scalar_names):
        """`scalars`, the record the window's loss launch writes, with a one-element view of every entry under its name
        (the first is `loss`), and the accumulation buffer"""
        self.scalars = torch.zeros(len(scalar_names), dtype=torch.float32, device=self.device)
        for i, name in enumerate(scalar_names):
            setattr(self, name, self.scalars[i:i + 1])
        self.accumulated = torch.zeros_like(self.params.grads)
        self._stage = {}

    def _finish_window(self, acts):
        """the tail of window_gradients behind the heads' backward pass: the torso backward, then the gradients clipped
        by their global norm or the norm alone (self.norm either way) -> the window's loss"""
        self.torso.backward(self.ctx, acts)
        if not self.clip_by_global_norm():
            self.grad_norm()
        return self.loss

    def stage_rows(self, obs, last_next_obs):
        """a window's n states and a state that does not follow them in memory (the observation before the reset behind
        a finished episode) -> one [n + 1, D] buffer"""
        T = obs.shape[0]
        buf = self._stage.get(T)
        if buf is None:
            buf = self._stage[T] = torch.empty(T + 1, obs.shape[1], dtype=obs.dtype, device=self.device)
        buf[:T].copy_(obs)
        buf[T].copy_(last_next_obs.view(-1))
        return buf

    def accumulate_window(self, *args, **kw):
        """accumulate_gradients (architecture.py:312-385): window_gradients, then accumulated += gradients"""
        loss = self.window_gradients(*args, **kw)
        self.lib.axpby(self.accumulated, 1.0, self.accumulated, 1.0, self.params.grads, self.params.size, self.ctx.stream)
        return loss

    def apply_accumulated(self, grad_scale=1.0):
        """apply_and_reset_gradients (architecture.py:469-521): one Adam step on the accumulated gradients, which are
        then cleared"""
        self.adam.step(float(grad_scale), grads=self.accumulated)
        self.accumulated.zero_()


class PolicyGradientNet(_WindowAccumulatingNet):
    """PolicyGradientNetworkParameters (agents/policy_gradients_agent.py:35-41): one embedder + FC middleware tower under
    a discrete PolicyHead (heads/policy_head.py:89-100): Dense(feat, A) named 'fc', default initialisation, whose outputs
    are the policy values (logits).  No target copy.  The head's loss and its gradient come from rlx_pg_head_loss
    (csrc/policy_gradient.hip); an update window's gradient is ADDED onto `accumulated`, which one Adam step consumes
    and clears (Architecture.accumulate_gradients / apply_and_reset_gradients)."""

    def __init__(self, device, obs_shape, n_actions, activation="relu", embedder="Medium", middleware="Medium",
                 learning_rate=2.5e-4, adam_beta1=0.9, adam_beta2=0.99, optimizer_epsilon=1e-4, clip_gradients=None,
                 beta_entropy=0.0, seed=0):
        self.A = discrete_policy_actions(n_actions)
        self.clip_gradients = clip_gradients
        self.beta_entropy = float(beta_entropy)
        feat = self._build_trunk(obs_shape, activation, embedder, middleware)
        self.head = G.Dense(self.params, "main/policy_values_head/fc", feat, self.A, None, 1)
        self.modules = [self.torso, self.head]
        self._finish(device, seed, learning_rate, adam_beta1, adam_beta2, optimizer_epsilon, has_target=False)
        self._finish_accumulating(("loss", "entropy"))               # (the mean entropy) of the last window

    def policy_values(self, obs, B, tag="act"):
        """the head's Dense output [B, A] (a Tensor; .data is the buffer): logits of the action probabilities"""
        return self.head.forward(self.ctx, self.trunk_forward(obs, B, tag)[-1], tag=tag)

    def window_gradients(self, obs, T, actions, advantages):
        """forward on the T states of one update window, the head loss against (actions, advantages), backward: the
        gradients in params.grads (clipped when clip_gradients is set), the loss and the mean entropy in self.scalars,
        tf.global_norm of the raw gradients in self.norm.  The context's buffers are keyed by shape, so every window
        length has its own activations and the means divide by the window's true length."""
        ctx = self.ctx
        acts = self.trunk_forward(obs, T, "train")
        z = self.head.forward(ctx, acts[-1], tag="train")
        self.lib.pg_head_loss(z.data, self.A, actions, advantages, self.beta_entropy, T, T, self.A, z.ensure_grad(),
                              self.A, self.scalars, self.status, ctx.stream)
        self.head.backward(ctx, acts[-1], z)
        return self._finish_window(acts)

    def learn_from_batch(self, obs, B, actions, advantages, grad_scale=1.0):
        """one NON-accumulating update on a batch of B rows: window_gradients, then one Adam step on params.grads
        (Architecture.train_on_batch; BCAgent.learn_from_batch with advantages of ones).  `accumulated` is not touched."""
        loss = self.window_gradients(obs, B, actions, advantages)
        self.adam.step(float(grad_scale))
        return loss


def actor_critic_net_kwargs(np_, alg, seed):
    """ActorCriticNetworkParameters + the algorithm's beta_entropy -> the keywords of ActorCriticNet's constructor"""
    heads = {h.head_type: h for h in np_.heads_parameters}
    return dict(policy_gradient_net_kwargs(np_, alg, seed), v_loss_weight=heads["VHead"].loss_weight)


class ActorCriticNet(_WindowAccumulatingNet):
    """ActorCriticNetworkParameters (agents/actor_critic_agent.py:69-77): one embedder + FC middleware tower under two
    heads — head 0 = VHead (heads/v_head.py:43-48: Dense(feat, 1), normalized-columns init std 1.0, MSE under
    loss_weight 0.5), head 1 = the discrete PolicyHead (Dense(feat, A) named 'fc', default initialisation).  No target
    copy; gradients clipped by global norm at 40.  Everything between the forward and the backward pass of an update
    window — the bootstrapped targets, the advantages, both heads' losses and gradients — is ONE launch,
    rlx_a3c_window_loss (csrc/a3c.hip)."""

    def __init__(self, device, obs_shape, n_actions, activation="relu", embedder="Medium", middleware="Medium",
                 learning_rate=2.5e-4, adam_beta1=0.9, adam_beta2=0.99, optimizer_epsilon=1e-4, clip_gradients=40.0,
                 beta_entropy=0.0, v_loss_weight=0.5, seed=0):
        self.A = discrete_policy_actions(n_actions)
        self.clip_gradients = clip_gradients
        self.beta_entropy, self.v_loss_weight = float(beta_entropy), float(v_loss_weight)
        feat = self._build_trunk(obs_shape, activation, embedder, middleware)
        self.v_head = G.Dense(self.params, "main/v_values_head/output", feat, 1, None, 1, init=G.normalized_columns(1.0))
        self.pi_head = G.Dense(self.params, "main/policy_values_head/fc", feat, self.A, None, 1)
        self.heads = [self.v_head, self.pi_head]
        self.modules = [self.torso] + self.heads
        self._finish(device, seed, learning_rate, adam_beta1, adam_beta2, optimizer_epsilon, has_target=False)
        # total loss, value loss, policy loss, mean entropy of the last window
        self._finish_accumulating(("loss", "value_loss", "policy_loss", "entropy"))

    def policy_values(self, obs, B, tag="act"):
        """the policy head's Dense output [B, A] (logits of the action probabilities); the V head is not run"""
        return self.pi_head.forward(self.ctx, self.trunk_forward(obs, B, tag)[-1], tag=tag)

    def predict(self, obs, B, tag="predict"):
        """both heads -> (V [B], logits [B, A]) as buffers"""
        feat = self.trunk_forward(obs, B, tag)[-1]
        v, z = self._heads_forward([(l, feat) for l in self.heads], tag)
        return v.data.view(B), z.data.view(B, self.A)

    def window_gradients(self, obs_rows, T, bootstrap, actions, targets, advantages, rewards=None, game_over=None,
                         discount=0.0, gae_lambda=0.0, rescaler=_rlx.A3C_TARGETS_GIVEN, estimate_with_gae=False):
        """forward on the T states of one update window and, with bootstrap, on the last next state behind them (obs_rows
        has T + bootstrap rows); rlx_a3c_window_loss against (actions, rewards, the device's game-over flag), which
        leaves the fp64 value targets and advantages in targets / advantages [T] — or, with the default rescaler, reads
        them from there; both heads backward, their input gradients summed; the torso backward: the gradients in
        params.grads (clipped when clip_gradients is set), the four scalars in self.scalars, tf.global_norm of the raw
        gradients in self.norm.  The context's buffers are keyed by shape; the means divide by T."""
        ctx, A = self.ctx, self.A
        rows = T + int(bool(bootstrap))
        acts = self.trunk_forward(obs_rows, rows, "train")
        fork = self._fork(acts[-1], self.heads, "train")
        v, z = outs = self._heads_forward(fork, "train")
        self.values = v.data.view(rows)                  # the 'Values' samples are its first T entries
        self.lib.a3c_window_loss(v.data, 1, z.data, A, actions, rewards, game_over, T, rows, A, float(discount),
                                 float(gae_lambda), int(rescaler), int(bool(estimate_with_gae)), self.beta_entropy,
                                 self.v_loss_weight, targets, advantages, v.ensure_grad(), 1, z.ensure_grad(), A,
                                 self.scalars, self.status, ctx.stream)
        self._heads_backward(acts[-1], fork, outs)
        return self._finish_window(acts)


def n_step_q_net_kwargs(np_, seed):
    """NStepQNetworkParameters -> the keywords of NStepQNet's constructor"""
    return dict(common_net_kwargs(np_, seed), clip_gradients=getattr(np_, "clip_gradients", None),
                replace_mse_with_huber_loss=np_.replace_mse_with_huber_loss)


class NStepQNet(_WindowAccumulatingNet):
    """NStepQNetworkParameters (agents/n_step_q_agent.py:34-43): one embedder + FC middleware tower under the plain QHead
    (Dense(feat, A), the layer and initialisation of DQNNet._q_head_layer), with a target copy; MSE unless
    replace_mse_with_huber_loss.  Everything between the forward and the backward pass of an update window — the
    bootstrapped N-step or 1-step targets from the target network, the Q head's loss on the taken action and its
    gradient — is ONE launch, rlx_nstep_q_window_loss (csrc/n_step_q.hip)."""

    def __init__(self, device, obs_shape, n_actions, activation="relu", embedder="Medium", middleware="Medium",
                 learning_rate=2.5e-4, adam_beta1=0.9, adam_beta2=0.99, optimizer_epsilon=1e-4, clip_gradients=None,
                 replace_mse_with_huber_loss=False, seed=0):
        self.A = int(n_actions)
        self.clip_gradients = clip_gradients
        self.huber = bool(replace_mse_with_huber_loss)
        feat = self._build_trunk(obs_shape, activation, embedder, middleware)
        self.q_head = G.Dense(self.params, "main/q_head/dense", feat, self.A, None, 1)
        self.modules = [self.torso, self.q_head]
        self._finish(device, seed, learning_rate, adam_beta1, adam_beta2, optimizer_epsilon, has_target=True)
        self._finish_accumulating(("loss",))                         # of the last window
        self.td_targets = None           # [T, A] of the last window: state_value_head_targets, the 'Q Values' samples

    def _q(self, obs, B, tag, weights=None):
        acts = self.trunk_forward(obs, B, tag, weights)
        return acts, self.q_head.forward(self.ctx, acts[-1], tag=tag, weights=weights)

    def q_values(self, obs, B, tag="act"):
        """the ONLINE network's Q values [B, A] (a Tensor; .data is the buffer), for acting"""
        return self._q(obs, B, tag)[1]

    def target_q_values(self, obs, rows, tag="target"):
        """the TARGET network's Q values [rows, A]"""
        return self._q(obs, rows, tag, self.target)[1]

    def window_gradients(self, obs, T, actions, targets, target_obs=None, rows_t=0, rewards=None, game_over=None,
                         discount=0.0, horizon=_rlx.NSTEPQ_TARGETS_GIVEN, target_matrix=None):
        """the online network forward on the T states of one update window and the target network on rows_t states
        behind them (one for 'N-Step', the T next states for '1-Step'); rlx_nstep_q_window_loss against (actions,
        rewards, the device's game-over flag), which leaves the fp32 targets in targets [T] — or, with the default
        horizon, reads them from there — and the whole target matrix in self.td_targets; the head and the torso
        backward: the gradients in params.grads (clipped when clip_gradients is set), the loss in self.loss,
        tf.global_norm of the raw gradients in self.norm.  target_matrix [T, A] (what Architecture.accumulate_gradients
        is handed): the head's loss against every column, which is rlx_regression_loss."""
        ctx, A = self.ctx, self.A
        q_t = self.target_q_values(target_obs, rows_t, tag="train_target").data if rows_t else None
        acts, q = self._q(obs, T, "train")
        # what the launch reads, kept for the tests: the two networks' outputs of the last window
        self.q_online, self.q_target = q.data.view(T, A), (q_t.view(rows_t, A) if rows_t else None)
        if target_matrix is not None:
            self.td_targets = target_matrix
            self.lib.regression_loss(q.data, A, target_matrix, A, None, T, A, int(self.huber), 1.0, 1.0,
                                     q.ensure_grad(), A, self.scalars, ctx.stream)
        else:
            self.td_targets = ctx.buffer(self.q_head.name + "/td_targets", (T, A), tag="train")
            self.lib.nstep_q_window_loss(q.data, A, q_t, A, rows_t, actions, rewards, game_over, T, A, float(discount),
                                         int(horizon), int(self.huber), targets, self.td_targets, A, q.ensure_grad(), A,
                                         self.scalars, self.status, ctx.stream)
        self.q_head.backward(ctx, acts[-1], q)
        return self._finish_window(acts)


def acer_net_kwargs(np_, alg, seed):
    """ACERNetworkParameters + the algorithm's head constants -> the keywords of ACERNet's constructor"""
    heads = {h.head_type: h for h in np_.heads_parameters}
    return dict(policy_gradient_net_kwargs(np_, alg, seed), q_loss_weight=heads["QHead"].loss_weight,
                importance_weight_truncation=alg.importance_weight_truncation, max_kl_divergence=alg.max_KL_divergence,
                trust_region=bool(getattr(alg, "apply_trust_region_to_gradients", False)))


class ACERNet(_WindowAccumulatingNet):
    """ACERNetworkParameters (agents/acer_agent.py:78-87): one embedder + FC middleware tower under two heads — head 0 =
    the plain QHead (Dense(feat, A), the layer and initialisation of NStepQNet's; MSE under loss_weight 0.5), head 1 =
    ACERPolicyHead (Dense(feat, A) named 'fc', default initialisation) — with a target copy, which is the AVERAGE policy
    network; gradients clipped by global norm at 40.  Everything between the forward and the backward pass of an update
    window — state values, importance weights, the Q-retrace targets, both heads' losses and gradients — is ONE launch,
    rlx_acer_window_loss (csrc/acer.hip).  A window's gradients REPLACE the accumulation buffer and are applied at
    once (NetworkWrapper.train_and_sync_networks, network_wrapper.py:156-177: accumulate_gradients(no_accumulation=True),
    then apply_gradients without a reset); the buffer keeps them, so the base's apply step applies the last window's
    gradients once more and then clears them (:179-203).  `adam_steps` counts the Adam steps."""

    def __init__(self, device, obs_shape, n_actions, activation="relu", embedder="Medium", middleware="Medium",
                 learning_rate=2.5e-4, adam_beta1=0.9, adam_beta2=0.99, optimizer_epsilon=1e-4, clip_gradients=40.0,
                 beta_entropy=0.0, q_loss_weight=0.5, importance_weight_truncation=10.0, max_kl_divergence=1.0,
                 trust_region=False, seed=0):
        self.A = discrete_policy_actions(n_actions)
        self.clip_gradients = clip_gradients
        self.beta_entropy, self.q_loss_weight = float(beta_entropy), float(q_loss_weight)
        self.truncation, self.max_kl = float(importance_weight_truncation), float(max_kl_divergence)
        self.trust_region = bool(trust_region)
        feat = self._build_trunk(obs_shape, activation, embedder, middleware)
        self.q_head = G.Dense(self.params, "main/q_head/dense", feat, self.A, None, 1)
        self.pi_head = G.Dense(self.params, "main/acer_policy_head/fc", feat, self.A, None, 1)
        self.heads = [self.q_head, self.pi_head]
        self.modules = [self.torso] + self.heads
        self._finish(device, seed, learning_rate, adam_beta1, adam_beta2, optimizer_epsilon, has_target=True)
        self._finish_accumulating(("loss", "q_loss", "policy_loss", "probability_loss", "bias_correction_loss",
                                   "kl_divergence", "entropy"))
        self.bootstrap_value = torch.zeros(1, dtype=torch.float32, device=device)
        self.adam_steps = 0
        self._window = {}

    def policy_values(self, obs, B, tag="act"):
        """the policy head's Dense output [B, A] (logits of the action probabilities); the Q head is not run"""
        return self.pi_head.forward(self.ctx, self.trunk_forward(obs, B, tag)[-1], tag=tag)

    def predict(self, obs, B, tag="predict", use_target=False):
        """both heads of the online network, or of the average (target) one -> (Q [B, A], logits [B, A]) as buffers"""
        w = self.target if use_target else None
        feat = self.trunk_forward(obs, B, tag, w)[-1]
        q, z = self._heads_forward([(l, feat) for l in self.heads], tag, w)
        return q.data.view(B, self.A), z.data.view(B, self.A)

    def average_policy_values(self, obs, B, tag="avg"):
        """the AVERAGE (target) network's policy logits [B, A]"""
        feat = self.trunk_forward(obs, B, tag, self.target)[-1]
        return self.pi_head.forward(self.ctx, feat, tag=tag, weights=self.target).data.view(B, self.A)

    def window_buffers(self, T):
        """the window's arrays the launch writes (or, given, reads): V, rho, rho_i, avg_policy, q_retrace, td_targets"""
        w = self._window.get(T)
        if w is None:
            z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)
            w = self._window[T] = dict(V=z(T), rho=z(T, self.A), rho_i=z(T), avg_policy=z(T, self.A), q_retrace=z(T),
                                       td_targets=z(T, self.A))
        return w

    def window_gradients(self, obs_rows, T, bootstrap, actions, mu=None, rewards=None, game_over=None, discount=0.0,
                         given=None):
        """the online network forward on the T states of one update window and, with bootstrap, on the state behind them
        (obs_rows has T + bootstrap rows), the average network's policy head on the T states; rlx_acer_window_loss
        against (mu, actions, rewards, the device's game-over flag), which leaves the window's arrays in
        self.window — or, with `given` (a dict of them: what Architecture.accumulate_gradients is handed), reads them;
        both heads backward, their input gradients summed; the torso backward: the gradients in params.grads (clipped
        when clip_gradients is set), the seven scalars in self.scalars, tf.global_norm of the raw gradients in
        self.norm.  The context's buffers are keyed by shape; the means divide by T."""
        ctx, A = self.ctx, self.A
        rows = T + int(bool(bootstrap))
        mode = _rlx.ACER_TRUST_REGION if self.trust_region else 0
        if given is None:
            w = self.window_buffers(T)
            avg_z = self.average_policy_values(obs_rows, T, tag="train_avg")
        else:
            w, avg_z, mode = given, None, mode | _rlx.ACER_TARGETS_GIVEN
        self.window = w
        acts = self.trunk_forward(obs_rows, rows, "train")
        fork = self._fork(acts[-1], self.heads, "train")
        q, z = outs = self._heads_forward(fork, "train")
        self.q_online, self.logits = q.data.view(rows, A), z.data.view(rows, A)    # what the launch reads (for the tests)
        self.lib.acer_window_loss(q.data, A, z.data, A, rows, avg_z, A, mu, A, actions, rewards, game_over, T, A,
                                  float(discount), self.truncation, self.max_kl, self.beta_entropy, self.q_loss_weight,
                                  mode, w["V"], w["rho"], A, w["rho_i"], w["avg_policy"], A, w["q_retrace"],
                                  self.bootstrap_value, w["td_targets"], A, q.ensure_grad(), A, z.ensure_grad(), A,
                                  self.scalars, self.status, ctx.stream)
        self._heads_backward(acts[-1], fork, outs)
        return self._finish_window(acts)

    def train_window(self, *args, rate=None, **kw):
        """train_and_sync_networks (network_wrapper.py:156-177): the window's gradients replace the accumulation buffer
        and are applied at once, the buffer is NOT cleared; then the average network moves by `rate`
        (acer_agent.py:167-168)"""
        loss = self.window_gradients(*args, **kw)
        self.accumulated.copy_(self.params.grads)
        self.adam.step(1.0, grads=self.accumulated)
        self.adam_steps += 1
        if rate is not None:
            self.update_target(rate)
        return loss

    def apply_accumulated(self, grad_scale=1.0):
        super().apply_accumulated(grad_scale)
        self.adam_steps += 1


class PPOCriticNet(_NetBase):
    """PPOCriticNetworkParameters (agents/ppo_agent.py:40-49): one embedder + FC middleware tower (tanh) under the plain
    VHead (heads/v_head.py:43-52: Dense(feat, 1), normalized-columns(1.0) initialisation, MSE through
    rlx_regression_loss), with a target copy."""

    def __init__(self, device, obs_shape, activation="tanh", embedder="Medium", middleware="Medium", learning_rate=2.5e-4,
                 adam_beta1=0.9, adam_beta2=0.99, optimizer_epsilon=1e-4, seed=0):
        feat = self._build_trunk(obs_shape, activation, embedder, middleware)
        self.v_head = G.Dense(self.params, "main/v_head/dense", feat, 1, None, 1, init=G.normalized_columns(1.0))
        self.modules = [self.torso, self.v_head]
        self._finish(device, seed, learning_rate, adam_beta1, adam_beta2, optimizer_epsilon)
        self.scalars = torch.zeros(1, dtype=torch.float32, device=device)
        self.loss = self.scalars[0:1]

    def values(self, obs, B, use_target=False, tag="val"):
        """V(s) [B] (fill_advantages, ppo_agent.py:163)"""
        w = self.target if use_target else None
        acts = self.trunk_forward(obs, B, tag, w)
        return self.v_head.forward(self.ctx, acts[-1], tag=tag, weights=w).data.view(-1)

    def forward_backward(self, obs, B, value_targets):
        """accumulate_gradients of one critic minibatch (:233): forward, MSE against the fp32 targets [B], backward;
        the loss in self.loss"""
        ctx = self.ctx
        acts = self.trunk_forward(obs, B, "train")
        v = self.v_head.forward(ctx, acts[-1], tag="train")
        self.lib.regression_loss(v.data, 1, value_targets, 1, None, B, 1, 0, 1.0, 1.0, v.ensure_grad(), 1, self.loss,
                                 ctx.stream)
        self.v_head.backward(ctx, acts[-1], v)
        self.torso.backward(ctx, acts)

    def train_minibatch(self, obs, B, value_targets, grad_scale=1.0):
        self.forward_backward(obs, B, value_targets)
        self.apply_gradients(grad_scale, with_norm=True)
        return self.loss


class PPOActorNet(_NetBase):
    """PPOActorNetworkParameters (agents/ppo_agent.py:52-62): one embedder + FC middleware tower (tanh) under the PPOHead
    built WITHOUT a clip range and with the KL penalty (heads/ppo_head.py:40-47, :66-72) — discrete: Dense(feat, A)
    'policy_fc'; continuous: 'policy_mean' with the normalized-columns(0.01) initialiser plus the state-independent
    'policy_log_std' vector — with a target copy (the old policy).  The head's loss and gradient are ONE launch
    (rlx_ppo_kl_discrete_loss / rlx_ppo_kl_continuous_loss, csrc/ppo_kl.hip); kl_coefficient lives on the device, an
    epoch's fetch sums in `epoch_sums`, and update_kl_coefficient() is ppo_agent.py:329-353 without a host read."""

    def __init__(self, device, obs_shape, n_actions, activation="tanh", embedder="Medium", middleware="Medium",
                 learning_rate=2.5e-4, adam_beta1=0.9, adam_beta2=0.99, optimizer_epsilon=1e-4, beta_entropy=0.01,
                 target_kl_divergence=0.01, initial_kl_coefficient=1.0, high_kl_penalty_coefficient=1000.0,
                 use_kl_regularization=True, seed=0, continuous=False):
        self.A = int(n_actions)
        self.continuous = bool(continuous)
        limit = 32 if self.continuous else 18
        if not 1 <= self.A <= limit:
            raise ValueError("the PPO head serves 1 .. %d %s (got %d)"
                             % (limit, "action dimensions" if self.continuous else "actions", self.A))
        self.beta, self.use_kl = float(beta_entropy), bool(use_kl_regularization)
        self.target_kl, self.high_kl = float(target_kl_divergence), float(high_kl_penalty_coefficient)
        feat = self._build_trunk(obs_shape, activation, embedder, middleware)
        if self.continuous:
            self.pi_head = G.Dense(self.params, "main/ppo_head/policy_mean", feat, self.A, None, 1,
                                   init=G.normalized_columns(0.01))
            self.params.add_group([("main/ppo_head/policy_log_std", (self.A,))])        # zeros (ppo_head.py:133-137)
        else:
            self.pi_head = G.Dense(self.params, "main/ppo_head/policy_fc", feat, self.A, None, 1)
        self.modules = [self.torso, self.pi_head]
        self._finish(device, seed, learning_rate, adam_beta1, adam_beta2, optimizer_epsilon)
        # [surrogate, mean entropy, mean KL, total, penalty factor c]
        self.scalars = torch.zeros(5, dtype=torch.float32, device=device)
        self.kl_coefficient = torch.full((1,), float(initial_kl_coefficient), dtype=torch.float32, device=device)
        self.epoch_sums = torch.zeros(4, dtype=torch.float32, device=device)   # += {KL, entropy, total, 1} per minibatch
        self.kl_mean = torch.zeros(1, dtype=torch.float32, device=device)

    def policy_probs(self, obs, B, use_target=False, tag="act", out=None):
        """softmax(policy_fc(tower(obs))) [B, A]; the target weights are the old policy"""
        w = self.target if use_target else None
        acts = self.trunk_forward(obs, B, tag, w)
        logits = self.pi_head.forward(self.ctx, acts[-1], tag=tag, weights=w)
        probs = out if out is not None else self.ctx.buffer("probs", (B, self.A), tag=tag)
        self.lib.softmax(logits.data, self.A, B, self.A, probs, self.A, self.ctx.stream)
        return probs

    def policy_mean_std(self, obs, B, use_target=False, tag="act", out_mean=None, out_std=None):
        """[policy_mean, policy_std] [B, A] each (ppo_head.py:138-144): std = exp(log_std) tiled over the batch"""
        w = self.target if use_target else None
        acts = self.trunk_forward(obs, B, tag, w)
        mean = self.pi_head.forward(self.ctx, acts[-1], tag=tag, weights=w).data.view(B, self.A)
        std = out_std if out_std is not None else self.ctx.buffer("policy_std", (B, self.A), tag=tag)
        self.lib.exp_rows(self.params.w("main/ppo_head/policy_log_std", 0, w), std, B, self.A, self.ctx.stream)
        if out_mean is not None:
            out_mean.copy_(mean)
            mean = out_mean
        return mean, std

    def forward_backward(self, obs, B, actions, advantages, old_policy, ratio_out=None, accumulate=True):
        """accumulate_gradients of one actor minibatch (ppo_agent.py:278-288): forward, the head launch, backward.
        old_policy: the old probabilities [B, A], or (old_mean, old_std).  accumulate: add the minibatch's fetches onto
        epoch_sums."""
        ctx = self.ctx
        acts = self.trunk_forward(obs, B, "train")
        z = self.pi_head.forward(ctx, acts[-1], tag="train")
        acc = self.epoch_sums if accumulate else None
        if self.continuous:
            old_mean, old_std = old_policy
            self.lib.ppo_kl_continuous_loss(z.data, self.A, self.params.w("main/ppo_head/policy_log_std"), actions,
                                            advantages, old_mean, old_std, self.A, B, self.A, self.beta, 1.0,
                                            self.kl_coefficient, 2.0 * self.target_kl, self.high_kl, int(self.use_kl),
                                            z.ensure_grad(), self.A, self.params.g("main/ppo_head/policy_log_std"),
                                            self.scalars, ratio_out, acc, ctx.stream)
        else:
            self.lib.ppo_kl_discrete_loss(z.data, self.A, actions, advantages, old_policy, self.A, B, self.A, self.beta,
                                          1.0, self.kl_coefficient, 2.0 * self.target_kl, self.high_kl, int(self.use_kl),
                                          z.ensure_grad(), self.A, self.scalars, ratio_out, self.status, acc, ctx.stream)
        self.pi_head.backward(ctx, acts[-1], z)
        self.torso.backward(ctx, acts)

    def train_minibatch(self, obs, B, actions, advantages, old_policy, grad_scale=1.0, ratio_out=None):
        self.forward_backward(obs, B, actions, advantages, old_policy, ratio_out)
        self.apply_gradients(grad_scale, with_norm=True)
        return self.scalars

    def reset_epoch_sums(self):
        self.epoch_sums.zero_()

    def update_kl_coefficient(self):
        """update_kl_coefficient (ppo_agent.py:329-353) from epoch_sums (the LAST epoch's: call reset_epoch_sums() before
        every epoch — forward_backward adds onto them by default); the mean KL goes to kl_mean.  With nothing
        accumulated since the reset the coefficient is kept and kl_mean is 0.  Nothing is read on the host."""
        self.lib.ppo_kl_coefficient_update(self.epoch_sums, self.target_kl, self.kl_coefficient, self.kl_mean,
                                           self.ctx.stream)


def dfp_net_kwargs(np_, seed):
    """DFPNetworkParameters -> the keywords of DFPNet's constructor (behind the shapes)."""
    head = np_.heads_parameters[0]
    return dict(embedders={k: (np_.embedder_schemes[k], np_.embedder_activations[k]) for k in DFPNet.INPUTS},
                head_activation=head.activation_function, learning_rate=np_.learning_rate,
                adam_beta1=np_.adam_optimizer_beta1, adam_beta2=np_.adam_optimizer_beta2,
                optimizer_epsilon=np_.optimizer_epsilon, clip_gradients=getattr(np_, "clip_gradients", None), seed=seed)


class DFPNet(_NetBase):
    """DFPNetworkParameters (agents/dfp_agent.py:42-73): three vector input embedders — goal, measurements, observation,
    each with its own scheme and activation — whose outputs are concatenated in sorted name order
    (general_network.py:252,277), no middleware (MiddlewareScheme.Empty), and the MeasurementsPredictionHead
    (heads/measurements_prediction_head.py:39-62): an expectation stream Dense(256, act) -> Dense(K) and an action stream
    Dense(256, act) -> Dense(A * K), K = num_predicted_steps_ahead * num_measurements, merged as csrc/dfp_merge.hpp
    states.  No target network.  The merge, the loss and the gradients of the two stream outputs are ONE launch
    (rlx_dfp_head_loss), acting is the forward pass + rlx_dfp_egreedy / rlx_dfp_argmax; every layer is a generic G.Dense
    launch (leaky_relu by default, which no fused launch serves).

    The goal is an input like the others: [B, M] rows (the agent repeats its current goal), so its embedder's weight
    gradients are sums over the rows like any layer's."""
    INPUTS = ("goal", "measurements", "observation")            # sorted: the order of the concatenation

    def __init__(self, device, obs_dim, n_measurements, n_actions, n_steps, embedders=None, head_activation="leaky_relu",
                 learning_rate=2.5e-4, adam_beta1=0.95, adam_beta2=0.99, optimizer_epsilon=1e-4, clip_gradients=None,
                 seed=0):
        self.obs_dim, self.M, self.A, self.S = int(obs_dim), int(n_measurements), int(n_actions), int(n_steps)
        self.K = self.S * self.M
        self.image = False
        self.clip_gradients = clip_gradients
        self.dims = {"goal": self.M, "measurements": self.M, "observation": self.obs_dim}
        default = {"goal": ([128, 128, 128], "leaky_relu"), "measurements": ([128, 128, 128], "leaky_relu"),
                   "observation": ("Medium", "leaky_relu")}
        embedders = dict(default, **(embedders or {}))
        if sorted(embedders) != list(self.INPUTS):
            raise ValueError("DFPNet takes the input embedders {}, got {}".format(list(self.INPUTS), sorted(embedders)))
        self.params = G.FlatParams()
        self.embedders, self.offsets, feat = {}, {}, 0
        for name in self.INPUTS:
            scheme, act = embedders[name]
            units = VECTOR_EMBEDDER[scheme] if isinstance(scheme, str) else list(scheme)
            layers, d = [], self.dims[name]
            for i, u in enumerate(units):
                layers.append(G.Dense(self.params, "main/%s/embedder/dense%d" % (name, i), d, int(u), act, 1))
                d = int(u)
            self.embedders[name] = G.Sequential(layers)
            self.offsets[name] = (feat, d)
            feat += d
        self.feat = feat
        hn = "main/future_measurements_head"
        self.e_fc = G.Dense(self.params, hn + "/expectation_stream/fc1", feat, 256, head_activation, 1)
        self.e_out = G.Dense(self.params, hn + "/expectation_stream/output", 256, self.K, None, 1)
        self.a_fc = G.Dense(self.params, hn + "/action_stream/fc1", feat, 256, head_activation, 1)
        self.a_out = G.Dense(self.params, hn + "/action_stream/output", 256, self.A * self.K, None, 1)
        self.modules = [self.embedders[n] for n in self.INPUTS] + [self.e_fc, self.e_out, self.a_fc, self.a_out]
        self._finish(device, seed, learning_rate, adam_beta1, adam_beta2, optimizer_epsilon, has_target=False)
        self.loss = torch.zeros(1, dtype=torch.float32, device=device)
        self.loss_ws = torch.zeros(256, dtype=torch.float32, device=device)       # per-row loss partials
        self.ticket = torch.zeros(1, dtype=torch.int32, device=device)

    def forward(self, inputs, B, tag="act", weights=None):
        """inputs: {'goal' [B, M], 'measurements' [B, M], 'observation' [B, D]} fp32 device tensors
        -> (E Tensor [1, B, K], X Tensor [1, B, A*K], saved)."""
        ctx = self.ctx
        merged = ctx.buffer("main/merged", (1, B, self.feat), tag=tag)
        acts = {}
        for name in self.INPUTS:
            x = G.input_tensor(inputs[name], B, self.dims[name])
            a = self.embedders[name].forward(ctx, x, tag=tag, weights=weights)
            off, d = self.offsets[name]
            self.lib.copy_2d(a[-1].data, d, merged.data_ptr() + 4 * off, self.feat, B, d, 1.0, ctx.stream)
            acts[name] = a
        m = G.Tensor(merged, B, self.feat, 1, grad_key=(ctx, "main/merged", tag))
        he = self.e_fc.forward(ctx, m, tag=tag, weights=weights)
        e = self.e_out.forward(ctx, he, tag=tag, weights=weights)
        ha = self.a_fc.forward(ctx, m, tag=tag, weights=weights)
        x = self.a_out.forward(ctx, ha, tag=tag, weights=weights)
        return e, x, (acts, m, he, ha)

    def can_act_fused(self, n_env):
        return False

    def streams(self, inputs, B, tag="act"):
        """the two stream outputs of a forward pass: E [B, K] and X [B, A*K] (what the acting launches read)."""
        e, x, _ = self.forward(inputs, B, tag=tag)
        return e.data.view(B, self.K), x.data.view(B, self.A * self.K)

    def backward(self, e, x, saved, B):
        """e.grad / x.grad hold the gradients of the two stream outputs -> params.grads."""
        ctx = self.ctx
        acts, m, he, ha = saved
        self.e_out.backward(ctx, he, e)
        self.a_out.backward(ctx, ha, x)
        # the two streams' input gradients add up in the concatenation's gradient
        side = G.Tensor(m.data, m.rows, m.cols, 1)
        side.grad = ctx.buffer("main/merged/side:grad", tuple(m.data.shape), tag="train")
        self.e_fc.backward(ctx, m, he)
        self.a_fc.backward(ctx, side, ha)
        g = m.grad
        self.lib.axpby(g, 1.0, g, 1.0, side.grad, g.numel(), ctx.stream)
        for name in self.INPUTS:
            seq, a = self.embedders[name], acts[name]
            if not seq.layers:
                continue
            off, d = self.offsets[name]
            out = a[-1]
            self.lib.copy_2d(g.data_ptr() + 4 * off, self.feat, out.ensure_grad(), d, B, d, 1.0, ctx.stream)
            out.grad_is_dz = False
            seq.backward(ctx, a)

    def accumulate(self, inputs, B, actions, future_measurements, y_out=None, targets_out=None):
        """forward, rlx_dfp_head_loss, backward: the gradients in params.grads, the loss in self.loss.
        future_measurements: fp32 [B, K], may hold NaN."""
        e, x, saved = self.forward(inputs, B, tag="train")
        K, AK = self.K, self.A * self.K
        self.lib.dfp_head_loss(e.data, K, x.data, AK, actions, future_measurements, self.A, K, B, 1.0, e.ensure_grad(), K,
                               x.ensure_grad(), AK, self.loss_ws, self.ticket, self.loss, self.status, y_out, targets_out,
                               self.ctx.stream)
        self.backward(e, x, saved, B)

    def learn_from_batch(self, inputs, B, actions, future_measurements, grad_scale=1.0, sync=None):
        """DFPAgent.learn_from_batch (agents/dfp_agent.py:150-167), all on device: ONE forward pass, the loss launch,
        backward, clip, Adam."""
        self.accumulate(inputs, B, actions, future_measurements)
        clipped = self.clip_by_global_norm()
        if sync is not None:
            sync.all_reduce_sum(self.params.grads)
        self.apply_gradients(grad_scale, with_norm=not clipped)
        return self.loss
