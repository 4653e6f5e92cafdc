"""numpy restatement of the imitation-learning launches, the twin of csrc/imitation.hip, pinned to the reference's own
code by tests/test_imitation_ref.py (recorded in tests/golden/imitation.npz).

  softmax_parts(logits)  -> (p, mx, s): the project's one softmax (c51_ref.softmax: csrc/policy_head.hpp, softmax_row), fp32:
      mx = max z;  e_j = fp32(exp(fp64(fp32(z_j - mx))));  s = e_0 + e_1 + .. in index order, every addition rounded to
      fp32;  p_j = fp32(e_j / s).
  classification_head_loss(logits, actions= | labels=, grad_scale) -> dict: ClassificationHead
      (heads/classification_head.py: tf.nn.softmax, softmax_cross_entropy_with_logits) summed as general_network.py:360
      sums it.  fp32 rounding points: t_j = fp32(z_j - mx);  logs = fp32(log(fp64(s)));  logp_j = fp32(t_j - logs);
      actions: loss_b = -logp_a;  labels: acc = 0, acc = fp32(acc + fp32(l_j * logp_j)) in index order, loss_b = -acc;
      dz_j = fp32(fp32(p_j - l_j) * grad_scale).  loss_sum = tree_sum(loss) — NOT np.sum; no 1/B anywhere.
  tree_sum(v)  the launch's batch sum: v padded with 0.f to T = max(64, len rounded up to a power of two); for d = T/2,
      T/4 .. 1: v[:d] = fp32(v[:d] + v[d:2d]); the result is v[0].
  imitation_selector(q, imitation, threshold, probs_in, seed, rank, event) -> (sel, familiarity, mask, zero_rows):
      DDQNBCQAgent.select_actions, NN branch (agents/ddqn_bcq_agent.py:115-133) up to its argmax: familiarity =
      softmax_parts(logits)[0] (or the probabilities handed in), mask = familiarity < fp32(threshold) compared in fp32
      (numpy compares a float32 array with a Python float in fp32; NaN is not masked), -inf there; a row whose maximum is
      then -inf takes bcq_ref.uniforms, exactly as bcq_ref.masked_selector.
  reward_model_schedule(epochs, imitation_epochs, batches_per_epoch) -> [(epoch, batch, kind)]: improve_reward_model's
      interleaving (:143-183): ONE generator per epoch; per batch the reward model while epoch < epochs, then the
      imitation model while epoch < imitation_epochs.
  one_hot(actions, A)  the target matrix of :168-169 (fp64 zeros with ones, as the reference builds it).
"""
import numpy as np

import bcq_ref
import c51_ref

F32 = np.float32
INPUT_PROBS = 1                                  # RLX_IMITATION_INPUT_PROBS


def _log32(v):
    return np.log(np.asarray(v, dtype=F32).astype(np.float64)).astype(F32)


def softmax_parts(logits):
    x = np.asarray(logits, dtype=F32)
    mx = x.max(axis=-1, keepdims=True)
    e = np.exp((x - mx).astype(np.float64)).astype(F32)
    s = np.zeros(x.shape[:-1], dtype=F32)
    for j in range(x.shape[-1]):
        s = s + e[..., j]
    p = e / s[..., None]
    assert p.dtype == F32 and np.array_equal(p.view(np.uint32), c51_ref.softmax(x).view(np.uint32))     # ONE definition
    return p, mx[..., 0], s


def tree_sum(v):
    v = np.asarray(v, dtype=F32).ravel()
    T = 64
    while T < v.size:
        T <<= 1
    w = np.zeros(T, dtype=F32)
    w[:v.size] = v
    d = T >> 1
    while d > 0:
        w[:d] = w[:d] + w[d:2 * d]
        d >>= 1
    return w[0]


def one_hot(actions, A):
    t = np.zeros((len(actions), A))
    t[range(len(actions)), np.asarray(actions)] = 1
    return t


def classification_head_loss(logits, actions=None, labels=None, grad_scale=1.0):
    assert (actions is None) != (labels is None), "exactly one of actions and labels"
    x = np.asarray(logits, dtype=F32)
    B, A = x.shape
    p, mx, s = softmax_parts(x)
    logp = (x - mx[:, None]) - _log32(s)[:, None]
    assert logp.dtype == F32
    gs = F32(grad_scale)
    rows = np.arange(B)
    if actions is not None:
        act = np.asarray(actions)
        valid = (act >= 0) & (act < A)
        a = np.where(valid, act, 0)
        l = np.zeros((B, A), dtype=F32)
        l[rows, a] = 1
        loss = np.where(valid, -logp[rows, a], F32(0)).astype(F32)
        dz = np.where(valid[:, None], (p - l) * gs, F32(0)).astype(F32)
        correct = int(((np.argmax(p, axis=1) == a) & valid).sum())
        status = int(not valid.all())
    else:
        l = np.asarray(labels, dtype=F32)
        acc = np.zeros(B, dtype=F32)
        for j in range(A):
            acc = acc + l[:, j] * logp[:, j]
        loss = -acc
        dz = (p - l) * gs
        correct = int((np.argmax(p, axis=1) == np.argmax(l, axis=1)).sum())
        status = 0
    assert loss.dtype == F32 and dz.dtype == F32
    return dict(probs=p, logp=logp, row_loss=loss, dlogits=dz, loss_sum=tree_sum(loss), correct=correct, status=status)


def cross_entropy_f64(logits, labels):
    """the same cross entropy evaluated in fp64 on the fp32 logits (the error yardstick of the restatement) -> per row"""
    x = np.asarray(logits, dtype=F32).astype(np.float64)
    t = x - x.max(axis=1, keepdims=True)
    logp = t - np.log(np.exp(t).sum(axis=1, keepdims=True))
    return -(np.asarray(labels, dtype=np.float64) * logp).sum(axis=1)


def imitation_selector(q_next_online, imitation, threshold, probs_in=False, seed=0, rank=0, event=0):
    sel = np.array(q_next_online, dtype=F32)
    fam = np.array(imitation, dtype=F32) if probs_in else softmax_parts(imitation)[0]
    with np.errstate(invalid="ignore"):
        mask = fam < F32(threshold)
    sel[mask] = -np.inf
    zero_rows = sel.max(axis=1) == -np.inf
    if zero_rows.any():
        sel[zero_rows] = bcq_ref.uniforms(sel.shape[0], sel.shape[1], seed, rank, event)[zero_rows]
    return sel, fam, mask, zero_rows


def reward_model_schedule(epochs, imitation_epochs, batches_per_epoch):
    out = []
    for epoch in range(max(epochs, imitation_epochs)):
        for i in range(batches_per_epoch):
            if epoch < epochs:
                out.append((epoch, i, "reward_model"))
            if epoch < imitation_epochs:
                out.append((epoch, i, "imitation_model"))
    return out


class MLP64(object):
    """float64 restatement of a one-tower network on vector observations (embedder and middleware Dense + relu under one
    linear head layer `head`) and of one whole update from a given gradient of the head's output: backward,
    l2_regularization * w on every gradient (general_network.py:354-358), TF1 Adam (as bcq_ref.MLP64)."""

    def __init__(self, named_arrays, head, lr, beta1=0.9, beta2=0.99, eps=1e-4):
        layers = {k.rsplit("/", 1)[0] for k in named_arrays}
        assert head in layers
        self.names = sorted(layers - {head}, key=lambda n: ("middleware" in n, n)) + [head]
        self.W = [np.array(named_arrays[n + "/kernel"][0], dtype=np.float64) for n in self.names]
        self.b = [np.array(named_arrays[n + "/bias"][0], dtype=np.float64) for n in self.names]
        self.lr, self.b1, self.b2, self.eps, self.t = lr, beta1, beta2, eps, 0
        self.m = [np.zeros_like(x) for x in self.W + self.b]
        self.v = [np.zeros_like(x) for x in self.W + self.b]

    def forward(self, x, keep=False):
        acts = [np.asarray(x, dtype=np.float64)]
        for i in range(len(self.W)):
            z = acts[-1] @ self.W[i] + self.b[i]
            acts.append(z if i == len(self.W) - 1 else np.maximum(z, 0.0))
        return acts if keep else acts[-1]

    def apply(self, acts, d, head_loss, l2=0.0):
        """d = dloss / d(head output) -> dict(loss, head_loss, norm) after one Adam step"""
        gW, gb = [None] * len(self.W), [None] * len(self.W)
        for i in reversed(range(len(self.W))):
            gW[i], gb[i] = acts[i].T @ d, d.sum(axis=0)
            if i:
                d = (d @ self.W[i].T) * (acts[i] > 0)
        sq = sum(float((w * w).sum()) for w in self.W + self.b)
        grads = [g + l2 * w for g, w in zip(gW + gb, self.W + self.b)]
        norm = float(np.sqrt(sum(float((g * g).sum()) for g in grads)))
        self.t += 1
        alpha = self.lr * np.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        for k, (w, g) in enumerate(zip(self.W + self.b, grads)):
            self.m[k] += (g - self.m[k]) * (1.0 - self.b1)
            self.v[k] += (g * g - self.v[k]) * (1.0 - self.b2)
            w -= self.m[k] * alpha / (np.sqrt(self.v[k]) + self.eps)
        return dict(loss=head_loss + 0.5 * l2 * sq, head_loss=head_loss, norm=norm)

    def classification_update(self, obs, labels, l2=0.0):
        """ClassificationHead: softmax cross entropy SUMMED over the batch, d = p - labels (no 1 / B)"""
        acts = self.forward(obs, keep=True)
        t = acts[-1] - acts[-1].max(axis=1, keepdims=True)
        logp = t - np.log(np.exp(t).sum(axis=1, keepdims=True))
        l = np.asarray(labels, dtype=np.float64)
        return self.apply(acts, np.exp(logp) - l, float(-(l * logp).sum()), l2)

    def bc_update(self, obs, actions):
        """BCAgent.learn_from_batch: the discrete PolicyHead's loss with targets of ones and no entropy term
        (pg_ref.head_loss in fp64)"""
        import pg_ref
        acts = self.forward(obs, keep=True)
        r = pg_ref.head_loss(acts[-1], actions, np.ones(len(actions)), 0.0, dtype=np.float64)
        return self.apply(acts, r["dlogits"], float(r["loss"]))
