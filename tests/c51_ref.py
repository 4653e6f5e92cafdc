"""numpy restatement of Categorical DQN's arithmetic (agents/categorical_dqn_agent.py:86-167 and
heads/categorical_q_head.py:42-58 of the reference), the twin of csrc/c51.hip.

logits [.., A, N] fp32 (the head's Dense output), z [N] fp64 (np.linspace(v_min, v_max, N)).
  softmax(logits)                      -> fp32 [.., A, N]: the kernels' softmax, bit for bit (max, fp64 exp rounded once,
                                          fp32 sum in atom order, fp32 division)
  q_values(p, z)                       -> fp64 [.., A]: np.dot, as distribution_prediction_to_q_values does
  q_values_device_order(p, z)          -> the same sum taken with j ascending, as the kernels take it
  project(p_next, z, r, d, g, order)   -> (a* [B], m [B, N] fp32): the reference's loop, fp64, one rounding to fp32
  cross_entropy(logits, labels)        -> [B, A]: softmax_cross_entropy_with_logits
  loss_and_grad(logits, m, actions)    -> ([B, A] losses, their sum, dlogits = softmax - labels on the taken action)
  update(...)                          -> everything rlx_c51_head_loss computes
  egreedy(q, u, ra, tie, eps)          -> actions: e_greedy.py:84-101 on fp64 Q values
"""
import numpy as np

F32 = np.float32


def support(v_min, v_max, atoms):
    return np.linspace(v_min, v_max, atoms)


def softmax(logits):
    x = np.asarray(logits, dtype=F32)
    mx = x.max(axis=-1, keepdims=True)
    e = np.exp((x - mx).astype(np.float64)).astype(F32)
    s = np.zeros(x.shape[:-1], dtype=F32)
    for j in range(x.shape[-1]):
        s = s + e[..., j]
    return e / s[..., None]


def softmax_f64(logits):
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def q_values(p, z):
    return np.dot(p, z)


def q_values_device_order(p, z):
    s = np.zeros(p.shape[:-1])
    for j in range(p.shape[-1]):
        s = s + p[..., j].astype(np.float64) * z[j]
    return s


def overhangs(z):
    """True where (z[-1] - z[0]) / (z[1] - z[0]) rounds to more than N - 1 (np.linspace(-10, 10, 256) does; the default
    51 atoms do not): an atom clipped at v_max then has ceil(bj) == N, and the reference raises IndexError."""
    return bool((z[-1] - z[0]) / (z[1] - z[0]) > z.size - 1)


def project(p_next, z, rewards, game_overs, discount, device_order=False, overhang="raise"):
    """categorical_dqn_agent.py:121-149 on the target network's distributions p_next [B, A, N].  overhang="drop": a
    contribution to the non-existent atom N (see overhangs(); its weight bj - l is a rounding error) is left out, as the
    kernel does, instead of raising as the reference would."""
    B = p_next.shape[0]
    q = q_values_device_order(p_next, z) if device_order else q_values(p_next, z)
    a_star = np.argmax(q, axis=1)
    r = np.asarray(rewards, dtype=np.float64)
    d = np.asarray(game_overs, dtype=np.float64)
    m = np.zeros((B, z.size))
    rows = np.arange(B)
    for j in range(z.size):
        tzj = np.fmax(np.fmin(r + (1.0 - d) * discount * z[j], z[-1]), z[0])
        bj = (tzj - z[0]) / (z[1] - z[0])
        u = (np.ceil(bj)).astype(int)
        l = (np.floor(bj)).astype(int)
        m[rows, l] += (p_next[rows, a_star, j] * (u - bj))
        ok = u < z.size if overhang == "drop" else slice(None)
        m[rows[ok], u[ok]] += (p_next[rows, a_star, j] * (bj - l))[ok]
    return a_star, m.astype(F32)


def cross_entropy(logits, labels, dtype=F32):
    """softmax_cross_entropy_with_logits: sum_j labels_j * (log sum_k exp(x_k - mx) - (x_j - mx)) -> [.., A]."""
    x = np.asarray(logits, dtype=dtype)
    sh = x - x.max(axis=-1, keepdims=True)
    if dtype is F32:
        e = np.exp(sh.astype(np.float64)).astype(F32)
        s = np.zeros(x.shape[:-1], dtype=F32)
        for j in range(x.shape[-1]):
            s = s + e[..., j]
    else:
        s = np.exp(sh).sum(axis=-1)
    return (np.asarray(labels, dtype=dtype) * (np.log(s)[..., None] - sh)).sum(axis=-1, dtype=dtype)


def loss_and_grad(logits, m, actions, dtype=F32):
    """labels = m for the taken action, the online softmax itself elsewhere (categorical_dqn_agent.py:153);
    -> (cross entropies [B, A], their sum over batch AND actions, dlogits [B, A, N] = softmax - labels: the gradient of
    TensorFlow's fused op, which is exactly zero off the taken action)."""
    B, A, N = logits.shape
    rows = np.arange(B)
    p = softmax(logits) if dtype is F32 else softmax_f64(logits)
    labels = p.copy()
    labels[rows, actions] = m
    ce = cross_entropy(logits, labels, dtype)
    d = np.zeros((B, A, N), dtype=dtype)
    d[rows, actions] = p[rows, actions] - m
    return ce, ce.sum(dtype=dtype), d


def update(logits, logits_next, z, actions, rewards, game_overs, discount, device_order=True, dtype=F32,
           overhang="raise"):
    """-> dict(a_star, m, action_losses [B, A], loss, dlogits [B, A, N], errors [B] fp64): everything
    rlx_c51_head_loss computes.  dtype=np.float64 evaluates the softmax-dependent values (loss, gradient, errors) in
    fp64 from the same a* and m."""
    a_star, m = project(softmax(logits_next), z, rewards, game_overs, discount, device_order, overhang)
    ce, loss, d = loss_and_grad(logits, m, actions, dtype)
    return dict(a_star=a_star, m=m, action_losses=ce, loss=loss, dlogits=d,
                errors=ce[np.arange(logits.shape[0]), actions].astype(np.float64))


def egreedy(q, explore_u, random_actions, tie, epsilon):
    out = np.empty(q.shape[0], dtype=np.int64)
    for e in range(q.shape[0]):
        if explore_u[e] < epsilon:
            out[e] = random_actions[e]
        else:
            out[e] = np.argmax(tie[e] * np.isclose(q[e], q[e].max()))
    return out
