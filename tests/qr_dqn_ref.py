"""numpy restatement of Quantile-Regression DQN's update arithmetic (agents/qr_dqn_agent.py:75-137 and
heads/quantile_regression_q_head.py:55-74 of the reference), the twin of csrc/qr_dqn.hip.

theta [B, A, N] fp32 (online quantiles), theta_next [B, A, N] fp32 (target quantiles on the next states).
  q_values(theta)                 -> fp64 [.., A]: np.dot with np.ones(N) / N, as get_q_values does
  targets(theta_next, r, d, g)    -> (a* [B], T [B, N] fp32): fp64 arithmetic, one rounding to fp32
  midpoints(theta_taken)          -> tau [B, N] fp32, indexed by the argsort itself (the reference's quirk), stable ties
  loss_and_grad(theta_taken, T, tau, kappa) -> (loss fp32, dtheta_taken [B, N] fp32)
  egreedy(q, u, ra, tie, eps)     -> actions: e_greedy.py:84-101 on fp64 Q values
"""
import numpy as np

F32 = np.float32


def q_values(theta):
    n = theta.shape[-1]
    return np.dot(theta, np.ones(n) / float(n))


def q_values_device_order(theta):
    """the device kernels' order: sum_j (double)theta_j * (1.0 / N), j ascending."""
    n = theta.shape[-1]
    w = 1.0 / float(n)
    s = np.zeros(theta.shape[:-1])
    for j in range(n):
        s = s + theta[..., j].astype(np.float64) * w
    return s


def targets(theta_next, rewards, game_overs, discount):
    B = theta_next.shape[0]
    a_star = np.argmax(q_values(theta_next), axis=1)
    r = np.asarray(rewards, dtype=np.float64).reshape(B, 1)
    d = np.asarray(game_overs, dtype=np.float64).reshape(B, 1)
    T = r + (1.0 - d) * discount * theta_next[np.arange(B), a_star]
    return a_star, T.astype(F32)


def midpoints(theta_taken):
    B, N = theta_taken.shape
    c = np.array(range(N + 1)) / float(N)
    mid = 0.5 * (c[1:] + c[:-1])
    out = np.tile(mid, (B, 1))
    order = np.argsort(theta_taken, axis=1, kind="stable")
    for b in range(B):
        out[b, :] = out[b, order[b]]
    return out.astype(F32)


def loss_and_grad(theta_taken, T, tau, kappa, dtype=F32):
    """quantile Huber loss, summed over the batch, and its gradient w.r.t. the taken action's atoms."""
    th = theta_taken.astype(dtype)
    e = T.astype(dtype)[:, None, :] - th[:, :, None]                        # e[b, i, j] = T_j - theta_i
    k = dtype(kappa)
    ae = np.abs(e)
    q = np.minimum(ae, k)
    h = k * (ae - q) + dtype(0.5) * (q * q)
    w = np.abs(tau.astype(dtype)[:, :, None] - (e < 0).astype(dtype))
    N = th.shape[1]
    loss = (w * h).sum(dtype=dtype) / dtype(N)
    g = -(w * np.sign(e) * q).sum(axis=2, dtype=dtype) / dtype(N)
    return dtype(loss), g.astype(dtype)


def update(theta, theta_next, actions, rewards, game_overs, discount, kappa):
    """everything rlx_qr_dqn_head_loss computes: (a*, T, tau, loss, dtheta [B, A, N])."""
    B, A, N = theta.shape
    a_star, T = targets(theta_next, rewards, game_overs, discount)
    taken = theta[np.arange(B), actions]
    tau = midpoints(taken)
    loss, g = loss_and_grad(taken, T, tau, kappa)
    d = np.zeros((B, A, N), dtype=F32)
    d[np.arange(B), actions] = g
    return a_star, T, tau, loss, d


def egreedy(q, explore_u, random_actions, tie, epsilon):
    out = np.empty(q.shape[0], dtype=np.int64)
    for e in range(q.shape[0]):
        if explore_u[e] < epsilon:
            out[e] = random_actions[e]
        else:
            out[e] = np.argmax(tie[e] * np.isclose(q[e], q[e].max()))
    return out
