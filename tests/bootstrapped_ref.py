"""numpy restatement of Bootstrapped DQN's update and acting arithmetic (agents/bootstrapped_dqn_agent.py:57-86,
exploration_policies/bootstrapped.py:72-85, heads/q_head.py + head.py:172-181 of the reference), the twin of
csrc/bootstrapped_dqn.hip.

Q arrays are [K, B, A] fp32 (head, row, action), masks [B, K] of 0 / 1.
  targets(q_online, q_next, q_sel, actions, r, d, masks, g) -> (a* [B, K], TD targets [K, B, A] fp32): per head and row
      with its bit set the Double-DQN target in fp64, rounded to fp32 once when it is stored; the online prediction
      everywhere else
  loss_and_grad(q_online, td_targets, huber) -> (total, head losses [K], dq [K, B, A]) in fp32: per head
      mean_b sum_a l(target, q), the total their sum in head order
  update(...)                     -> everything rlx_bootstrapped_dqn_head_loss computes
  action_values(q [n, K, A], heads, vote) -> [n, A]: the selected head's values, or the vote's one-hot vector
  egreedy(values, u, ra, tie, eps) -> actions: e_greedy.py:84-101
  mask_words(masks)               -> uint32 [B], bit h = head h
"""
import numpy as np

F32 = np.float32


def mask_words(masks):
    m = np.asarray(masks, dtype=np.uint64)
    return (m << np.arange(m.shape[-1], dtype=np.uint64)).sum(axis=-1).astype(np.uint32)


def targets(q_online, q_next, q_sel, actions, rewards, game_overs, masks, discount):
    K, B, A = q_online.shape
    td = q_online.copy()
    a_star = np.zeros((B, K), dtype=np.int64)
    for i in range(B):
        for h in range(K):
            a_star[i, h] = np.argmax(q_sel[h][i], 0)
            if masks[i][h] == 1:
                td[h][i, actions[i]] = np.float64(rewards[i]) + (1.0 - np.float64(game_overs[i])) * discount * \
                    np.float64(q_next[h][i][a_star[i, h]])
    return a_star, td


def loss_and_grad(q_online, td_targets, huber, grad_scale=1.0):
    K, B, A = q_online.shape
    e = (q_online - td_targets).astype(F32)
    if huber:
        ae = np.abs(e)
        l = np.where(ae <= 1, F32(0.5) * e * e, ae - F32(0.5)).astype(F32)
        g = np.clip(e, -1, 1).astype(F32)
    else:
        l = (e * e).astype(F32)
        g = (F32(2) * e).astype(F32)
    head_losses = (l.sum(axis=2, dtype=F32).sum(axis=1, dtype=F32) / F32(B)).astype(F32)
    total = F32(0)
    for h in range(K):
        total = F32(total + head_losses[h])
    return total, head_losses, (F32(grad_scale) * g / F32(B)).astype(F32)


def update(q_online, q_next, q_sel, actions, rewards, game_overs, masks, discount, huber):
    a_star, td = targets(q_online, q_next, q_sel, actions, rewards, game_overs, masks, discount)
    total, head_losses, dq = loss_and_grad(q_online, td, huber)
    return dict(a_star=a_star, td_targets=td, loss=total, head_losses=head_losses, dq=dq)


def columns(x):
    """[K, B, A] -> the head layer's layout [B, K * A] (column h * A + a)."""
    K, B, A = x.shape
    return np.ascontiguousarray(np.transpose(x, (1, 0, 2)).reshape(B, K * A))


def action_values(q, heads, vote):
    n, K, A = q.shape
    out = np.zeros((n, A), dtype=F32)
    for e in range(n):
        if not vote:
            out[e] = q[e, heads[e]]
        else:
            top = np.argmax(np.bincount(np.argmax(q[e], axis=-1)))
            out[e] = np.eye(A)[top]
    return out


def egreedy(values, explore_u, random_actions, tie, epsilon):
    out = np.empty(values.shape[0], dtype=np.int64)
    for e in range(values.shape[0]):
        if explore_u[e] < epsilon:
            out[e] = random_actions[e]
        else:
            out[e] = np.argmax(tie[e] * np.isclose(values[e], values[e].max()))
    return out
