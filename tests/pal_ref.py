"""numpy restatement of the Persistent Advantage Learning and Mixed Monte Carlo targets (agents/pal_agent.py:70-111,
agents/mmc_agent.py:57-83 of the reference), of the Q head's loss on them (heads/q_head.py + head.py:172-181) and of
its gradient: the twin of csrc/pal.hip, pinned to the reference's own agents by tests/test_pal_mmc_ref.py.

Per row i with taken action a (all Q arrays [B, A] fp32, total_returns fp64):
    sel = first argmax of q_sel[i]                                   (the online network on s')
    y   = r + (1 - game_over) * discount * q_next[i][sel]            fp64, stored into the fp32 array      (rounding 1)
  PAL (q_cur, the target network on s, is given):
    adv  = max(q_cur[i]) - q_cur[i][a]                               fp32 - fp32
    adv' = max(q_next[i]) - q_next[i][sel]                           fp32 - fp32
    T    = fp32(y) - fp32(alpha) * (min(adv, adv') if persistent else adv)    an fp32 product, an fp32 subtraction  (2)
    T    = fp32( fp64(fp32(1 - rate) * T) + rate * MC )              an fp32 product, an fp64 product, an fp64 sum   (3)
  MMC (q_cur is None):
    T    = fp32( (1 - rate) * y + rate * MC )                        all fp64, rounded once

The fp32 products are what the reference's expressions give under numpy >= 2 (NEP 50): a Python float times an
np.float32 scalar stays float32, so `self.alpha * min(...)` and `(1 - rate) * TD_targets[i, a]` are fp32 products with
fp32(alpha) and fp32 of the Python double 1 - rate.  Under numpy 1.x value-based casting made both products fp64 (the
scalar was promoted); the goldens (tests/golden/pal_mmc.npz) were recorded under numpy 2.2.6 and decide for the
arithmetic above.

  targets(...)       -> TD targets [B, A] fp32 (q_online except at [i, a_i])
  loss_and_grad(...) -> (loss, dq [B, A]) fp32: the row terms summed in the kernel's tree — blockDim leaves (64 doubled
                        until it holds the batch, rows beyond it zeros), halving strides — then divided by B
  update(...)        -> dict(td_targets, dq, loss, terms)
"""
import numpy as np

F32 = np.float32


def targets(q_online, q_cur, q_next, q_sel, actions, rewards, game_overs, total_returns, discount, alpha=0.9,
            persistent=False, rate=0.1):
    B, A = q_online.shape
    td = np.array(q_online, dtype=F32)
    a32, keep32 = F32(alpha), F32(1.0 - rate)
    for i in range(B):
        a = int(actions[i])
        sel = int(np.argmax(q_sel[i]))
        y = np.float64(rewards[i]) + (1.0 - np.float64(bool(game_overs[i]))) * discount * np.float64(q_next[i][sel])
        mc = np.float64(total_returns[i])
        if q_cur is None:
            td[i, a] = (1.0 - rate) * y + rate * mc
            continue
        t = F32(y)
        adv = F32(np.max(q_cur[i]) - q_cur[i][a])
        if persistent:
            adv = min(adv, F32(np.max(q_next[i]) - q_next[i][sel]))
        t = F32(t - F32(a32 * adv))
        td[i, a] = np.float64(F32(keep32 * t)) + rate * mc
    return td


def tree_leaves(B):
    n = 64
    while n < B:
        n <<= 1
    return n


def loss_and_grad(q_online, td_targets, actions, huber, grad_scale=1.0):
    B, A = q_online.shape
    rows = np.arange(B)
    e = (q_online[rows, actions] - td_targets[rows, actions]).astype(F32)
    if huber:
        ae = np.abs(e)
        l = np.where(ae <= 1, F32(0.5) * e * e, ae - F32(0.5)).astype(F32)
        g = np.clip(e, -1, 1).astype(F32)
    else:
        l = (e * e).astype(F32)
        g = (F32(2) * e).astype(F32)
    n = tree_leaves(B)
    red = np.zeros(n, dtype=F32)
    red[:B] = l
    d = n >> 1
    while d > 0:
        red[:d] = red[:d] + red[d:2 * d]
        d >>= 1
    dq = np.zeros((B, A), dtype=F32)
    dq[rows, actions] = (F32(grad_scale) * g / F32(B)).astype(F32)
    return F32(red[0] / F32(B)), dq, l


def update(q_online, q_cur, q_next, q_sel, actions, rewards, game_overs, total_returns, discount, alpha, persistent,
           rate, huber, grad_scale=1.0):
    td = targets(q_online, q_cur, q_next, q_sel, actions, rewards, game_overs, total_returns, discount, alpha,
                 persistent, rate)
    loss, dq, terms = loss_and_grad(q_online, td, actions, huber, grad_scale)
    return dict(td_targets=td, dq=dq, loss=loss, terms=terms)
