"""numpy restatement of the Actor-Critic agent's arithmetic on ONE update window (agents/actor_critic_agent.py:108-186,
heads/head.py:170-181 for the V head and heads/policy_head.py:75-100 for the policy head of the reference), the twin of
csrc/a3c.hip.  The policy head is tests/pg_ref.py's; it is imported, not restated.

The window's targets (fp64, then ONE rounding to fp32 at the head's placeholders):
  discount_sum(x, g)                    -> scipy.signal.lfilter([1], [1, -g], x[::-1])[::-1] as the sequential
                                           recurrence y_i = x_i + g * y_{i+1} (a rounded product, then a rounded sum)
  window_targets(V, boot, rewards, game_over, discount, gae_lambda, rescaler, estimate_state_value_using_gae)
                                        -> the value targets and the advantages, fp64 [T] and fp32 [T]
The rounding points.  The reference mixes the network's fp32 outputs, fp64 rewards (np.array of Python floats) and
Python floats; what an intermediate's type is follows numpy's promotion rule (NEP 50, numpy >= 2; the fixture
tests/golden/a3c.npz was recorded with numpy 2.2.6 and names its numpy).  The affected lines:
  :152  `discount * R` on the FIRST pass of the A_VALUE loop, when R is the (1, 1) fp32 prediction: the Python float is
        weak, so this is an fp32 product of fp32(discount) and the prediction.  `batch.rewards()[i] + ...` adds an
        np.float64 scalar, which is not weak: R is fp64 from then on, and every later product and sum is fp64.
        With a game over R starts as the int 0 and everything is fp64.
  :154  `R - current_state_values[i]`: fp64 minus fp32 -> fp64.
  :117  `discount * values[1:]` on the fp32 array of np.append: an fp32 product with fp32(discount); adding the fp64
        rewards and subtracting the fp32 values[:-1] are fp64 operations on the widened values.
  :113  np.array(rewards.tolist() + [values[-1]]): the fp32 bootstrap widened to fp64, exactly.
  :121  `gae + values[:-1]`: fp64 plus the widened fp32 values.
(numpy < 2 promoted by VALUE: there `np.float64 scalar + fp32 array` stayed fp32 and the A_VALUE loop ran in fp32.)

The loss of a window of T rows (fp32; the forward pass has T + 1 rows when the window bootstraps, and the extra row has
no term and a zero gradient; every mean divides by T):
  head_losses(V, logits, actions, targets32, advantages32, beta, v_loss_weight, T)
      value loss  = mean_b w * (V_b - target_b)^2                 (VHead: MSE under loss_weight w = 0.5; losses[0])
      policy loss = -mean_b log pi_b(a_b) adv_b                   (losses[1]; the entropy regulariser is losses[2])
      total       = value loss + (policy loss - beta * mean entropy)
      dV_b = (w * (2 (V_b - target_b))) / T,   dlogits = pg_ref.head_loss's
  The batch sums are the device's: thread t of 256 adds the terms of rows t, t + 256, ... in row order, then the 256
  partials are folded in halves (tree_sum).  pg_ref.head_loss sums with np.sum, so the two scalars it would give are
  re-summed here from pg_ref.head_rows' row terms; its dlogits and status are used as they are.
"""
import numpy as np

import pg_ref

F32 = np.float32
A_VALUE, GAE = 5, 8                                                  # PolicyGradientRescaler's values
THREADS = 256
STATUS_BAD_ACTION, STATUS_NO_BOOTSTRAP_ROW = 1, 2


def discount_sum(x, g):
    """ActorCriticAgent.discount (:108-109): y_i = x_i + g * y_{i+1}, y_n = 0, fp64, one step after the other"""
    x = np.asarray(x, dtype=np.float64)
    y = np.empty_like(x)
    p = 0.0                                                          # g * y_{i+1}
    for i in reversed(range(x.size)):
        y[i] = x[i] + p
        p = g * y[i]
    return y


def window_targets(V, boot, rewards, game_over, discount, gae_lambda=0.96, rescaler=A_VALUE, estimate_with_gae=False):
    """V fp32 [T]: the V head on the window's states; boot: the V head on the last next state (fp32; unused with a game
    over); rewards: the filtered rewards, fp32-exact -> dict(targets, advantages: fp64 [T]; targets32, advantages32)"""
    V = np.asarray(V, dtype=F32).reshape(-1)
    r = np.asarray(rewards, dtype=np.float64).reshape(-1)
    T = V.size
    V64 = V.astype(np.float64)
    last = F32(0) if game_over else F32(boot)
    if rescaler == A_VALUE:
        targets, adv = np.empty(T), np.empty(T)
        # discount * R of the first pass: 0.0 with a game over, else the fp32 product (see the module text)
        p = 0.0 if game_over else np.float64(F32(discount) * last)
        for i in reversed(range(T)):
            R = r[i] + p
            targets[i] = R
            adv[i] = R - V64[i]
            p = discount * R
    elif rescaler == GAE:
        values = np.append(V, last)                                  # fp32 [T + 1]
        deltas = (r + (F32(discount) * values[1:]).astype(np.float64)) - values[:-1].astype(np.float64)
        adv = discount_sum(deltas, discount * gae_lambda)
        if estimate_with_gae:
            targets = adv + V64
        else:
            targets = discount_sum(np.append(r, np.float64(values[-1])), discount)[:-1]
    else:
        raise ValueError("The requested policy gradient rescaler is not available")
    return dict(targets=targets, advantages=adv, targets32=targets.astype(F32), advantages32=adv.astype(F32))


def tree_sum(terms):
    """the device's batch sum of fp32 row terms: thread t adds rows t, t + 256, ... in row order from 0.0, then the 256
    partials are folded in halves"""
    part = np.zeros(THREADS, dtype=F32)
    terms = np.asarray(terms, dtype=F32)
    for b0 in range(0, terms.size, THREADS):
        chunk = terms[b0:b0 + THREADS]
        part[:chunk.size] = part[:chunk.size] + chunk
    s = THREADS // 2
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def head_losses(V, logits, actions, targets32, advantages32, beta, v_loss_weight=0.5, T=None):
    """V [R], logits [R, A] with R = T or T + 1 -> the four scalars, dV [R], dlogits [R, A], status"""
    V = np.asarray(V, dtype=F32).reshape(-1)
    x = np.asarray(logits, dtype=F32)
    R, A = x.shape
    T = R if T is None else T
    tgt, adv = np.asarray(targets32, dtype=F32)[:T], np.asarray(advantages32, dtype=F32)[:T]
    fT, w, b = F32(T), F32(v_loss_weight), F32(beta)
    d = V[:T] - tgt
    value_loss = tree_sum(w * (d * d)) / fT
    dV = np.zeros(R, dtype=F32)
    dV[:T] = (w * (F32(2) * d)) / fT
    pol = pg_ref.head_loss(x, actions, adv, beta, T=T)
    act = np.asarray(actions)[:T]
    valid = (act >= 0) & (act < A)
    p, q, S, lp, H = pg_ref.head_rows(x[:T])
    a = np.where(valid, act, 0)
    zero = F32(0)
    mean_h = tree_sum(np.where(valid, H, zero)) / fT
    policy_loss = -(tree_sum(np.where(valid, lp[np.arange(T), a] * adv, zero)) / fT)
    total = value_loss + (policy_loss - b * mean_h)
    return dict(loss=total, value_loss=value_loss, policy_loss=policy_loss, entropy=mean_h, dV=dV,
                dlogits=pol["dlogits"], status=pol["status"])


def window_loss(V, logits, actions, rewards, game_over, discount, gae_lambda, rescaler, estimate_with_gae, beta,
                v_loss_weight=0.5):
    """everything rlx_a3c_window_loss computes: V [R], logits [R, A] with R = T + 1 (the last row is the bootstrap
    state) or R = T (allowed only with a game over)"""
    V = np.asarray(V, dtype=F32).reshape(-1)
    T = len(rewards)
    if V.size == T and not game_over:
        return dict(status=STATUS_NO_BOOTSTRAP_ROW)
    w = window_targets(V[:T], V[T] if V.size > T else 0, rewards, game_over, discount, gae_lambda, rescaler,
                       estimate_with_gae)
    return dict(w, **head_losses(V, logits, actions, w["targets32"], w["advantages32"], beta, v_loss_weight, T))
