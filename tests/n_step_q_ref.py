"""numpy restatement of the N-step Q agent's arithmetic on ONE update window (agents/n_step_q_agent.py:99-140 of the
reference, heads/head.py:143-186 for the Q head's loss), the twin of csrc/n_step_q.hip.

The window's targets (one value per row, written into column actions[i] of the online prediction, an fp32 array: the
assignment is the ONE rounding to fp32):
  window_targets(q_target, rewards, game_over, discount, horizon) -> fp32 [T]
The rounding points.  The reference mixes the networks' fp32 outputs, fp64 rewards (np.array of Python floats) and
Python floats; what an intermediate's type is follows numpy's promotion rule (NEP 50, numpy >= 2; the fixture
tests/golden/n_step_q.npz names its numpy).  The affected lines:
  'N-Step'
  :121  R = np.max(<fp32 [1, A]>): an np.float32 scalar.
  :124  `discount * R` on the FIRST pass of the loop: the Python float is weak, so this is an fp32 product of
        fp32(discount) and the maximum.  `batch.rewards()[i] + ...` adds an np.float64 scalar, which is not weak: R is
        fp64 from then on, and every later product and sum is fp64.  With a game over R starts as the int 0 and
        everything is fp64.
  :125  the assignment rounds R to fp32; R itself stays fp64 for the next pass.
  '1-Step'
  :114  `(1.0 - batch.game_overs()[i])`: a weak Python float minus np.bool_ -> np.float64; `* discount` -> np.float64;
        `* np.max(q_st_plus_1[i], 0)`: np.float64 times np.float32, both strong -> an fp64 product of the widened
        maximum; plus the fp64 reward; the assignment rounds once.  So this branch's `discount * max` is an fp64
        product where 'N-Step''s first one is fp32.  A game over multiplies by 0.0: the target is the reward.
(numpy < 2 promoted by VALUE: both branches then ran in fp32 after the first sum.)

The loss of a window of T rows (fp32, the Q head's convention of csrc/losses_body.hpp):
  head_loss(q_online, actions, targets, huber) -> loss, dq [T, A], td_targets [T, A], status
      e_b = q_online[b][a_b] - target_b;   l, g = e^2, 2e  (MSE)  or  the Huber terms with delta 1
      loss = (1/T) sum_b l_b,   dq[b][a_b] = ((1 * 1) * g) / T, every other entry exactly 0
  A row whose action is outside [0, A) raises status bit 0, has no term, a zero dq row, and keeps the online row as its
  td_targets row; the mean still divides by T.
  The batch sum is the device's: a3c_ref.tree_sum (thread t of 256 adds rows t, t + 256, ... in row order, then the
  256 partials are folded in halves).
"""
import numpy as np

from a3c_ref import tree_sum

F32 = np.float32
N_STEP, ONE_STEP, TARGETS_GIVEN = 0, 1, -1                           # RLX_NSTEPQ_*
HORIZONS = {'N-Step': N_STEP, '1-Step': ONE_STEP}
STATUS_BAD_ACTION, STATUS_NO_TARGET_ROWS = 1, 2


def window_targets(q_target, rewards, game_over, discount, horizon):
    """q_target fp32 [rows_t, A]: the TARGET network on the state behind the window (N_STEP; unused with a game over)
    or on the T next states (ONE_STEP; its last row unused with a game over); rewards: the filtered rewards, fp32-exact;
    game_over: the last transition's flag -> fp32 [T]"""
    r = np.asarray(rewards, dtype=np.float64).reshape(-1)
    T = r.size
    out = np.empty(T, dtype=F32)
    if horizon == N_STEP:
        # discount * R of the first pass: 0.0 with a game over, else the fp32 product (:124, see the module text)
        p = 0.0 if game_over else np.float64(F32(discount) * np.asarray(q_target, dtype=F32)[0].max())
        for i in reversed(range(T)):
            R = r[i] + p
            out[i] = R                                               # :125, the rounding
            p = discount * R
    elif horizon == ONE_STEP:
        q = np.asarray(q_target, dtype=F32)
        for i in range(T):
            over = 1.0 if (game_over and i == T - 1) else 0.0
            out[i] = r[i] + ((1.0 - over) * discount) * np.float64(q[i].max())       # :112-114
    else:
        raise ValueError("The available values for targets_horizon are: 1-Step, N-Step")
    return out


def head_loss(q_online, actions, targets, huber=False):
    """q_online fp32 [T, A], targets fp32 [T] -> dict(loss, dq, td_targets, status)"""
    q = np.asarray(q_online, dtype=F32)
    T, A = q.shape
    act, tgt = np.asarray(actions).reshape(-1), np.asarray(targets, dtype=F32).reshape(-1)
    valid = (act >= 0) & (act < A)
    a = np.where(valid, act, 0)
    rows = np.arange(T)
    e = q[rows, a] - tgt
    if huber:
        ab = np.abs(e)
        l = np.where(ab <= F32(1), F32(0.5) * e * e, ab - F32(0.5)).astype(F32)
        g = np.minimum(np.maximum(e, F32(-1)), F32(1))
    else:
        l, g = e * e, F32(2) * e
    fT = F32(T)
    loss = tree_sum(np.where(valid, l, F32(0))) / fT
    dq = np.zeros((T, A), dtype=F32)
    dq[rows[valid], a[valid]] = ((F32(1) * F32(1) * g) / fT)[valid]
    td = q.copy()
    td[rows[valid], a[valid]] = tgt[valid]
    return dict(loss=F32(loss), dq=dq, td_targets=td, status=0 if valid.all() else STATUS_BAD_ACTION)


def loss64(q_online, actions, targets, huber=False):
    """the same loss in fp64 with numpy's own sum (what the gradient test differentiates)"""
    q = np.asarray(q_online, dtype=np.float64)
    e = q[np.arange(q.shape[0]), np.asarray(actions)] - np.asarray(targets, dtype=np.float64)
    l = np.where(np.abs(e) <= 1, 0.5 * e * e, np.abs(e) - 0.5) if huber else e * e
    return l.mean()


def window_loss(q_online, q_target, actions, rewards, game_over, discount, horizon, huber=False):
    """everything rlx_nstep_q_window_loss computes.  q_target may be None or short: a non-terminal N_STEP window needs
    one row, a ONE_STEP window T rows, else status bit 1 and nothing else."""
    T = len(rewards)
    rows_t = 0 if q_target is None else len(q_target)
    if (horizon == N_STEP and not game_over and rows_t < 1) or (horizon == ONE_STEP and rows_t < T):
        return dict(status=STATUS_NO_TARGET_ROWS)
    targets = window_targets(q_target, rewards, game_over, discount, horizon)
    out = head_loss(q_online, actions, targets, huber)
    act = np.asarray(actions).reshape(-1)
    valid = (act >= 0) & (act < np.asarray(q_online).shape[1])
    return dict(out, targets=targets, valid=valid)
