"""What the target-kernel tests hold csrc/targets.hip to: one numpy function per entry point.

The TD-target arithmetic itself is NOT restated here.  oracle/targets.py states it (dqn_targets, ac_td_targets,
td3_smooth_actions) and tests/golden/targets.npz pins that module to the reference agents' own learn_from_batch.  This
module adds what the entry points have and the oracle has not: the status word and the rows it protects, `q_stride`, the
per-dimension action bounds, the three-block layout of the merged critic inputs, the head loss with its gradient, the
order of the loss sum, and the Q head's backward pass with its error bounds.

Two rules come from numpy, not from a sentence written here:
  selection is np.argmax    -> the FIRST maximum wins, and a NaN counts as the maximum: the first NaN of a row wins;
  every clip is np.clip     -> a NaN value stays NaN (C's fmin / fmax would return the bound).

Every rounding point, by name:
  y64    the TD target in float64, the oracle's expression: r + (1.0 - done) * discount * q_next[a*], left to right
  y32    fp32(y64): the ONE rounding of the target, on its way into the fp32 target matrix (dqn_agent.py:103)
  err    |y64 - float64(q[b][a_b])| in float64 (dqn_agent.py:102): it sees y64, not y32
  e      fp32: q[b][a_b] - y32, one fp32 subtraction
  w      fp32(weight): the float64 importance weight is fed to an fp32 placeholder
  l, g   MSE: e*e and 2e.  Huber: 0.5*e*e for |e| <= 1, |e| - 0.5 otherwise, and clip(e, -1, 1).  fp32, left to right
  term   fp32: w * l
  dq     fp32: ((grad_scale * w) * g) / fp32(B), left to right, at [b][a_b]; exactly 0.0 in the row's other columns
  loss   loss_f32: the halving tree below over `threads` terms, then one division by fp32(B)
         loss_f64: the mean of float64(w) * l(float64(q) - float64(y32)), everything after y32 in float64

`done` is a byte and only its truth counts (0 / 1 / 255): the wrappers turn it into a bool before the oracle sees it.

  dqn_targets(...)          -> (fp32 matrix, float64 errors, status)
  dqn_head_loss(...)        -> dict(dq, td_errors, td_targets, loss_f32, loss_f64, valid, nan_huber, status)
  loss_threads(B), loss_tree_f32(terms, B), loss_bound(B, terms)
  ac_td_targets(...), td3_smooth_actions(...), ac_merge_inputs(...), sac_value_targets(...)
  head_backward(x, w, dq, lower_activation) -> dict(dw, db, dx, dw_bound, db_bound, dx_bound), float64"""
import numpy as np

from oracle import targets as T

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24                       # fp32 unit roundoff
TINY = 2.0 ** -149                   # the smallest fp32 denormal: what one underflowing operation can lose


def gamma(n, u=U):
    """Higham's gamma_n = n u / (1 - n u): (1 + d_1) ... (1 + d_n) = 1 + t with |t| <= gamma_n for |d_i| <= u"""
    return n * u / (1.0 - n * u)


def _valid_rows(actions, A):
    actions = np.asarray(actions)
    return (actions >= 0) & (actions < A)


# ------------------------------------------------------------------------------------------------ rlx_dqn_targets

def dqn_targets(q_next_t, q_sel, td_targets, actions, rewards, dones, discount):
    """td_targets: Q_online(s, .) on entry, fp32 [B, A].  q_sel None: the target net selects (DQN).
    -> (fp32 [B, A], float64 |TD errors| [B], status).  A row whose action is outside [0, A) keeps its entry values
    (its error is NaN here: the entry point leaves that element unwritten) and sets bit 0 of the status."""
    q_next_t = np.asarray(q_next_t, dtype=F32)
    td_targets = np.array(td_targets, dtype=F32, copy=True)
    B, A = td_targets.shape
    actions = np.asarray(actions)
    ok = _valid_rows(actions, A)
    errors = np.full(B, np.nan, dtype=F64)
    if ok.any():
        done = np.asarray(dones)[ok] != 0
        with np.errstate(invalid="ignore", over="ignore"):
            tt, err = T.dqn_targets(q_next_t[ok], td_targets[ok], actions[ok], np.asarray(rewards, dtype=F32)[ok], done,
                                    discount, q_next_online=None if q_sel is None else np.asarray(q_sel, dtype=F32)[ok])
        td_targets[ok] = tt
        errors[ok] = err
    return td_targets, errors, 0 if ok.all() else 1


# ------------------------------------------------------------------------------------------------ rlx_dqn_head_loss

def loss_threads(B):
    """the launch's block size: the smallest power of two >= max(64, B)"""
    t = 64
    while t < B:
        t *= 2
    return t


def loss_tree_f32(terms, B):
    """The kernel's own sum: thread i < B holds term i, every other thread of the block 0.0f; red[i] += red[i + d] for
    d = threads / 2, threads / 4, ... 1; then one division by fp32(B)."""
    red = np.zeros(loss_threads(B), dtype=F32)
    red[:B] = np.asarray(terms, dtype=F32)
    d = red.size // 2
    with np.errstate(invalid="ignore", over="ignore"):
        while d > 0:
            red[:d] = red[:d] + red[d:2 * d]
            d //= 2
        return red[0] / F32(B)


def loss_bound(B, terms64):
    """|loss_f32 - loss_f64| <= gamma_(log2(threads) + 5) * mean_b |w_b l_b|  +  (5 B + threads) * TINY / B.

    Per term, against the float64 value of w * l(e) with e = q - y32 exact in float64 (both operands are fp32 numbers, the
    float64 difference is exact):
      e_hat = e (1 + d1)                                          the fp32 subtraction
      MSE:           l_hat = e^2 (1 + d1)^2 (1 + d2)              one product                          -> 3 factors
      Huber, |e|<=1: 0.5 * e_hat is exact, times e_hat: the same 3 factors.  (|e| <= 1 implies |e_hat| <= 1: rounding is
                     monotonic and 1 is an fp32 number, so the branch is the exact one.)
      Huber, |e|>1:  l_hat = (|e| (1 + d1) - 0.5)(1 + d2); |e| / (|e| - 0.5) < 2, so the error d1 of e is at most 2 |d1|
                     relative to l                                                                     -> 3 factors
                     (|e_hat| may round to exactly 1 and take the quadratic branch: 0.5 against |e| - 0.5 with
                     1 < |e| <= 1 + u, a relative error below 2 u, inside the same 3 factors.)
      term = w l_hat (1 + d3)                                                                          -> 4 factors
    A term then passes through log2(threads) additions of the halving tree -- the zeros of the threads past B are added
    exactly, but every level still rounds the running sum -- and one division by fp32(B), which is B exactly (B <= 1024):
    log2(threads) + 1 further factors.  The second summand covers results that underflow (none does in the tests)."""
    depth = int(np.log2(loss_threads(B)))
    return gamma(depth + 5) * float(np.mean(np.abs(terms64))) + (5 * B + loss_threads(B)) * TINY / B


def _huber_or_mse(e, huber):
    """(l, g) in e's own precision, the kernel's expressions in its order"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if not huber:
            return e * e, e.dtype.type(2.0) * e
        ae = np.abs(e)
        half = e.dtype.type(0.5)
        return np.where(ae <= 1, half * e * e, ae - half), np.clip(e, -1, 1)


def dqn_head_loss(q, q_next_t, q_sel, actions, rewards, dones, weights, discount, huber, grad_scale):
    """q, q_next_t, q_sel: fp32 [B, A] (q_sel None: DQN).  weights: float64 [B] or None.
    -> dict: dq fp32 [B, A] (rows outside `valid` are 0.0: what the one-launch form writes; the stand-alone kernel leaves
       them unwritten), td_errors float64 [B] and td_targets fp32 [B, A] (rows outside `valid`: NaN / q), loss_f32,
       loss_f64, valid [B] bool, nan_huber [B] bool (Huber rows whose e is NaN: their dq[b][a_b] is left out of the
       comparison), status."""
    q = np.asarray(q, dtype=F32)
    B, A = q.shape
    actions = np.asarray(actions)
    td_targets, td_errors, status = dqn_targets(q_next_t, q_sel, q, actions, rewards, dones, discount)
    ok = _valid_rows(actions, A)
    rows = np.nonzero(ok)[0]
    act = actions[rows]
    qa, y32 = q[rows, act], td_targets[rows, act]                  # y32: rounded ONCE, by the assignment into the matrix
    w = np.ones(B, dtype=F32) if weights is None else np.asarray(weights, dtype=F64).astype(F32)
    w = w[rows]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        e = qa - y32                                                # fp32
        l, g = _huber_or_mse(e, huber)
        term = np.zeros(B, dtype=F32)
        term[rows] = w * l
        dq = np.zeros((B, A), dtype=F32)
        dq[rows, act] = F32(grad_scale) * w * g / F32(B)
        e64 = qa.astype(F64) - y32.astype(F64)
        l64, _ = _huber_or_mse(e64, huber)
        term64 = np.zeros(B, dtype=F64)
        term64[rows] = w.astype(F64) * l64
    nan_huber = np.zeros(B, dtype=bool)
    nan_huber[rows] = np.isnan(e) & bool(huber)
    return dict(dq=dq, td_errors=td_errors, td_targets=td_targets, loss_f32=loss_tree_f32(term, B),
                loss_f64=F64(term64.sum() / B), loss_bound=loss_bound(B, term64), terms64=term64, valid=ok,
                nan_huber=nan_huber, status=status)


# ------------------------------------------------------------------------------------------------ actor-critic targets

def ac_td_targets(rewards, dones, q_next, q_stride, discount, use_non_zero_discount_for_terminal_states, clip):
    """q_next: fp32 with `q_stride` values per row, of which the first is read.  clip: None or (low, high).
    -> fp32 [B]: the oracle's float64 target, rounded once.
    The oracle is handed what the reference's agents hold: float64 rewards and game_overs, a python float discount and
    the fp32 network output.  So numpy evaluates (1.0 - game_overs) * discount * q_next in float64, but the
    `discount * q_next` of the non-zero-terminal-discount branch as an fp32 product: fp32(discount) * q_next, rounded
    to fp32, and only its sum with the rewards in float64."""
    q = np.asarray(q_next, dtype=F32).reshape(len(rewards), q_stride)[:, :1]
    assert isinstance(discount, float)                              # a np.float64 would promote the product
    done = np.asarray(dones) != 0
    with np.errstate(invalid="ignore", over="ignore"):
        t = T.ac_td_targets(np.asarray(rewards, dtype=F32), done, q, discount,
                            bool(use_non_zero_discount_for_terminal_states), clip)
        return t[:, 0].astype(F32)


def td3_smooth_actions(next_actions, noise, noise_clipping, low, high):
    """low / high: fp32 [A], one bound per action dimension -> fp32 [B, A]"""
    with np.errstate(invalid="ignore", over="ignore"):
        sm = T.td3_smooth_actions(np.asarray(next_actions, dtype=F32), np.asarray(noise, dtype=F64), noise_clipping,
                                  np.asarray(low, dtype=F32).astype(F64), np.asarray(high, dtype=F32).astype(F64))
        return sm.astype(F32)


def ac_merge_inputs(actions, obs, next_actions, noise, noise_clipping, low, high, next_obs):
    """-> (merged2 fp32 [2, B, A + D], obs_columns fp32 [B, D]): block 0 = [actions | obs], block 1 = [a' | next_obs] with
    a' = next_actions (noise None: DDPG, neither bound is looked at) or their smoothed values (TD3); the third block's
    observation columns equal obs and its action columns are not written."""
    actions, obs = np.asarray(actions, dtype=F32), np.asarray(obs, dtype=F32)
    next_actions, next_obs = np.asarray(next_actions, dtype=F32), np.asarray(next_obs, dtype=F32)
    a2 = next_actions if noise is None else td3_smooth_actions(next_actions, noise, noise_clipping, low, high)
    return np.stack([np.concatenate([actions, obs], 1), np.concatenate([a2, next_obs], 1)]), obs.copy()


def sac_value_targets(q_min, logprob):
    """soft_actor_critic_agent.py:244: both operands are fp32 arrays in the reference, one fp32 subtraction"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(q_min, dtype=F32) - np.asarray(logprob, dtype=F32)


# ------------------------------------------------------------------------------------------------ the head's backward pass

def act_deriv_out(y, kind):
    """derivative of the lower layer's activation, from its OUTPUT y (float64): 0 none, 1 relu, 2 tanh"""
    if kind == 1:
        return (y > 0).astype(F64)
    if kind == 2:
        return 1.0 - y * y
    return np.ones_like(y)


def head_backward(x, w, dq, lower_activation):
    """x fp32 [B, K] (the lower layer's output), w fp32 [K, N], dq fp32 [B, N] -> float64 dw [K, N], db [N], dx [B, K]
    and a bound on the error of ANY fp32 evaluation of each:

    dw[k][n] = sum_b x[b][k] dq[b][n]: B products and B - 1 additions.  Whatever the order, and whether or not a product
      and its addition are fused, a term passes through at most B roundings: |dw_hat - dw| <= gamma_B sum_b |x| |dq|.
    db[n] = sum_b dq[b][n]: at most B - 1 additions per term, gamma_B sum_b |dq| covers it.
    dx[b][k] = (sum_n dq[b][n] w[k][n]) * act'(x[b][k]): with m = the largest number of non-zero dq in a row (1 for the
      DQN head: only the taken action's column), the sum has m products and the zeros add nothing: s_hat = s (1 + t),
      |t| <= gamma_m, taken over |dq| |w|.  none: dx = s.  relu: times an exact 0 or 1.  tanh: f_hat = fl(1 - fl(y y))
      = (1 - y^2)(1 + d3) - y^2 d2 (1 + d3), and one more product, so
      |dx_hat - dx| <= gamma_(m+2) S |1 - y^2| + u (1 + gamma_(m+2)) S y^2  with  S = sum_n |dq| |w|.
    Each bound carries TINY per operation for results that underflow."""
    x64, w64, d64 = (np.asarray(a, dtype=F32).astype(F64) for a in (x, w, dq))
    B = x64.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        dw = x64.T @ d64
        db = d64.sum(0)
        s = d64 @ w64.T
        S = np.abs(d64) @ np.abs(w64).T
        f = act_deriv_out(x64, lower_activation)
        dx = s * f
        m = max(1, int((d64 != 0).sum(1).max()))
        dw_bound = gamma(B) * (np.abs(x64).T @ np.abs(d64)) + 2 * B * TINY
        db_bound = gamma(B) * np.abs(d64).sum(0) + B * TINY
        if lower_activation == 2:
            y2 = x64 * x64
            dx_bound = gamma(m + 2) * S * np.abs(1.0 - y2) + U * (1.0 + gamma(m + 2)) * S * y2 + (2 * m + 3) * TINY
        else:
            dx_bound = gamma(m) * S * f + (2 * m + 1) * TINY
    return dict(dw=dw, db=db, dx=dx, dw_bound=dw_bound, db_bound=db_bound, dx_bound=dx_bound)


def within(got, want, bound):
    """every finite reference value is met to its bound; where the reference is NaN the result is NaN, where it is
    infinite the result is that infinity.  -> (ok, the worst |error| / bound over the finite entries)"""
    got, want, bound = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64), np.asarray(bound, dtype=F64)
    fin = np.isfinite(want) & np.isfinite(bound)
    nan, inf = np.isnan(want), np.isinf(want)
    ok = bool(np.isnan(got[nan]).all()) and np.array_equal(got[inf], want[inf])
    err = np.abs(got[fin] - want[fin])
    ok = ok and bool((err <= bound[fin]).all())
    ratio = float((err[bound[fin] > 0] / bound[fin][bound[fin] > 0]).max()) if (bound[fin] > 0).any() else 0.0
    return ok, ratio
