"""numpy float64 restatement of the head losses of csrc/losses.hip (and the softmax that csrc/explore.hip repeats),
written from the reference's formulas (paths under rl_coach/architectures/tensorflow_components/heads/): head.py:143-186
(loss = mean_b(loss_weight * w_b * sum_dims l)), q_head.py / v_head.py (l = mean squared error, or huber with delta 1),
ppo_head.py:52-144 (Categorical / MultivariateNormalDiag log-probabilities, likelihood ratio, clipped surrogate, entropy,
KL) and the TD target of an actor-critic update (agents/ddpg_agent.py:156-164, td3_agent.py:168-180) -- NOT from
oracle/losses.py, which this module never imports: tests/test_head_loss_ref.py compares the two.

Every function takes the fp32 device inputs and evaluates in float64.  Next to every value it returns `units`: the bound
on the kernel's rounding error in units of 2^-24 (U24, the relative error of one fp32 rounding), so that a tolerance is

    U24 * units,        units = sum over the kernel's fp32 operations of  c_op * (the magnitude that operation perturbs)

with every c_op COUNTED from the kernel's chain of operations and written down in the function's docstring -- none is
measured.  The counting rules:
  * +, -, *, / round once: 1 unit of the result's magnitude (HIP's fp32 division is correctly rounded); a product that
    the compiler contracts into an FMA rounds less often, never more;
  * a sum of n terms added in sequence: n - 1 units of sum |terms|;
  * the workgroup sum over the batch (a per-thread stride loop, then the LDS tree): sum_depth(batch) units of sum |terms|;
  * expf is documented at 1 ulp and logf at 2 ulp (HIP math API, single precision): 1 ulp <= 2 units of the result, so
    expf costs EXPF = 2 units relative and logf LOGF = 4 units of |log|;
  * an absolute error d in an exponent is a relative error d of expf's result (e^d - 1 = d to first order), an
    absolute error d in logf's argument x is d / x in its result;
  * a result below the smallest normal number (2^-126) is rounded to a multiple of 2^-149: magnitudes that a tolerance
    is relative to are floored at TINY = 2^-126.
Terms of second order in 2^-24 are left out (they are below 1e-5 of the first-order bound for every case used).

Case generators (ppo_discrete_case, ppo_continuous_case, huber_case) live here too; the properties they promise are
asserted by tests/test_head_loss_ref.py.
"""
import numpy as np

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24
EXPF, LOGF = 2.0, 4.0                               # units: expf 1 ulp, logf 2 ulp (see above)
TINY = 2.0 ** -126
EPS32 = float(np.finfo(np.float32).eps)             # rl_coach/utils.py:38
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
MAX_BLOCK = 1024                                    # kMaxBlock of csrc/losses_body.hpp


def _f64(x):
    return np.asarray(x, dtype=F32).astype(F64)


def block_for(batch):
    """threads of the single workgroup that csrc/losses.hip launches for `batch` rows"""
    t = 64
    while t < batch and t < MAX_BLOCK:
        t <<= 1
    return t


def sum_depth(batch):
    """fp32 additions on the longest path of the workgroup sum over the batch: a thread adds its ceil(batch / threads)
    rows in sequence (the first addition, to 0, is exact), then log2(threads) levels of the tree."""
    nt = block_for(batch)
    return (-(-batch // nt) - 1) + int(np.log2(nt))


# ------------------------------------------------------------------------------------------------ softmax
def softmax(logits):
    """tf.nn.softmax (ppo_head.py:110): p_j = exp(z_j - max) / sum_k exp(z_k - max)   -> (p [B, n], units [B, n]).
    Counted, with d_j = z_j - max (one rounding: |d_j| units absolute, which expf turns into |d_j| relative):
      e_j = expf(d_j)          |d_j| + EXPF                                       relative
      s = sum_k e_k            sum_k p_k (|d_k| + EXPF) + (n - 1)                 relative (all terms positive)
      p_j = e_j / s            the two above + 1
    units_j = max(p_j, TINY) * (|d_j| + sum_k p_k |d_k| + 2 EXPF + n).  An entry with p_j = 0 (d_j = -inf, or exp
    underflowed) contributes nothing to s."""
    z = _f64(logits)
    with np.errstate(all="ignore"):
        d = z - z.max(axis=1, keepdims=True)
        e = np.exp(d)
        p = e / e.sum(axis=1, keepdims=True)
        ad = np.where(p > 0, np.abs(d), 0.0)
    n = z.shape[1]
    units = np.maximum(p, TINY) * (ad + (p * ad).sum(axis=1, keepdims=True) + 2 * EXPF + n)
    return p, units


# ------------------------------------------------------------------------------------------------ regression heads
def regression_loss(out, target, weights=None, kind="mse", loss_weight=1.0, grad_scale=1.0):
    """Head.set_loss (head.py:172-177): loss = mean_b(loss_weight * w_b * sum_j l(target, out)), l = (t - o)^2 or huber
    with delta 1 (0.5 e^2 for |e| <= 1, |e| - 0.5 beyond), and grad = grad_scale * d loss / d out.
    -> dict(loss, loss_units, grad [B, D], grad_units [B, D]).
    Counted (e = o - t carries 1 unit relative):
      l        mse e * e: 2 + 1 = 3.  huber inside: (0.5 e) * e, 3; outside: |e| - 0.5 carries |e| + l <= 4 l units
               (l >= 0.5, |e| <= 3 l).  Both branches agree at |e| = 1 in value and slope, so an e that rounds across
               the boundary changes l only in second order.                                            <= 4 relative
      row      sum of D terms l >= 0: 4 + (D - 1)
      w        loss_weight * w_b: 1;  w * row: 1;  the batch sum: sum_depth(B);  / B: 1
    loss_units = (D + 6 + sum_depth(B)) * mean_b |w_b| row_b.
      grad     grad_scale * w: 1 + 1 (w);  * g: 1 + 1 (g = 2 e or clip(e, -1, 1));  / B: 1     grad_units = 5 |grad|."""
    o, t = _f64(out), _f64(target)
    B, D = o.shape
    w = F64(F32(loss_weight)) * (np.ones(B) if weights is None else _f64(weights))
    e = o - t
    a = np.abs(e)
    if kind == "mse":
        l, g = e * e, 2.0 * e
    else:
        l, g = np.where(a <= 1.0, 0.5 * e * e, a - 0.5), np.clip(e, -1.0, 1.0)
    row = l.sum(axis=1)
    loss = np.mean(w * row)
    grad = F64(F32(grad_scale)) * w[:, None] * g / B
    return dict(loss=loss, loss_units=(D + 6 + sum_depth(B)) * np.mean(np.abs(w) * row),
                grad=grad, grad_units=5.0 * np.abs(grad))


# ------------------------------------------------------------------------------------------------ discrete PPO head
def _clip_band(clip_eps, clip_scale):
    """1 -+ clip_eps * clip_scale (ppo_head.py:82-83) from the fp32 scalars"""
    ce = F64(F32(clip_eps)) * (1.0 if clip_scale is None else F64(F32(clip_scale)))
    return 1.0 - ce, 1.0 + ce, ce


def _surrogate(ratio, ratio_units, adv, lo, hi, ce):
    """the clipped surrogate of one row and its routing (ppo_head.py:84-87).  tf.minimum gives the gradient to
    ratio * adv where it is <= clipped * adv, else to the clipped branch, whose clip_by_value passes it inside [lo, hi].
      clipped      the ratio's units inside the band; on a bound: clip_eps (its product with clip_scale) + hi (1 -+ it)
      s1, s2       the factor's units * |adv| + 1 * |s|;  min(s1, s2) is perturbed by no more than the larger of the two"""
    clipped = np.clip(ratio, lo, hi)
    inside = (ratio >= lo) & (ratio <= hi)
    clipped_units = np.where(inside, ratio_units, ce + hi)
    s1, s2 = ratio * adv, clipped * adv
    sur = np.minimum(s1, s2)
    sur_units = np.maximum(np.abs(adv) * ratio_units + np.abs(s1), np.abs(adv) * clipped_units + np.abs(s2))
    passes = (s1 <= s2) | inside
    return clipped, clipped_units, sur, sur_units, passes


def _batch_mean(x, x_units, B, depth):
    """sum over the rows (depth additions), * (1 / B): 1 for the reciprocal, 1 for the product"""
    return x.sum() / B, (x_units.sum() + (depth + 2) * np.abs(x).sum()) / B


def ppo_discrete_loss(logits, actions, advantages, old_probs, clip_eps, beta, clip_scale=None, grad_scale=1.0):
    """PPOHead with a discrete action space (ppo_head.py:60-116) from the policy_fc logits z [B, n], the old policy's
    probabilities po [B, n] (Categorical(probs=po) renormalises them), actions [B], advantages [B].  A row whose action
    lies outside [0, n) is rejected: it adds nothing to the three batch sums, which are still divided by B.
    -> dict of value / value_units pairs: ratio, clipped [B]; dlogits [B, n]; scalars [4] = surrogate, mean entropy,
       mean KL(old || new), total = surrogate - beta * entropy; plus valid, passes [B] (bool) and lo, hi.
    Counted per row, in units; d_j = z_j - max, sm = softmax(z), D = sum_k sm_k |d_k|:
      se = sum expf(d_j)           D + EXPF + (n - 1)                                  relative
      lse = max + logf(se)         A_lse = D + EXPF + n - 1 + LOGF |log se| + |lse|    absolute
      so = sum po_j                n - 1 relative;  lso = logf(so): A_lso = n - 1 + LOGF |lso|
      lp_j = z_j - lse             A_lp_j = A_lse + |lp_j|;        p_j = expf(lp_j): A_lp_j + EXPF relative
      lpo_j = logf(po_j) - lso     A_lpo_j = LOGF |log po_j| + A_lso + |lpo_j|
      x = lp_a - lpo_a             A_x = A_lp_a + A_lpo_a + |x|;   ratio = expf(x): A_x + EXPF relative
      entropy = -sum p_j lp_j      sum_j [p_j |lp_j| (A_lp_j + EXPF + 1) + p_j A_lp_j] + (n - 1) sum_j |p_j lp_j|
      kl = sum (po_j / so) (lpo_j - lp_j), q_j = po_j / so (n relative), f_j = lpo_j - lp_j (A_lpo_j + A_lp_j + |f_j|):
                                   sum_j [q_j (A_lpo_j + A_lp_j + |f_j|) + (n + 1) |q_j f_j|] + (n - 1) sum_j |q_j f_j|
      scalars                      _batch_mean of the rows;  total: surrogate's + |beta| (entropy's + |entropy|) + |total|
      g_logp = -adv ratio / B      (|adv| ratio_units + 2 |adv ratio|) / B   where the gradient passes, else exactly 0
      t1_j = g_logp ([j = a] - p_j)      g_logp_units |[j = a] - p_j| + |g_logp| (p_j (A_lp_j + EXPF) + |[j = a] - p_j|) + |t1_j|
      t2_j = (beta / B) p_j (lp_j + H)   |gb p_j| (A_lp_j + H_units + |lp_j + H|) + |t2_j| (1 + A_lp_j + EXPF + 2)
      dlogits_j = grad_scale (t1_j + t2_j)    |grad_scale| (t1's + t2's + 2 |t1_j + t2_j|)"""
    z, po = _f64(logits), _f64(old_probs)
    adv = _f64(advantages)
    a = np.asarray(actions).astype(np.int64)
    B, n = z.shape
    valid = (a >= 0) & (a < n)
    ac = np.where(valid, a, 0)
    rows = np.arange(B)
    lo, hi, ce = _clip_band(clip_eps, clip_scale)
    bt, gs = F64(F32(beta)), F64(F32(grad_scale))
    with np.errstate(all="ignore"):
        mx = z.max(axis=1, keepdims=True)
        d = z - mx
        e = np.exp(d)
        se = e.sum(axis=1, keepdims=True)
        sm = e / se
        Dw = (sm * np.abs(d)).sum(axis=1, keepdims=True)
        lse = mx + np.log(se)
        A_lse = Dw + EXPF + n - 1 + LOGF * np.abs(np.log(se)) + np.abs(lse)
        so = po.sum(axis=1, keepdims=True)
        lso = np.log(so)
        A_lso = n - 1 + LOGF * np.abs(lso)
        lp = z - lse
        A_lp = A_lse + np.abs(lp)
        p = np.exp(lp)
        lpo = np.log(po) - lso
        A_lpo = LOGF * np.abs(np.log(po)) + A_lso + np.abs(lpo)
    x = lp[rows, ac] - lpo[rows, ac]
    A_x = A_lp[rows, ac] + A_lpo[rows, ac] + np.abs(x)
    ratio = np.exp(x)
    ratio_units = ratio * (A_x + EXPF)
    clipped, clipped_units, sur, sur_units, passes = _surrogate(ratio, ratio_units, adv, lo, hi, ce)
    pl = p * lp
    ent = -pl.sum(axis=1)
    ent_units = (np.abs(pl) * (A_lp + EXPF + 1) + p * A_lp).sum(axis=1) + (n - 1) * np.abs(pl).sum(axis=1)
    q = po / so
    f = lpo - lp
    qf = q * f
    kl = qf.sum(axis=1)
    kl_units = (q * (A_lpo + A_lp + np.abs(f)) + (n + 1) * np.abs(qf)).sum(axis=1) + (n - 1) * np.abs(qf).sum(axis=1)
    depth = sum_depth(B)
    v = valid.astype(F64)
    s_sur, u_sur = _batch_mean(sur * v, sur_units * v, B, depth)
    s_ent, u_ent = _batch_mean(ent * v, ent_units * v, B, depth)
    s_kl, u_kl = _batch_mean(kl * v, kl_units * v, B, depth)
    total = -s_sur - bt * s_ent
    u_total = u_sur + abs(bt) * (u_ent + abs(s_ent)) + abs(total)
    g_logp = np.where(passes, -adv * ratio, 0.0) / B
    g_logp_units = np.where(passes, (np.abs(adv) * ratio_units + 2 * np.abs(adv * ratio)) / B, 0.0)
    onehot = (np.arange(n)[None, :] == ac[:, None]).astype(F64)
    w1 = onehot - p
    t1 = g_logp[:, None] * w1
    t1_units = g_logp_units[:, None] * np.abs(w1) + np.abs(g_logp)[:, None] * (p * (A_lp + EXPF) + np.abs(w1)) + np.abs(t1)
    gb = bt / B
    h = lp + ent[:, None]
    t2 = gb * p * h
    t2_units = np.abs(gb * p) * (A_lp + ent_units[:, None] + np.abs(h)) + np.abs(t2) * (3 + A_lp + EXPF)
    dl = gs * (t1 + t2)
    dl_units = abs(gs) * (t1_units + t2_units + 2 * np.abs(t1 + t2))
    return dict(ratio=ratio, ratio_units=ratio_units, clipped=clipped, clipped_units=clipped_units,
                dlogits=dl, dlogits_units=dl_units,
                scalars=np.array([-s_sur, s_ent, s_kl, total]), scalars_units=np.array([u_sur, u_ent, u_kl, u_total]),
                valid=valid, passes=passes, lo=lo, hi=hi, entropy_rows=ent, kl_rows=kl, surrogate_rows=sur)


# ------------------------------------------------------------------------------------------------ continuous PPO head
def ppo_continuous_loss(mean, log_std, actions, advantages, old_mean, old_std, clip_eps, beta, clip_scale=None,
                        grad_scale=1.0):
    """PPOHead with a box action space (ppo_head.py:118-144 + :60-98): the policy is MultivariateNormalDiag(mean [B, A],
    exp(log_std [A]) + eps), the old policy MultivariateNormalDiag(old_mean, old_std + eps), eps = finfo(float32).eps.
    -> dict of value / value_units pairs: ratio, clipped [B]; dmean [B, A]; dlog_std [A]; scalars [4] (the entropy is the
       same for every row); plus passes, lo, hi.
    Counted, per dimension, c = 0.5 log(2 pi) (the kernel's fp32 constant: 1 unit of c):
      sd = expf(ls) + eps          EXPF + 1 = 3 relative;   sdo = old_std + eps: 1
      z = (x - mu) / sd            1 + 1 + 3 = 5;   h = 0.5 z^2: 11;   zo = (x - mo) / sdo: 3;   ho = 0.5 zo^2: 7
      log sd                       3 + LOGF |log sd| absolute;   log sdo: 1 + LOGF |log sdo|
      term = -h - log sd - c       11 h + 3 + LOGF |log sd| + |h + log sd| + c + |term|;  logp = sum of A terms, added to
                                   0 in sequence: sum of the terms' units + (A - 1) sum |term|;  the old policy alike
      ratio = expf(logp - logp_old)      logp's + logp_old's + |logp - logp_old| + EXPF, relative
      kl term = logf(sd / sdo) + (sdo^2 + dm^2) / (2 sd^2) - 0.5,  dm = mo - mu:
                                   5 + LOGF |log(sd / sdo)|  +  (4 + 7 + 1) quotient  +  |log + quotient|  +  |term|;
                                   the row sum adds A sum |term|
      entropy = sum_a (0.5 + c) + log sd     per term 1.42 + c + 3 + LOGF |log sd| + |term|; the sum A sum |term|
      g_logp = -adv ratio * (grad_scale / B)      ratio's relative + 3
      dmean = g_logp (x - mu) / (sd sd)           g_logp's + 1 + 1 + 7 + 1 = ratio's relative + 13
      part_b = g_logp (d^2 / sd^3 - 1 / sd) e     |g_logp e| (15 d^2 / sd^3 + 4 / sd + |difference|) + |part| (g_logp's + 4)
      dlog_std = sum_b part_b - grad_scale beta e / sd      the parts' + log2(threads) sum |part_b| + 8 |entropy term|
                                                            + |dlog_std|"""
    mu, x, mo = _f64(mean), _f64(actions), _f64(old_mean)
    ls, adv = _f64(log_std).reshape(-1), _f64(advantages)
    B, A = mu.shape
    lo, hi, ce = _clip_band(clip_eps, clip_scale)
    bt, gs = F64(F32(beta)), F64(F32(grad_scale))
    c = HALF_LOG_2PI
    e = np.exp(ls)
    sd = e + EPS32
    sdo = _f64(old_std) + EPS32
    z, zo = (x - mu) / sd, (x - mo) / sdo
    h, ho = 0.5 * z * z, 0.5 * zo * zo
    lsd, lsdo = np.log(sd), np.log(sdo)
    term, termo = -h - lsd - c, -ho - lsdo - c
    term_units = 11 * h + 3 + LOGF * np.abs(lsd) + np.abs(h + lsd) + c + np.abs(term)
    termo_units = 7 * ho + 1 + LOGF * np.abs(lsdo) + np.abs(ho + lsdo) + c + np.abs(termo)
    logp, logpo = term.sum(axis=1), termo.sum(axis=1)
    logp_units = term_units.sum(axis=1) + (A - 1) * np.abs(term).sum(axis=1)
    logpo_units = termo_units.sum(axis=1) + (A - 1) * np.abs(termo).sum(axis=1)
    dx = logp - logpo
    ratio = np.exp(dx)
    ratio_rel = logp_units + logpo_units + np.abs(dx) + EXPF
    ratio_units = ratio * ratio_rel
    clipped, clipped_units, sur, sur_units, passes = _surrogate(ratio, ratio_units, adv, lo, hi, ce)
    dm = mo - mu
    lg, quo = np.log(sd / sdo), (sdo * sdo + dm * dm) / (2.0 * sd * sd)
    klt = lg + quo - 0.5
    klt_units = 5 + LOGF * np.abs(lg) + 12 * quo + np.abs(lg + quo) + np.abs(klt)
    kl = klt.sum(axis=1)
    kl_units = klt_units.sum(axis=1) + A * np.abs(klt).sum(axis=1)
    et = 0.5 + c + lsd
    ent = et.sum()
    ent_units = (1.42 + c + 3 + LOGF * np.abs(lsd) + np.abs(et)).sum() + A * np.abs(et).sum()
    depth = int(np.log2(block_for(B)))
    s_sur, u_sur = _batch_mean(sur, sur_units, B, depth)
    s_kl, u_kl = _batch_mean(kl, kl_units, B, depth)
    total = -s_sur - bt * ent
    u_total = u_sur + abs(bt) * (ent_units + abs(ent)) + abs(total)
    g_logp = np.where(passes, -adv * ratio, 0.0) * gs / B
    g_rel = ratio_rel + 3
    d = x - mu
    dmean = g_logp[:, None] * d / (sd * sd)
    dmean_units = np.abs(dmean) * (ratio_rel + 13)[:, None]
    t3, t1 = d * d / sd ** 3, 1.0 / sd
    part = g_logp[:, None] * (t3 - t1) * e
    part_units = np.abs(g_logp[:, None] * e) * (15 * t3 + 4 * t1 + np.abs(t3 - t1)) + np.abs(part) * (g_rel + 4)[:, None]
    et2 = gs * bt * e / sd
    dls = part.sum(axis=0) - et2
    dls_units = part_units.sum(axis=0) + depth * np.abs(part).sum(axis=0) + 8 * np.abs(et2) + np.abs(dls)
    return dict(ratio=ratio, ratio_units=ratio_units, clipped=clipped, clipped_units=clipped_units,
                dmean=dmean, dmean_units=dmean_units, dlog_std=dls, dlog_std_units=dls_units,
                scalars=np.array([-s_sur, ent, s_kl, total]), scalars_units=np.array([u_sur, ent_units, u_kl, u_total]),
                passes=passes, lo=lo, hi=hi)


# ------------------------------------------------------------------------------------------------ actor-critic critics
def ac_critic_losses(q_next1, q_next2, rewards, game_overs, discount, q, loss_weight=1.0, clip=None,
                     use_non_zero_discount_for_terminal_states=False, td_targets=None):
    """The critic update of DDPG / TD3 / SAC (ddpg_agent.py:156-164, td3_agent.py:168-180): q_next = min of the two target
    critics (q_next2 None: q_next1), y = r + (1 - done) * discount * q_next in float64 (with
    use_non_zero_discount_for_terminal_states: r + float64(fp32(discount) * q_next), the reference's fp32 product, done
    ignored), optionally clipped to clip = (low, high), cast to fp32; per stream t the
    head's loss_weight * mean((q_t - y)^2) and its gradient; total = the sum of the stream losses.
    td_targets: evaluate the losses at these fp32 targets (the device's own) instead of at float32(y).
    -> dict(q_min [B] exact (a selection), y [B] float64 before the cast, y_units = |y| (one rounding, the cast),
            loss [T], loss_units, dq [T, B], dq_units, total, total_units).
    Counted: every stream is regression_loss with D = 1; total adds T losses in sequence: their units + T sum |loss_t|."""
    q1 = np.asarray(q_next1, dtype=F32)
    qn = q1 if q_next2 is None else np.where(q1 <= np.asarray(q_next2, dtype=F32), q1, np.asarray(q_next2, dtype=F32))
    r, done = _f64(rewards), np.asarray(game_overs).astype(bool)
    if use_non_zero_discount_for_terminal_states:
        # `discount * q_st_plus_1` (ddpg_agent.py:157): a python float times the fp32 network output is an fp32 product
        y = r + (F32(discount) * qn).astype(F64)
    else:
        y = r + (1.0 - done.astype(F64)) * F64(discount) * qn.astype(F64)
    if clip is not None:
        y = np.minimum(np.maximum(y, F64(clip[0])), F64(clip[1]))
    y32 = y.astype(F32) if td_targets is None else np.asarray(td_targets, dtype=F32)
    q = np.asarray(q, dtype=F32)
    T = q.shape[0]
    parts = [regression_loss(q[t][:, None], y32[:, None], None, "mse", loss_weight, 1.0) for t in range(T)]
    loss = np.array([p["loss"] for p in parts])
    loss_units = np.array([p["loss_units"] for p in parts])
    return dict(q_min=qn, y=y, y_units=np.abs(y), loss=loss, loss_units=loss_units,
                dq=np.stack([p["grad"][:, 0] for p in parts]), dq_units=np.stack([p["grad_units"][:, 0] for p in parts]),
                total=loss.sum(), total_units=loss_units.sum() + T * np.abs(loss).sum())


# ------------------------------------------------------------------------------------------------ case generators
CLIP_MARGIN = 1e-3                                   # every ratio is at least this far, relatively, from 1 -+ clip_eps
QUADRANTS = ("hi_pos", "hi_neg", "lo_pos", "lo_neg", "in_pos", "in_neg")
MIN_QUADRANT_ROWS = 6                                # a batch with fewer rows cannot hold one row of every kind


def quadrant_of(ratio, adv, lo, hi):
    """the name in QUADRANTS of every row"""
    band = np.where(ratio > hi, "hi", np.where(ratio < lo, "lo", "in"))
    return np.char.add(np.char.add(band, "_"), np.where(adv > 0, "pos", "neg"))


def _far_from_bounds(ratio, lo, hi):
    return (np.abs(ratio - lo) >= CLIP_MARGIN * lo) & (np.abs(ratio - hi) >= CLIP_MARGIN * hi)


def _wanted(B, rng):
    """kinds [B]: the six kinds of QUADRANTS in turn, from a random start"""
    return np.array(QUADRANTS)[(np.arange(B) + rng.randint(6)) % 6]


def _advantages(kinds, rng):
    sign = np.where(np.char.endswith(kinds, "pos"), 1.0, -1.0)
    return (sign * rng.uniform(0.1, 2.0, kinds.size)).astype(F32)


def _resample(B, kinds, draw, evaluate, can_leave_band, lo, hi):
    """rows are drawn again until each one's float64 ratio lies in the band its kind names, CLIP_MARGIN clear of both
    bounds and inside [0.05, 20] -- nothing is left to be skipped when a kernel is compared"""
    rows = draw(np.arange(B))
    todo = np.arange(B)
    for _ in range(400):
        ratio = evaluate(rows, todo)
        band = np.where(ratio > hi, "hi", np.where(ratio < lo, "lo", "in"))
        want = np.array([k[:2] for k in kinds[todo]]) if can_leave_band else np.full(todo.size, "in")
        ok = (band == want) & _far_from_bounds(ratio, lo, hi) & (ratio > 0.05) & (ratio < 20)
        todo = todo[~ok]
        if todo.size == 0:
            return rows
        new = draw(todo)
        for k in rows:
            rows[k][todo] = new[k]
    raise AssertionError("no admissible draw for %d rows" % todo.size)


def ppo_discrete_case(rng, B, n, clip_eps=0.2, ld=None, ld_old=None):
    """-> dict(logits [B, ld], old_probs [B, ld_old] fp32 with NaN beyond column n, actions int32, advantages fp32,
    kinds [B]).  Logits are N(0, 1); the old probabilities are a softmax of the logits plus noise of scale 0.2, 1 or 2,
    every third row times a factor in [0.5, 3] (un-normalised), all strictly positive.  Promised: every float64 ratio
    is CLIP_MARGIN away from 1 -+ clip_eps; for B >= MIN_QUADRANT_ROWS and n >= 2 each kind of QUADRANTS holds at least
    max(1, B // 16) rows (with one action the ratio is 1 in every row: all rows lie inside the band); |adv| >= 0.1."""
    ld, ld_old = ld or n, ld_old or n
    kinds = _wanted(B, rng)
    adv = _advantages(kinds, rng)
    lo, hi, _ = _clip_band(clip_eps, None)

    def draw(idx):
        m = idx.size
        z = rng.randn(m, n).astype(F32)
        noise = rng.choice([0.2, 1.0, 2.0], size=(m, 1)) * rng.randn(m, n)
        o = np.exp(z.astype(F64) + noise)
        o = o / o.sum(axis=1, keepdims=True) * np.where(idx % 3 == 0, rng.uniform(0.5, 3.0, m), 1.0)[:, None]
        return dict(z=z, po=np.maximum(o, 1e-30).astype(F32), a=rng.randint(0, n, m).astype(np.int32))

    def evaluate(rows, idx):
        return ppo_discrete_loss(rows["z"][idx], rows["a"][idx], adv[idx], rows["po"][idx], clip_eps, 0.0)["ratio"]

    rows = _resample(B, kinds, draw, evaluate, n >= 2, lo, hi)
    logits, old = np.full((B, ld), np.nan, dtype=F32), np.full((B, ld_old), np.nan, dtype=F32)
    logits[:, :n], old[:, :n] = rows["z"], rows["po"]
    return dict(logits=logits, old_probs=old, actions=rows["a"], advantages=adv, kinds=kinds)


def ppo_continuous_case(rng, B, A, clip_eps=0.2, ld=None, ld_old=None):
    """-> dict(mean [B, ld], old_mean / old_std [B, ld_old] fp32 with NaN beyond column A, log_std [A], actions [B, A],
    advantages, kinds).  log_std U(-1, 0.5), actions = mean + sd N(0, 1), old_mean = mean + s sd N(0, 1) with s one of
    0.1, 0.5, 1 per row, old_std = sd exp(0.1 N(0, 1)) > 0.  Promises as ppo_discrete_case (every A can leave the band)."""
    ld, ld_old = ld or A, ld_old or A
    kinds = _wanted(B, rng)
    adv = _advantages(kinds, rng)
    lo, hi, _ = _clip_band(clip_eps, None)
    ls = rng.uniform(-1.0, 0.5, A).astype(F32)
    sd = np.exp(ls.astype(F64))

    def draw(idx):
        m = idx.size
        mu = (0.5 * rng.randn(m, A)).astype(F32)
        x = (mu + sd * rng.randn(m, A)).astype(F32)
        mo = (mu + rng.choice([0.1, 0.5, 1.0], size=(m, 1)) * sd * rng.randn(m, A)).astype(F32)
        so = (sd * np.exp(0.1 * rng.randn(m, A))).astype(F32)
        return dict(mu=mu, x=x, mo=mo, so=so)

    def evaluate(rows, idx):
        return ppo_continuous_loss(rows["mu"][idx], ls, rows["x"][idx], adv[idx], rows["mo"][idx], rows["so"][idx],
                                   clip_eps, 0.0)["ratio"]

    rows = _resample(B, kinds, draw, evaluate, True, lo, hi)
    mean = np.full((B, ld), np.nan, dtype=F32)
    om, os_ = np.full((B, ld_old), np.nan, dtype=F32), np.full((B, ld_old), np.nan, dtype=F32)
    mean[:, :A], om[:, :A], os_[:, :A] = rows["mu"], rows["mo"], rows["so"]
    return dict(mean=mean, log_std=ls, actions=rows["x"], advantages=adv, old_mean=om, old_std=os_, kinds=kinds)


HUBER_EDGES = tuple(F32(s) * v for s in (1, -1) for v in
                    (F32(1), np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2)))) + (F32(0),)


def huber_case(rng, B, D, ld_out=None, ld_target=None):
    """-> (out [B, ld_out], target [B, ld_target], weights [B]) fp32 with NaN beyond column D.  Errors are N(0, 2) on
    N(0, 1) targets, except that the seven values of HUBER_EDGES (+-1, one fp32 step inside, one outside, 0) are planted
    on a zero target -- so that out - target IS the planted value in fp32 -- one after the other from element 0 on, as far
    as B * D reaches (all seven when B * D >= 7)."""
    ld_out, ld_target = ld_out or D, ld_target or D
    t = rng.randn(B, D).astype(F32)
    o = (t + 2.0 * rng.randn(B, D)).astype(F32)
    k = min(B * D, len(HUBER_EDGES))
    t.reshape(-1)[:k] = 0
    o.reshape(-1)[:k] = HUBER_EDGES[:k]
    out, target = np.full((B, ld_out), np.nan, dtype=F32), np.full((B, ld_target), np.nan, dtype=F32)
    out[:, :D], target[:, :D] = o, t
    return out, target, rng.uniform(0.2, 2.0, B).astype(F32)
