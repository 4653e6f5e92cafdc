"""numpy float64 restatement of the small kernels that carry data between network passes: the twin of the glue entry
points of csrc/actor_critic.hip, csrc/targets.hip (dueling merge), csrc/optim.hip (global norm, clip) and csrc/gemm.hip
(activation derivative).  Written from the reference's formulas (paths under rl_coach/architectures/tensorflow_components/):
heads/sac_head.py:58-97, heads/sac_q_head.py:63-88, heads/dueling_q_head.py:33-48, heads/ppo_head.py:139,
architecture.py:194-200,238-240 and TensorFlow's documented clip_by_value / minimum / clip_by_global_norm rules -- NOT
from oracle/ac_nets.py, which this module never imports: tests/test_glue_ref.py compares the two.

Every function takes the fp32 device inputs and evaluates in float64, so a result is the exact value up to ~1e-16; the
*_f32 variants restate a kernel's own fp32 evaluation order where the kernel owes bit equality.

  copy_2d(src, scale)                       -> scale * src (exact in float64: a 24 x 24 bit product)
  axpby(a, x, b, y)                         -> (a x + b y, |a x| + |b y|)
  exp_rows(log_std, batch)                  -> tile(exp(log_std))
  min_pair(q1, q2, grad_scale)              -> (min, g1, g2): a tie (q1 == q2, +-0.0 included) goes to q1; a NaN is kept
  sac_min_targets(q1, q2, logp, grad_scale) -> (min, min - logp, g1, g2)
  dueling_combine(v, adv) / _backward(dq)   -> float64;  dueling_combine_f32 / _backward_f32: fp32, sums in index order
  global_norm(x)                            -> sqrt(sum x^2)
  clip_by_global_norm(g, norm, clip)        -> float64;  clip_by_global_norm_f32: the kernel's fp32 expression
  act_backward(dy, y, kind)                 -> dy * act'(y), act' written through the activation's output
  sac_head_forward(...) / sac_head_backward(...) -> dicts, see there
  sac_head_case(rng, B, A, ld)              -> inputs that hold every branch of the head (see there)
"""
import numpy as np

F32 = np.float32
F64 = np.float64
EPS32 = float(np.finfo(np.float32).eps)             # rl_coach/utils.py:38
LOG_SIG_CAP_MIN, LOG_SIG_CAP_MAX = -20.0, 2.0       # sac_head.py:26-27
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
U24 = 2.0 ** -24                                    # half an ulp of 1.0f: the relative error of one fp32 rounding


def _f64(x):
    return np.asarray(x, dtype=F32).astype(F64)


def copy_2d(src, scale):
    return F64(F32(scale)) * _f64(src)


def axpby(a, x, b, y=None):
    ax = F64(F32(a)) * _f64(x)
    by = np.zeros_like(ax) if y is None else F64(F32(b)) * _f64(y)
    return ax + by, np.abs(ax) + np.abs(by)


def exp_rows(log_std, batch):
    return np.tile(np.exp(_f64(log_std)), (batch, 1))


def min_pair(q1, q2, grad_scale):
    """tf.minimum(q1, q2) and the gradient of its sum: TensorFlow gives the gradient of minimum(x, y) to x where
    x <= y.  The value on a tie is q1's (which matters only for the sign of a zero).  A NaN of either side is the minimum
    (np.minimum / tf.minimum keep it): q1's where q1 is one, q2's otherwise, and value and gradient go to the same side."""
    q1, q2 = np.asarray(q1, dtype=F32), np.asarray(q2, dtype=F32)
    first = (q1 <= q2) | np.isnan(q1)
    gs = F32(grad_scale)
    return np.where(first, q1, q2), np.where(first, gs, F32(0)), np.where(first, F32(0), gs)


def sac_min_targets(q1, q2, logp, grad_scale):
    m, g1, g2 = min_pair(q1, q2, grad_scale)
    return m, m.astype(F64) - _f64(logp), g1, g2          # soft_actor_critic_agent.py:244


def dueling_combine(v, adv):
    v, adv = _f64(v), _f64(adv)
    return v[:, None] + (adv - adv.mean(axis=1, keepdims=True))        # dueling_q_head.py:47-48


def dueling_combine_backward(dq):
    dq = _f64(dq)
    return dq.sum(axis=1), dq - dq.mean(axis=1, keepdims=True)


def _rowsum_f32(x):
    s = np.zeros(x.shape[0], dtype=F32)
    for i in range(x.shape[1]):
        s = s + x[:, i]
    return s


def dueling_combine_f32(v, adv):
    v, adv = np.asarray(v, dtype=F32), np.asarray(adv, dtype=F32)
    mean = _rowsum_f32(adv) / F32(adv.shape[1])
    return v[:, None] + (adv - mean[:, None])


def dueling_combine_backward_f32(dq):
    dq = np.asarray(dq, dtype=F32)
    s = _rowsum_f32(dq)
    return s, dq - (s / F32(dq.shape[1]))[:, None]


def global_norm(x):
    return float(np.sqrt(np.sum(_f64(x) ** 2)))


def _tf_minimum(x, y):
    """TensorFlow's minimum kernel is (y < x) ? y : x: a NaN in x comes through."""
    return y if y < x else x


def clip_by_global_norm(g, norm, clip):
    """tf.clip_by_global_norm: t * clip_norm * minimum(1 / global_norm, 1 / clip_norm).  A NaN norm gives NaN
    everywhere; an infinite norm gives a scale of 0 (0 for finite entries, NaN for infinite ones)."""
    with np.errstate(all="ignore"):
        norm, clip = F64(F32(norm)), F64(F32(clip))
        return _f64(g) * (clip * _tf_minimum(1.0 / norm, 1.0 / clip))


def clip_by_global_norm_f32(g, norm, clip):
    with np.errstate(all="ignore"):
        norm, clip = F32(norm), F32(clip)
        scale = clip * _tf_minimum(F32(1) / norm, F32(1) / clip)
        return np.asarray(g, dtype=F32) * scale


def act_backward(dy, y, kind):
    dy, y = _f64(dy), _f64(y)
    if kind == "relu":
        return dy * (y > 0)
    if kind == "tanh":
        return dy * (1.0 - y * y)
    return dy


# ------------------------------------------------------------------------------------------------ SACPolicyHead
def _head_common(mu_logsig, normals, A, raw=None):
    x = _f64(mu_logsig)
    mu, ls_raw = x[:, :A], x[:, A:2 * A]
    ls = np.minimum(np.maximum(ls_raw, LOG_SIG_CAP_MIN), LOG_SIG_CAP_MAX)       # tf.clip_by_value :65-66
    sd = np.exp(ls)
    e = np.asarray(normals, dtype=F64).astype(F32).astype(F64)                   # the draw is an fp32 tensor
    raw_exact = mu + sd * e                                                      # MultivariateNormalDiag.sample() :80
    raw = raw_exact if raw is None else _f64(raw)
    t = np.tanh(raw)
    # 1 - t^2 without cancellation (float64 tanh is exactly 1 beyond |raw| = 19): sech^2 = 4 e^-2|r| / (1 + e^-2|r|)^2
    q = np.exp(-2.0 * np.abs(raw))
    u = 4.0 * q / (1.0 + q) ** 2
    return dict(mu=mu, ls_raw=ls_raw, ls=ls, sd=sd, e=e, raw_exact=raw_exact, raw=raw, t=t, u=u, cond=1.0 / (u + EPS32),
                below=ls_raw < LOG_SIG_CAP_MIN, above=ls_raw > LOG_SIG_CAP_MAX,
                on_bound=(ls_raw == LOG_SIG_CAP_MIN) | (ls_raw == LOG_SIG_CAP_MAX))


def sac_head_forward(mu_logsig, normals, A, raw=None):
    """SACPolicyHead outputs [0]..[4] for the dense output mu_logsig [B, >= 2A] (fp32) and the standard normal draws
    [B, A].  raw: evaluate the squashed actions and the log-probability at this fp32 raw_actions tensor instead of the
    exact sample -- sac_head.py:83,91 compute both FROM the sampled tensor, so that is the reference for a device that
    has already rounded its sample.

    -> mean, log_std, raw (the exact sample), act, logp [B], and what the tolerances need:
       cond = 1 / (1 - t^2 + eps) per element, below / above / on_bound: where log_std left, or sits on, [-20, 2],
       z = (raw - mu) / sd, raw_mag = |mu| + |sd e|,
       logp_t_unit [B] = sum_a (2|t| + 1) cond, logp_g_unit [B] = sum_a (z^2 / 2 + |ls| + 0.92)."""
    c = _head_common(mu_logsig, normals, A, raw)
    z = (c["raw"] - c["mu"]) / c["sd"]
    gauss = -0.5 * z * z - c["ls"] - HALF_LOG_2PI                                # log_prob :91
    corr = np.log(c["u"] + EPS32)                                                # _squash_correction :58
    return dict(mean=c["mu"], log_std=c["ls"], raw=c["raw_exact"], act=c["t"], logp=gauss.sum(axis=1) - corr.sum(axis=1),
                cond=c["cond"], below=c["below"], above=c["above"], on_bound=c["on_bound"], z=z,
                raw_mag=np.abs(c["mu"]) + np.abs(c["sd"] * c["e"]),
                logp_t_unit=((2 * np.abs(c["t"]) + 1) * c["cond"]).sum(axis=1),
                logp_g_unit=(0.5 * z * z + np.abs(c["ls"]) + 0.92).sum(axis=1))


def sac_head_backward(mu_logsig, normals, A, logp_weight=0.0, action_weights=None, action_weight_scale=1.0):
    """d / d mu_logsig of  logp_weight * mean_b(logp_b) + action_weight_scale * sum(action_weights * tanh(raw)), through
    the reparameterised sample raw = mu + exp(clip(log_std)) * e (tf.gradients of outputs [5] and [3]).  The Gaussian
    terms of logp cancel through the reparameterisation except -log_std; the squash correction leaves
    2 t (1 - t^2) / (1 - t^2 + eps) per unit of raw.  clip_by_value = minimum(maximum(x, lo), hi) passes the gradient
    where lo <= x <= hi, both ends included.

    -> d_mu, d_ls [B, A] and the masks of sac_head_forward, plus mu_unit / ls_unit: the first-order effect on d_mu /
       d_ls of fp32 roundings of relative size 2^-24 in every intermediate (see the derivation below)."""
    c = _head_common(mu_logsig, normals, A)
    B = c["mu"].shape[0]
    t, u, cond, sde = c["t"], c["u"], c["cond"], c["sd"] * c["e"]
    w = F64(F32(logp_weight)) / B
    aw = np.zeros_like(t) if action_weights is None else F64(F32(action_weight_scale)) * _f64(action_weights)
    g_raw = w * 2.0 * t * u * cond + aw * u
    inside = ~(c["below"] | c["above"])
    d_ls = np.where(inside, g_raw * sde - w, 0.0)
    # Error model, in units of 2^-24.  The device holds t with an error dt = |t| (tanhf, a few ulp) + (1 - t^2) d_raw
    # where d_raw = 2 (|mu| + |sd e|) is the rounding of the sample; 1 - t^2 then carries du = 2|t| dt + 1.  g_raw
    # depends on u = 1 - t^2 through  w 2t u / (u + eps)  (derivative w 2t eps cond^2)  and  aw u  (derivative aw), and
    # on t directly through the factor 2t (derivative w 2 u cond <= 2w); its own operations round |g_raw| and |w|.
    dt = np.abs(t) + u * 2.0 * (np.abs(c["mu"]) + np.abs(sde))
    du = 2.0 * np.abs(t) * dt + 1.0
    mu_unit = (np.abs(w) * 2.0 * np.abs(t) * EPS32 * cond ** 2 + np.abs(aw)) * du + np.abs(w) * 2.0 * u * cond * dt + \
        np.abs(g_raw) + np.abs(w)
    ls_unit = np.where(inside, mu_unit * np.abs(sde) + np.abs(g_raw * sde) + np.abs(w), 0.0)
    return dict(d_mu=g_raw, d_ls=d_ls, mu_unit=mu_unit, ls_unit=ls_unit, cond=cond, below=c["below"], above=c["above"],
                on_bound=c["on_bound"], raw=c["raw_exact"])


# Shares of the elements of sac_head_case() outside its plain rows, in twentieths.
_LS_KINDS = ["interior"] * 8 + ["below"] * 4 + ["above"] * 4 + ["lo_bound"] * 2 + ["hi_bound"] * 2
_RAW_KINDS = ["ordinary"] * 10 + ["near_sat"] * 5 + ["saturated"] * 5
CATEGORY_MIN_SHARE = 0.05


def sac_head_case(rng, B, A, ld=None, plain_rows=None):
    """-> (mu_logsig [B, ld] fp32, normals [B, A] float64, plain [B] bool).  Every element draws one log-std kind and,
    independently, one raw-action kind; mu is then solved so that the sample lands where its kind says:
      log_std   interior U(-6, 1.9) | below U(-45, -20.5) | above U(2.5, 30) | exactly -20 | exactly 2
      raw       ordinary |raw| <= 1.5 | near saturation |raw| in U(4.2, 8.8) | saturated |raw| in U(10.5, 20)
    The first B // 8 rows (`plain`) are interior and ordinary throughout, and narrower: log_std U(-3, -1.5), |raw| <= 1
    -- the rows on which a tolerance must stay tight.  Columns beyond 2A (ld > 2A) hold a large sentinel that no output may depend on."""
    ld = 2 * A if ld is None else ld
    n_plain = B // 8 if plain_rows is None else plain_rows
    plain = np.arange(B) < n_plain
    n = B * A
    ls_kind = np.array(_LS_KINDS)[rng.permutation(n) % 20].reshape(B, A)
    raw_kind = np.array(_RAW_KINDS)[rng.permutation(n) % 20].reshape(B, A)
    ls_kind[plain], raw_kind[plain] = "interior", "ordinary"
    ls = rng.uniform(-6.0, 1.9, (B, A))
    ls = np.where(plain[:, None], rng.uniform(-3.0, -1.5, (B, A)), ls)
    ls = np.where(ls_kind == "below", rng.uniform(-45.0, -20.5, (B, A)), ls)
    ls = np.where(ls_kind == "above", rng.uniform(2.5, 30.0, (B, A)), ls)
    ls = np.where(ls_kind == "lo_bound", LOG_SIG_CAP_MIN, ls)
    ls = np.where(ls_kind == "hi_bound", LOG_SIG_CAP_MAX, ls).astype(F32)
    normals = rng.standard_normal((B, A))
    target = rng.uniform(-1.5, 1.5, (B, A))
    target = np.where(plain[:, None], rng.uniform(-1.0, 1.0, (B, A)), target)
    sign = np.where(rng.rand(B, A) < 0.5, -1.0, 1.0)
    target = np.where(raw_kind == "near_sat", sign * rng.uniform(4.2, 8.8, (B, A)), target)
    target = np.where(raw_kind == "saturated", sign * rng.uniform(10.5, 20.0, (B, A)), target)
    sd = np.exp(np.clip(ls.astype(F64), LOG_SIG_CAP_MIN, LOG_SIG_CAP_MAX))
    mu = (target - sd * normals.astype(F32).astype(F64)).astype(F32)
    x = np.full((B, ld), 7e4, dtype=F32)
    x[:, :A], x[:, A:2 * A] = mu, ls
    return x, normals, plain


def sac_head_categories(fwd):
    """the shares (a)-(f) of the issue from a sac_head_forward() result: {name: fraction of the B*A elements}."""
    r = np.abs(fwd["raw"])
    lo = fwd["on_bound"] & (fwd["log_std"] == LOG_SIG_CAP_MIN)
    hi = fwd["on_bound"] & (fwd["log_std"] == LOG_SIG_CAP_MAX)
    masks = dict(interior=~(fwd["below"] | fwd["above"] | fwd["on_bound"]), below=fwd["below"], above=fwd["above"],
                 lo_bound=lo, hi_bound=hi, near_sat=(r >= 4) & (r <= 9), saturated=r > 10)
    return {k: float(m.mean()) for k, m in masks.items()}


def ulp_distance(got, ref64):
    """|got - ref| in units of the fp32 spacing at |ref| (ref64 is float64; 0 where both are exactly equal)."""
    got, ref64 = np.asarray(got, dtype=F32).astype(F64), np.asarray(ref64, dtype=F64)
    with np.errstate(over="ignore"):
        spacing = np.spacing(np.abs(ref64).astype(F32)).astype(F64)
    return np.abs(got - ref64) / spacing
