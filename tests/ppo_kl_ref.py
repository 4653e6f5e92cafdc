"""numpy float64 restatement of the PPO-penalty head of csrc/ppo_kl.hip and of its coefficient update, written from the
reference (paths under rl_coach/): architectures/tensorflow_components/heads/ppo_head.py:52-98 built with
clip_likelihood_ratio_using_epsilon = None and use_kl_regularization, and agents/ppo_agent.py:296-353.

    surrogate = -mean_b(ratio_b adv_b)                                                   ppo_head.py:88-90
    KL        = mean_b KL(old_b || new_b),    entropy = mean_b H(new_b)                   :62-66
    total     = surrogate + kl_coefficient KL + high max(0, KL - kl_cutoff)^2 - beta entropy      :68-72, :95-97
    c         = d(the two KL terms) / d KL = kl_coefficient + 2 high max(0, KL - kl_cutoff)
    d total / d z_b = (-adv_b ratio_b / B) dlogp_b/dz + (c / B) dKL_b/dz - (beta / B) dH_b/dz,   times grad_scale

The per-row terms (log-probabilities, ratio, entropy, KL, and the dlogp / dH part of the gradient) are those of
tests/head_loss_ref.py, evaluated at a clip range that cannot bind; this module imports them, adds what depends on the
batch mean of the KL, and counts the error bound of every value the way that module does (units of 2^-24, every
coefficient counted from the kernel's chain of fp32 operations and written in the docstring, none measured).

The coefficient update restates update_kl_coefficient in the number types NEP 50 gives its numpy scalars: the fp32
mean KL against the python floats 1.3 * kl_target / 0.7 * kl_target ROUNDED to fp32, the fp32 coefficient times /
divided by 1.5 in fp32."""
import numpy as np

import head_loss_ref as H

F32, F64 = np.float32, np.float64
U24 = H.U24
NO_CLIP = 3.0e38                                      # kNoClip of csrc/ppo_kl.hip: 1 -+ NO_CLIP clips no finite ratio
MAX_ACTIONS, MAX_ACTION_DIM = 18, 32
HINGE_MARGIN = 0.1                                    # |KL - kl_cutoff| >= HINGE_MARGIN |kl_cutoff| in every case


def _f64(x):
    return np.asarray(x, dtype=F32).astype(F64)


# ------------------------------------------------------------------------------------------------ the batch-level part
def kl_penalty(sur, u_sur, ent_term, u_ent_term, kl, u_kl, kl_coefficient, kl_cutoff, high, use_kl):
    """-> dict(c, c_units, total, total_units, side) from the batch means and their units.
    Counted (klc, cutoff, high are fp32 inputs, exact; 2 * high is exact):
      h = max(0, KL - cutoff)      above the hinge: u_kl + |h|;  below: exactly 0 (the cases keep HINGE_MARGIN)
      c = klc + (2 high) h         2 high h_units + |2 high h| + |c|
      s1 = sur + klc KL            u_sur + |klc| u_kl + |klc KL| + |s1|
      s2 = s1 + high (h h)         + high (2 h h_units + h^2) + high h^2 + |s2|
      total = s2 - ent_term        + u_ent_term + |total|
    without use_kl: c = 0 exactly and total = sur - ent_term: u_sur + u_ent_term + |total|."""
    if not use_kl:
        total = sur - ent_term
        return dict(c=0.0, c_units=0.0, total=total, total_units=u_sur + u_ent_term + abs(total), side="off")
    klc, cut, hi = F64(F32(kl_coefficient)), F64(F32(kl_cutoff)), F64(F32(high))
    assert abs(kl - cut) >= HINGE_MARGIN * abs(cut) and U24 * u_kl < 0.1 * abs(kl - cut), \
        "a case on the hinge: KL %r, cutoff %r" % (kl, cut)
    above = kl > cut
    h = kl - cut if above else 0.0
    h_units = u_kl + abs(h) if above else 0.0
    c = klc + 2 * hi * h
    c_units = 2 * hi * h_units + abs(2 * hi * h) + abs(c)
    s1 = sur + klc * kl
    s2 = s1 + hi * h * h
    total = s2 - ent_term
    total_units = (u_sur + abs(klc) * u_kl + abs(klc * kl) + abs(s1) + hi * (2 * h * h_units + h * h) + hi * h * h
                   + abs(s2) + u_ent_term + abs(total))
    return dict(c=c, c_units=c_units, total=total, total_units=total_units, side="above" if above else "below")


# ------------------------------------------------------------------------------------------------ discrete head
def ppo_kl_discrete_loss(logits, actions, advantages, old_probs, beta, kl_coefficient, kl_cutoff, high, use_kl=True,
                         grad_scale=1.0):
    """rlx_ppo_kl_discrete_loss from the logits z [B, n], old probabilities po [B, n], actions [B], advantages [B].
    -> dict of value / value_units pairs: ratio [B] (0 in a rejected row), dlogits [B, n] (0 in a rejected row),
       scalars [5] = surrogate, mean entropy, mean KL, total, c; plus valid [B], side ('below' / 'above' / 'off').
    Phases A and B are head_loss_ref.ppo_discrete_loss at clip range NO_CLIP and grad_scale 1 (the kernel calls
    rlx_losses::ppo_discrete_row with exactly these): g0 = d(surrogate - beta entropy)/dz with its units.  Counted on top:
      entropy term of the total    (beta ent_sum) (1 / B): |beta| (u_ent + 2 |entropy|)
      cb = c / B                   c_units / B + |cb|
      p_j = expf(z_j - max) / se   head_loss_ref.softmax's units (the same chain)
      q_j = po_j / so              n - 1 (so) + 1 = n relative
      k_j = p_j - q_j              p_units_j + n q_j + |k_j|
      t_j = cb k_j                 cb_units |k_j| + |cb| k_units_j + |t_j|
      dlogits_j = grad_scale (g0_j + t_j)      |grad_scale| (g0_units_j + t_units_j + 2 |g0_j + t_j|)"""
    base = H.ppo_discrete_loss(logits, actions, advantages, old_probs, NO_CLIP, beta, None, 1.0)
    assert base["passes"].all()
    z, po = _f64(logits), _f64(old_probs)
    B, n = z.shape
    valid = base["valid"]
    bt, gs = F64(F32(beta)), F64(F32(grad_scale))
    s_sur, s_ent, s_kl = base["scalars"][:3]
    u_sur, u_ent, u_kl = base["scalars_units"][:3]
    pen = kl_penalty(s_sur, u_sur, bt * s_ent, abs(bt) * (u_ent + 2 * abs(s_ent)), s_kl, u_kl, kl_coefficient, kl_cutoff,
                     high, use_kl)
    g0, g0_units = base["dlogits"], base["dlogits_units"]
    if use_kl:
        cb = pen["c"] / B
        cb_units = pen["c_units"] / B + abs(cb)
        p, p_units = H.softmax(logits)
        q = po / po.sum(axis=1, keepdims=True)
        k = p - q
        k_units = p_units + n * q + np.abs(k)
        t = cb * k
        t_units = cb_units * np.abs(k) + abs(cb) * k_units + np.abs(t)
    else:
        t, t_units = np.zeros_like(g0), np.zeros_like(g0)
    g = g0 + t
    dl = gs * g
    dl_units = abs(gs) * (g0_units + t_units + 2 * np.abs(g))
    v = valid[:, None]
    return dict(ratio=np.where(valid, base["ratio"], 0.0), ratio_units=np.where(valid, base["ratio_units"], 0.0),
                dlogits=np.where(v, dl, 0.0), dlogits_units=np.where(v, dl_units, 0.0),
                scalars=np.array([s_sur, s_ent, s_kl, pen["total"], pen["c"]]),
                scalars_units=np.array([u_sur, u_ent, u_kl, pen["total_units"], pen["c_units"]]),
                valid=valid, side=pen["side"], kl_rows=base["kl_rows"])


def discrete_total(logits, actions, advantages, old_probs, beta, kl_coefficient, kl_cutoff, high, use_kl):
    """the total loss alone, in float64 from float64 logits (for central differences)"""
    z, po, adv = np.asarray(logits, F64), np.asarray(old_probs, F64), np.asarray(advantages, F64)
    a = np.asarray(actions)
    rows = np.arange(z.shape[0])
    lp = z - z.max(axis=1, keepdims=True)
    lp = lp - np.log(np.exp(lp).sum(axis=1, keepdims=True))
    q = po / po.sum(axis=1, keepdims=True)
    sur = -np.mean(np.exp(lp[rows, a] - np.log(q[rows, a])) * adv)
    ent = np.mean(-(np.exp(lp) * lp).sum(axis=1))
    kl = np.mean((q * (np.log(q) - lp)).sum(axis=1))
    total = sur - beta * ent
    if use_kl:
        total += kl_coefficient * kl + high * max(0.0, kl - kl_cutoff) ** 2
    return total


# ------------------------------------------------------------------------------------------------ continuous head
def ppo_kl_continuous_loss(mean, log_std, actions, advantages, old_mean, old_std, beta, kl_coefficient, kl_cutoff, high,
                           use_kl=True, grad_scale=1.0):
    """rlx_ppo_kl_continuous_loss: MultivariateNormalDiag(mean [B, A], exp(log_std [A]) + eps) against
    MultivariateNormalDiag(old_mean, old_std + eps) (ppo_head.py:118-144).
    -> dict of value / value_units pairs: ratio [B], dmean [B, A], dlog_std [A], scalars [5]; plus side.
    ratio, surrogate, entropy (the same in every row) and KL with their units are head_loss_ref.ppo_continuous_loss's at
    clip range NO_CLIP: the kernel RESTATES ppo_continuous_loss_kernel's chain of operations for them.  Counted on top,
    per dimension (R = the ratio's relative units; sd = expf(ls) + eps: 3 relative; sd sd: 7; sdo = old_std + eps: 1):
      g_logp = -adv ratio / B                R + 2
      t = g_logp (x - mu) / (sd sd)          R + 2 + 1 + 1 + 7 + 1 = R + 12
      k = -(mo - mu) / (sd sd)               1 + 7 + 1 = 9
      u = cb k                               cb_units |k| + 9 |cb k| + |u|
      dmean = grad_scale (t + u)             |grad_scale| (t's + u's + 2 |t + u|)
      part1 = g_logp (d^2 / sd^3 - 1 / sd) e         |g_logp e| (15 d^2 / sd^3 + 4 / sd + |difference|) + |part1| (R + 6)
      quo = (sdo^2 + dm^2) / (sd sd)         3 sdo^2 / sd^2 + 3 dm^2 / sd^2 + (1 + 7 + 1) quo  <=  12 quo
      w = (1 - quo) e / sd                   (12 quo + |1 - quo|) e / sd + 7 |w|
      part2 = cb w                           cb_units |w| + |cb| w_units + |part2|
      part = part1 + part2                   + |part|
      dlog_std = grad_scale (sum_b part - beta e / sd)
                                             |grad_scale| (the parts' + log2(threads) sum |part| + 7 |beta e / sd| + 2 |.|)"""
    base = H.ppo_continuous_loss(mean, log_std, actions, advantages, old_mean, old_std, NO_CLIP, beta, None, 1.0)
    assert base["passes"].all()
    mu, x, mo = _f64(mean), _f64(actions), _f64(old_mean)
    ls, adv = _f64(log_std).reshape(-1), _f64(advantages)
    B, A = mu.shape
    bt, gs = F64(F32(beta)), F64(F32(grad_scale))
    s_sur, ent, s_kl = base["scalars"][:3]
    u_sur, u_ent, u_kl = base["scalars_units"][:3]
    pen = kl_penalty(s_sur, u_sur, bt * ent, abs(bt) * (u_ent + abs(ent)), s_kl, u_kl, kl_coefficient, kl_cutoff, high,
                     use_kl)
    ratio = base["ratio"]
    R = (base["ratio_units"] / ratio)[:, None]
    e = np.exp(ls)
    sd = e + H.EPS32
    sdo = _f64(old_std) + H.EPS32
    g_logp = (-adv * ratio / B)[:, None]
    d, dm = x - mu, mo - mu
    t = g_logp * d / (sd * sd)
    t_units = np.abs(t) * (R + 12)
    t3, t1 = d * d / sd ** 3, 1.0 / sd
    part1 = g_logp * (t3 - t1) * e
    part1_units = np.abs(g_logp * e) * (15 * t3 + 4 * t1 + np.abs(t3 - t1)) + np.abs(part1) * (R + 6)
    if use_kl:
        cb = pen["c"] / B
        cb_units = pen["c_units"] / B + abs(cb)
        k = -dm / (sd * sd)
        u = cb * k
        u_units = cb_units * np.abs(k) + 9 * np.abs(u) + np.abs(u)
        quo = (sdo * sdo + dm * dm) / (sd * sd)
        w = (1.0 - quo) * e / sd
        w_units = (12 * quo + np.abs(1.0 - quo)) * e / sd + 7 * np.abs(w)
        part2 = cb * w
        part2_units = cb_units * np.abs(w) + abs(cb) * w_units + np.abs(part2)
    else:
        u, u_units, part2, part2_units = (np.zeros_like(t) for _ in range(4))
    dmean = gs * (t + u)
    dmean_units = abs(gs) * (t_units + u_units + 2 * np.abs(t + u))
    part = part1 + part2
    part_units = part1_units + part2_units + np.abs(part)
    depth = int(np.log2(H.block_for(B)))
    et = bt * e / sd
    inner = part.sum(axis=0) - et
    dls = gs * inner
    dls_units = abs(gs) * (part_units.sum(axis=0) + depth * np.abs(part).sum(axis=0) + 7 * np.abs(et) + 2 * np.abs(inner))
    return dict(ratio=ratio, ratio_units=base["ratio_units"], dmean=dmean, dmean_units=dmean_units,
                dlog_std=dls, dlog_std_units=dls_units,
                scalars=np.array([s_sur, ent, s_kl, pen["total"], pen["c"]]),
                scalars_units=np.array([u_sur, u_ent, u_kl, pen["total_units"], pen["c_units"]]), side=pen["side"])


def continuous_total(mean, log_std, actions, advantages, old_mean, old_std, beta, kl_coefficient, kl_cutoff, high,
                     use_kl):
    """the total loss alone, in float64 from float64 mean / log_std (for central differences)"""
    mu, ls, x = np.asarray(mean, F64), np.asarray(log_std, F64).reshape(-1), np.asarray(actions, F64)
    mo, adv = np.asarray(old_mean, F64), np.asarray(advantages, F64)
    sd, sdo = np.exp(ls) + H.EPS32, np.asarray(old_std, F64) + H.EPS32
    c = H.HALF_LOG_2PI
    logp = (-0.5 * ((x - mu) / sd) ** 2 - np.log(sd) - c).sum(axis=1)
    logpo = (-0.5 * ((x - mo) / sdo) ** 2 - np.log(sdo) - c).sum(axis=1)
    sur = -np.mean(np.exp(logp - logpo) * adv)
    ent = (0.5 + c + np.log(sd)).sum()
    kl = np.mean((np.log(sd / sdo) + (sdo * sdo + (mo - mu) ** 2) / (2.0 * sd * sd) - 0.5).sum(axis=1))
    total = sur - beta * ent
    if use_kl:
        total += kl_coefficient * kl + high * max(0.0, kl - kl_cutoff) ** 2
    return total


# ------------------------------------------------------------------------------------------------ the coefficient
def accumulate(scalar_sets, start=None):
    """the `accumulate` buffer after one launch per entry of scalar_sets (each the launch's fp32 scalars[5]): fp32 sums
    of {mean KL, mean entropy, total, 1} added in launch order (np.mean(loss[key], 0) of ppo_agent.py:303-304 adds the
    rows of a float32 [k, 2] array in this order, then divides by k)"""
    acc = np.zeros(4, dtype=F32) if start is None else np.array(start, dtype=F32)
    for s in scalar_sets:
        s = np.asarray(s, dtype=F32)
        acc = (acc + np.array([s[2], s[1], s[3], 1.0], dtype=F32)).astype(F32)
    return acc


def kl_coefficient_update(epoch_sums, target_kl, kl_coefficient):
    """update_kl_coefficient (ppo_agent.py:329-353) -> (new coefficient, mean KL), both np.float32.
    :324  total_kl = np.mean(fetch_result, 0)[0]: a float32 (the fetches are float32): the fp32 sum over the fp32 count
    :336  kl_coefficient: the float32 value of the tf.Variable
    :339  total_kl > 1.3 * kl_target: float32 against a python float -- weak under NEP 50, so the product of the two
          python floats (fp64) is ROUNDED to fp32 and the comparison is fp32; :342 alike with 0.7
    :341  new_kl_coefficient *= 1.5: float32 times a python float: the fp32 product;  :344 the fp32 quotient"""
    sums = np.asarray(epoch_sums, dtype=F32)
    kl = F32(sums[0] / sums[3])
    c = F32(kl_coefficient)
    hi, lo = F32(1.3 * float(target_kl)), F32(0.7 * float(target_kl))
    if kl > hi:
        c = F32(c * F32(1.5))
    elif kl < lo:
        c = F32(c / F32(1.5))
    return c, kl


# ------------------------------------------------------------------------------------------------ case generators
def cutoff_for(kl_mean, side):
    """a kl_cutoff that puts kl_mean on `side` of the hinge with room to spare: KL = cutoff / 2 below, 2 cutoff above.
    A KL mean of exactly 0 (one action: both policies are the point mass) lies above only a negative cutoff."""
    if kl_mean == 0.0:
        return F32(0.02 if side == "below" else -0.02)
    return F32(2.0 * kl_mean if side == "below" else 0.5 * kl_mean)


def discrete_case(seed, B, n, ld=None, ld_old=None):
    """head_loss_ref.ppo_discrete_case plus the float64 KL mean of the batch"""
    case = H.ppo_discrete_case(np.random.RandomState(seed), B, n, ld=ld, ld_old=ld_old)
    ref = H.ppo_discrete_loss(case["logits"][:, :n], case["actions"], case["advantages"], case["old_probs"][:, :n],
                              NO_CLIP, 0.0)
    case["kl_mean"] = float(ref["scalars"][2])
    return case


def continuous_case(seed, B, A, ld=None, ld_old=None):
    """head_loss_ref.ppo_continuous_case plus the float64 KL mean of the batch"""
    case = H.ppo_continuous_case(np.random.RandomState(seed), B, A, ld=ld, ld_old=ld_old)
    ref = H.ppo_continuous_loss(case["mean"][:, :A], case["log_std"], case["actions"], case["advantages"],
                                case["old_mean"][:, :A], case["old_std"][:, :A], NO_CLIP, 0.0)
    case["kl_mean"] = float(ref["scalars"][2])
    return case


# ------------------------------------------------------------------------------------------------ the training phase
def episode_bounds(lengths):
    """[(first row, one past the last row)] of the dataset's episodes, in order"""
    ends = np.cumsum(np.asarray(lengths, dtype=np.int64))
    return list(zip((ends - np.asarray(lengths)).tolist(), ends.tolist()))


def gae_advantages(V, rewards, lengths, discount, gae_lambda):
    """fill_advantages with the GAE rescaler (ppo_agent.py:163-189) -> (raw, standardised), fp64 [N].
    :163  V = critic.predict(...).squeeze(): fp32 [N]
    :177-178  np.append(V[episode], np.zeros((1,))): the zero bootstrap is fp64, so the rollout's values are WIDENED to
          fp64 and everything below runs in fp64 (unlike ActorCriticAgent.learn_from_batch, whose values stay fp32)
    :181  batch.rewards(): the rewards as fp64
    actor_critic_agent.py:117-118  deltas = r + discount * v[1:] - v[:-1];  gae = lfilter([1], [1, -discount * lambda])
          over the reversed deltas: y_i = delta_i + (discount * lambda) * y_{i+1}, one step after the other
          (a3c_ref.discount_sum)
    :189  (adv - np.mean(adv)) / np.std(adv) over ALL rows: numpy's own pairwise sums, no epsilon"""
    import a3c_ref
    V = np.asarray(V, dtype=F32).reshape(-1)
    r = np.asarray(rewards, dtype=F32).astype(F64)
    raw = np.array([])
    for lo, hi in episode_bounds(lengths):
        v = np.append(V[lo:hi], np.zeros((1,)))
        assert v.dtype == F64
        deltas = r[lo:hi] + discount * v[1:] - v[:-1]
        raw = np.append(raw, a3c_ref.discount_sum(deltas, discount * gae_lambda))
    return raw, (raw - np.mean(raw)) / np.std(raw)


def value_targets(rewards, lengths, discount):
    """train_value_network's targets (:207): Episode.update_discounted_rewards with n_step -1 (core_types.py:780-801,
    pg_ref.returns) per episode, fp64 [N]; the device rounds them to fp32 once"""
    import pg_ref
    r = np.asarray(rewards, dtype=F32)
    return np.concatenate([pg_ref.returns(r[lo:hi], discount) for lo, hi in episode_bounds(lengths)])


def minibatches(n_rows, num_steps, batch_size, epochs=1):
    """[(first row, one past the last)] of every minibatch of `epochs` passes: the training set is the first num_steps
    rows of the dataset (:377), split in dataset order with the tail dropped (:212 / :260), no shuffle (:259)"""
    used = min(int(num_steps), int(n_rows))
    one = [(i * batch_size, (i + 1) * batch_size) for i in range(used // batch_size)]
    return one * epochs


def epoch_means(kl, entropy):
    """the last epoch's means of the fetches (:303-304, :324-326) from the fp32 [epochs, n_batches] tables: what the
    `accumulate` buffer of the last epoch holds, divided by its count"""
    sums = accumulate([[0.0, e, k, 0.0, 0.0] for k, e in zip(np.asarray(kl)[-1], np.asarray(entropy)[-1])])
    return sums, F32(sums[0] / sums[3]), F32(sums[1] / sums[3])
