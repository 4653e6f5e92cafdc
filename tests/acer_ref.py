"""numpy restatement of the ACER agent's arithmetic on ONE update window (agents/acer_agent.py:118-165 of the reference
for the Q-retrace targets, heads/acer_policy_head.py:47-113 for the policy head, heads/head.py:143-186 for the Q head's
loss), the twin of csrc/acer.hip, and of the consecutive-transition draw of the episodic replay
(memories/episodic/episodic_experience_replay.py:112-119).  The policy row arithmetic (softmax, p + eps, the normalised
log pi, the entropy) is tests/pg_ref.py's head_rows; it is imported, not restated.

The window (window_values).  The reference mixes the networks' fp32 outputs, fp64 rewards (np.array of Python floats)
and Python floats; what an intermediate's type is follows numpy's promotion rule (NEP 50, numpy >= 2; the fixture
tests/golden/acer.npz names its numpy).  The rounding points, by the reference's line:
  :129  current_state_values = np.sum(policy_prob * Q_values, axis=1): an fp32 product, then numpy's add.reduce over the
        contiguous last axis (np_sum_rows): a plain loop for A < 8, from A = 8 on eight interleaved accumulators over the
        multiples of 8, folded as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), the remainder added in order.
  :138  rho = policy_prob / (mu + eps): eps is the np.float32 scalar, mu the stored fp32 probabilities: fp32 throughout.
  :141  rho_bar = np.minimum(1.0, rho_i): fp32 (the Python float is weak).
  :144  Qret = 0 (the int) on a game over;
  :147  else the fp32 scalar np.sum(Q * p, axis=1)[0] of the state behind the window (the same reduction).
  :150  `discount * Qret` on the FIRST pass when bootstrapped: the Python float is weak, so an fp32 product of
        fp32(discount) and the fp32 scalar.  `batch.rewards()[i] + ...` adds an np.float64 scalar, which is not weak:
        Qret is fp64 from then on, and every later product and sum is fp64.  With a game over everything is fp64.
  :151  the store into the fp32 matrix rounds once; Qret itself stays fp64.
  :152  rho_bar[i] * (Qret - Q_i[i]) + V[i]: np.float32 scalars meeting an np.float64 scalar, all strong: fp64 on the
        widened values.
  :133  Q_head_targets = Q_values is the SAME array: the matrix handed to the policy head as 'output_1_3' carries the
        retrace values in the taken entries (td_targets here serves as both).  Q_i (:135) is a copy made before.
A row whose action is outside [0, A) (the reference would raise) is defined as: rho_i = 0 and Q_i = 0, so the
recurrence passes V_i on; its td_targets row stays the online row.

The heads (head_losses; fp32, every mean divides by T, the batch sums are the device's a3c_ref.tree_sum):
  Q head       e_b = Q[b][a_b] - q_retrace_b;  l, g = e^2, 2e;  Q loss = (1/T) sum_b w * l_b;  dQ[b][a_b] = ((1 * w) * g) / T
               and every other entry exactly 0 (the target matrix equals the prediction there).
  policy head  p, q = p + eps, S, log pi, H of pg_ref.head_rows.
               probability term_b     = (log pi_b(a_b) * (q_retrace_b - V_b)) * min(c, rho_i_b)                  (:75-79)
               bias-correction term_b = sum_k ((log(q_k) * (Q'_k - V)) * relu(1 - c / (rho_k + eps))) * p_k     (:81-88)
                   log(q_k) is NOT normalised; the trailing p_k is under stop_gradient; Q' is the aliased matrix
               KL term_b              = sum_k (qa_k / Sa) * (log pi_avg,k - log pi_k), qa = avg + eps, Sa = sum qa (:98-100)
               probability loss = -(1/T) sum, bias-correction loss = -(1/T) sum, policy loss = their sum (:90),
               total = Q loss + (policy loss - beta * mean H) (the regulariser exists when beta != 0, :56-58).
  gradient     g_k = dL/dp_k of the row = (beta / T) (log pi_k + H) / S - (coef / T) ([k == a] / q_a - 1 / S) - (w_k / q_k) / T
               with coef = (q_retrace - V) * min(c, rho_i) and w_k = ((Q'_k - V) * relu(1 - c / (rho_k + eps))) * p_k
  trust region (the layer's `grad`, :103-112, applied to g when asked): g' = (-g) * T;  k = -(avg / q);
               adj = relu((sum k g' - delta) / (sum k^2 + eps));  g' = g' - adj * k;  g = (-g') / T
  dlogits      dz_j = p_j (g_j - sum_k g_k p_k)
The reference builds its losses from policy_probs BEFORE `self.output = trust_region_layer(self.output)`, and
tf.gradients(total_loss, weights) never meets that identity tensor: the layer changes no gradient there.  The faithful
default is trust = False.
"""
import numpy as np

import pg_ref
from a3c_ref import tree_sum
from pg_ref import _seq_sum

F32 = np.float32
EPS = np.finfo(np.float32).eps                                       # rl_coach/utils.py: eps
MODE_TRUST_REGION, MODE_TARGETS_GIVEN = 1, 2                         # RLX_ACER_*
STATUS_BAD_ACTION, STATUS_NO_BOOTSTRAP_ROW = 1, 2
SCALARS = ("loss", "q_loss", "policy_loss", "probability_loss", "bias_correction_loss", "kl", "entropy")


def np_sum_rows(x):
    """np.sum(x, axis=-1) of a C-contiguous fp32 array, restated (numpy/_core/src/umath/loops_utils.h, pairwise_sum,
    n <= 128): every addition is one fp32 addition"""
    x = np.asarray(x)
    A = x.shape[-1]
    if A < 8:
        return _seq_sum(x)
    r = [x[..., j] for j in range(8)]
    i = 8
    while i < A - A % 8:
        r = [r[j] + x[..., i + j] for j in range(8)]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for j in range(i, A):
        res = res + x[..., j]
    return res


def _valid(actions, A):
    act = np.asarray(actions).reshape(-1)
    valid = (act >= 0) & (act < A)
    return act, valid, np.where(valid, act, 0)


def window_values(Q, P, mu, actions, rewards, game_over, discount, boot=None, first_product_fp64=False):
    """Q, P (the online network's Q values and policy probabilities on the window's states), mu (the stored behaviour
    probabilities): fp32 [T, A]; rewards: the filtered rewards, fp32-exact; boot: np_sum_rows(Q * p) of the state behind
    the window (fp32; unused with a game over).  first_product_fp64 is the OTHER candidate for :150's first product
    (what the fixture tells apart) -> dict(V, rho, rho_i, q_retrace [T] fp32, td_targets [T, A])"""
    Q, P, mu = (np.asarray(v, dtype=F32) for v in (Q, P, mu))
    T, A = Q.shape
    act, valid, a = _valid(actions, A)
    rows = np.arange(T)
    r = np.asarray(rewards, dtype=np.float64).reshape(-1)
    V = np_sum_rows(P * Q)                                           # :129
    rho = P / (mu + F32(EPS))                                        # :138
    rho_i = np.where(valid, rho[rows, a], F32(0)).astype(F32)
    rho_bar = np.minimum(F32(1), rho_i)                              # :141
    Q_i = np.where(valid, Q[rows, a], F32(0)).astype(F32)            # :135, a copy
    if game_over:
        p = 0.0
    elif first_product_fp64:
        p = discount * np.float64(F32(boot))
    else:
        p = np.float64(F32(discount) * F32(boot))                    # :150, first pass
    q_retrace = np.empty(T, dtype=F32)
    for i in reversed(range(T)):
        R = r[i] + p
        q_retrace[i] = R                                             # :151, the rounding
        Qret = np.float64(rho_bar[i]) * (R - np.float64(Q_i[i])) + np.float64(V[i])      # :152
        p = discount * Qret
    td = Q.copy()
    td[rows[valid], a[valid]] = q_retrace[valid]                     # :133, :151: the aliased matrix
    return dict(V=V, rho=rho, rho_i=rho_i, q_retrace=q_retrace, td_targets=td, valid=valid)


def bootstrap_value(Q_row, P_row):
    """:147 on the one row behind the window"""
    return np_sum_rows((np.asarray(P_row, F32) * np.asarray(Q_row, F32)).reshape(1, -1))[0]


def trust_region(g, avg, q, delta, fT, dtype=F32):
    """the layer's `grad` (:103-112) on rows of g = dL/dp"""
    gp = (-g) * fT
    k = -(avg / q)
    adj = np.maximum((_seq_sum(k * gp) - dtype(delta)) / (_seq_sum(k * k) + dtype(EPS)), dtype(0))
    gp = gp - adj[:, None] * k
    return (-gp) / fT, adj


def head_rows_terms(logits, avg, rho, rho_i, q_retrace, V, td, actions, c, dtype=F32, p_stop=None):
    """the per-row terms of the policy head, rows [T, A] -> dict; p_stop replaces the stop_gradient factor"""
    x = np.asarray(logits, dtype=dtype)
    T, A = x.shape
    act, valid, a = _valid(actions, A)
    rows = np.arange(T)
    p, q, S, lp, H = pg_ref.head_rows(x, dtype)
    log = (lambda v: np.log(v.astype(np.float64)).astype(F32)) if dtype is F32 else np.log
    c, eps = dtype(c), dtype(EPS)
    adv = np.asarray(q_retrace, dtype) - np.asarray(V, dtype)
    trunc = np.minimum(c, np.asarray(rho_i, dtype))
    prob = (lp[rows, a] * adv) * trunc
    f = np.maximum(dtype(1) - c / (np.asarray(rho, dtype) + eps), dtype(0))
    dQ = (np.asarray(td, dtype) - np.asarray(V, dtype)[:, None]) * f
    ps = p if p_stop is None else p_stop
    bias = _seq_sum(((log(q) * (np.asarray(td, dtype) - np.asarray(V, dtype)[:, None])) * f) * ps)
    qa = np.asarray(avg, dtype) + eps
    Sa = _seq_sum(qa)
    lpa = log(qa) - log(Sa)[:, None]
    kl = _seq_sum((qa / Sa[:, None]) * (lpa - lp))
    return dict(p=p, q=q, S=S, lp=lp, H=H, prob=prob, bias=bias, kl=kl, coef=adv * trunc, w=dQ * ps, valid=valid, a=a)


def head_losses(Q, logits, avg, rho, rho_i, q_retrace, V, td, actions, c=10.0, delta=1.0, beta=0.0, q_weight=0.5,
                trust=False, T=None, dtype=F32, total=tree_sum):
    """Q, logits [R, A] with R = T or T + 1 (the bootstrap row has no term and zero gradient rows); the other arrays
    have T rows -> the seven scalars, dQ [R, A], dlogits [R, A], status"""
    Q, x = np.asarray(Q, dtype=dtype), np.asarray(logits, dtype=dtype)
    R, A = x.shape
    T = R if T is None else T
    t = head_rows_terms(x[:T], avg, rho, rho_i, q_retrace, V, td, np.asarray(actions)[:T], c, dtype)
    valid, a, rows = t["valid"], t["a"], np.arange(T)
    fT, w, b, zero = dtype(T), dtype(q_weight), dtype(beta), dtype(0)
    e = Q[rows, a] - np.asarray(q_retrace, dtype)
    q_loss = total(np.where(valid, w * (e * e), zero)) / fT
    dQ = np.zeros((R, A), dtype=dtype)
    dQ[rows[valid], a[valid]] = (((dtype(1) * w) * (dtype(2) * e)) / fT)[valid]
    prob_loss = -(total(np.where(valid, t["prob"], zero)) / fT)
    bias_loss = -(total(np.where(valid, t["bias"], zero)) / fT)
    kl = total(np.where(valid, t["kl"], zero)) / fT
    mean_h = total(np.where(valid, t["H"], zero)) / fT
    policy_loss = prob_loss + bias_loss
    p, q, S, lp, H = t["p"], t["q"], t["S"], t["lp"], t["H"]
    onehot = np.zeros((T, A), dtype=dtype)
    onehot[rows, a] = 1
    dlog = onehot * (dtype(1) / q) - (dtype(1) / S)[:, None]
    g = (b / fT) * ((lp + H[:, None]) / S[:, None]) - (t["coef"] / fT)[:, None] * dlog - (t["w"] / q) / fT
    adj = np.zeros(T, dtype=dtype)
    if trust:
        g, adj = trust_region(g, np.asarray(avg, dtype), q, delta, fT, dtype)
    dot = _seq_sum(g * p)
    dz = np.zeros((R, A), dtype=dtype)
    dz[:T] = np.where(valid[:, None], p * (g - dot[:, None]), zero)
    return dict(loss=q_loss + (policy_loss - b * mean_h), q_loss=q_loss, policy_loss=policy_loss,
                probability_loss=prob_loss, bias_correction_loss=bias_loss, kl=kl, entropy=mean_h, dQ=dQ, dlogits=dz,
                adj=adj, status=0 if valid.all() else STATUS_BAD_ACTION)


def policy_loss64(logits, p_stop, avg, rho, rho_i, q_retrace, V, td, actions, c, beta):
    """the policy head's loss (+ regulariser) in fp64 with numpy's own sums and the stop_gradient factor held at
    p_stop: what the gradient test differentiates"""
    t = head_rows_terms(logits, avg, rho, rho_i, q_retrace, V, td, actions, c, np.float64, p_stop=p_stop)
    return -t["prob"].mean() - t["bias"].mean() - beta * t["H"].mean()


def window_loss(Q, logits, avg_logits, mu, actions, rewards, game_over, discount, c=10.0, delta=1.0, beta=0.0,
                q_weight=0.5, trust=False):
    """everything rlx_acer_window_loss computes: Q, logits [R, A] with R = T + 1 (the last row is the state behind the
    window) or R = T (allowed only with a game over); avg_logits: the average network on the T states"""
    Q, x = np.asarray(Q, dtype=F32), np.asarray(logits, dtype=F32)
    T = len(rewards)
    if Q.shape[0] == T and not game_over:
        return dict(status=STATUS_NO_BOOTSTRAP_ROW)
    P = pg_ref.head_rows(x)[0]
    avg = pg_ref.head_rows(np.asarray(avg_logits, dtype=F32)[:T])[0]
    boot = bootstrap_value(Q[T], P[T]) if Q.shape[0] > T and not game_over else F32(0)   # :143-147: not asked for
    w = window_values(Q[:T], P[:T], mu, actions, rewards, game_over, discount, boot)
    out = head_losses(Q, x, avg, w["rho"], w["rho_i"], w["q_retrace"], w["V"], w["td_targets"], actions, c, delta, beta,
                      q_weight, trust, T)
    return dict(w, avg=avg, boot=boot, **out)


# ---------------------------------------------------------------------------------------------------- the replay
def sample_consecutive(lengths, size, rng=np.random):
    """EpisodicExperienceReplay.sample(size, is_consecutive_transitions=True) (:112-119) over complete episodes of
    `lengths` (oldest first), draw for draw -> (episode, start, stop): transitions [start, stop) of that episode.
    randint(size, length) is the window's END and never reaches the episode's last transition: an episode longer than
    `size` never yields its terminal transition; a shorter or equal one is taken whole."""
    if len(lengths) == 0:
        raise ValueError("The episodic replay buffer cannot be sampled since there are no complete episodes yet.")
    e = rng.randint(0, len(lengths))                                 # :113 (num_complete_episodes())
    n = int(lengths[e])
    if n <= size:                                                    # :115-116
        return e, 0, n
    end = rng.randint(size, n)                                       # :118
    return e, end - size, end
