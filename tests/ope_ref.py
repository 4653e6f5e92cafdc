"""numpy restatement of the off-policy evaluators of Batch RL: the twin of csrc/ope.hip, pinned to the reference's own
OpeManager / DoublyRobust / SequentialDoublyRobust / WeightedImportanceSampling by tests/test_ope_ref.py (recorded in
tests/golden/ope.npz).

  softmax32(q, T)            fp32 [n, A]: z = q / fp32(T); minus the row maximum; exp in fp32; the sum in action order from
                             fp32(0); one division per entry — every operation rounded to fp32 on its own
                             (heads/q_head.py:56-68 is tf.nn.softmax(q / T))
  behaviour_probabilities(q, u, epsilon, force_uniform, T)
                             fp32 [n_env, A]: the uniform vector fp32(1) / fp32(A) where force_uniform or u < epsilon, else
                             softmax32 (value_optimization_agent.py:98-102, e_greedy.py:84-101, spaces.py:458)
  rows(q, rm, d, actions, rewards, mu, T, pi=None)
                             the per-row columns of rlx_ope_rows, fp64 from fp32 values widened once, sums over the actions
                             in action order: rho, v, q_taken, ips, dm (with the reward model's row j // d), dr, status.
                             pi: use these policy probabilities (a device's, read back) instead of softmax32
  estimates(cols, rewards, episode_offsets, returns, discount)
                             -> (values [5], scales [5], extras): IPS, DM, DR, sequential DR, WIS with np.mean for the
                             dataset means and the reference's sequential per-episode loops (rl/sequential_doubly_robust.py:
                             40-51, rl/weighted_importance_sampling.py:41-55).  A scale is the same computation on absolute
                             values: the mean of |terms|; the recurrence run on |A_j|, |B_j|; sum w |R| / sum w.
  evaluate(...)              rows + estimates

d = the reference's batch size reproduces ope_manager.py:80 (every row of inference batch i is multiplied by the reward
model's output of dataset row i); d = 1 is the direct method of the paper.
"""
import numpy as np

F32 = np.float32
NAMES = ("ips", "dm", "dr", "seq_dr", "wis")


def softmax32(q, T):
    q = np.asarray(q, dtype=F32)
    z = q / F32(T)
    z = z - z.max(axis=1, keepdims=True)
    with np.errstate(under="ignore"):
        e = np.exp(z)
    assert e.dtype == F32
    s = np.zeros(q.shape[0], dtype=F32)
    for k in range(q.shape[1]):
        s = s + e[:, k]
    return e / s[:, None]


def behaviour_probabilities(q, u, epsilon, force_uniform, T):
    q = np.asarray(q, dtype=F32)
    out = softmax32(q, T)
    uniform = np.ones(q.shape[0], dtype=bool) if force_uniform else np.asarray(u, dtype=np.float64) < float(epsilon)
    out[uniform] = F32(1) / F32(q.shape[1])
    return out


def rows(q, rm, d, actions, rewards, mu, T, pi=None):
    q, rm, mu = (np.asarray(x, dtype=F32) for x in (q, rm, mu))
    n, A = q.shape
    pi = softmax32(q, T) if pi is None else np.asarray(pi, dtype=F32)
    actions = np.asarray(actions, dtype=np.int64)
    bad = (actions < 0) | (actions >= A)
    act = np.where(bad, 0, actions)
    j = np.arange(n)
    p64, q64, rm64 = pi.astype(np.float64), q.astype(np.float64), rm.astype(np.float64)
    r = np.asarray(rewards, dtype=F32).astype(np.float64)
    v, dm = np.zeros(n), np.zeros(n)
    for k in range(A):
        v = v + p64[:, k] * q64[:, k]
        dm = dm + p64[:, k] * rm64[j // int(d), k]
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = p64[j, act] / mu.astype(np.float64)[j, act]
        qa = q64[j, act]
        ips = rho * r
        dr = rho * (r - rm64[j, act])
    cols = dict(rho=rho, v=v, q_taken=qa, ips=ips, dm=dm, dr=dr)
    for c in cols.values():
        c[bad] = 0.0
    cols["pi"], cols["status"] = pi, int(bad.any())
    return cols


def estimates(cols, rewards, episode_offsets, returns, discount):
    rho, v, qa = cols["rho"], cols["v"], cols["q_taken"]
    r = np.asarray(rewards, dtype=F32).astype(np.float64)
    off = [int(x) for x in episode_offsets]
    n, E = len(rho), len(off) - 1
    with np.errstate(invalid="ignore", over="ignore"):
        ips, dm = np.mean(cols["ips"]), np.mean(cols["dm"])
        dr = np.mean(cols["dr"]) + dm
        s_ips, s_dm = np.mean(np.abs(cols["ips"])), np.mean(np.abs(cols["dm"]))
        s_dr = np.mean(np.abs(cols["dr"])) + s_dm
        a_abs, b_abs = np.abs(v + rho * (r - qa)), np.abs(discount * rho)
        ep_seq, ep_seq_abs, ep_w = [], [], []
        for e in range(E):
            acc, acc_abs, w = 0.0, 0.0, 1.0
            for j in reversed(range(off[e], off[e + 1])):
                acc = v[j] + rho[j] * (r[j] + discount * acc - qa[j])
                acc_abs = a_abs[j] + b_abs[j] * acc_abs
            for j in range(off[e], off[e + 1]):
                w *= rho[j]
            ep_seq.append(acc)
            ep_seq_abs.append(acc_abs)
            ep_w.append(w)
        seq, s_seq = np.array(ep_seq).mean(), np.array(ep_seq_abs).mean()
        total = sum(ep_w)
        wis, s_wis = 0.0, 0.0
        if total != 0:
            for e in range(E):
                if off[e + 1] > off[e]:
                    wis += ep_w[e] * float(returns[off[e]])
                    s_wis += abs(ep_w[e]) * abs(float(returns[off[e]]))
            wis /= total
            s_wis /= abs(total)
    values = np.array([ips, dm, dr, seq, wis], dtype=np.float64)
    scales = np.array([s_ips, s_dm, s_dr, s_seq, s_wis], dtype=np.float64)
    return values, scales, dict(ep_seq_dr=np.array(ep_seq), ep_seq_dr_scale=np.array(ep_seq_abs), ep_w=np.array(ep_w),
                                sum_w=float(total), episodes=E, rows=n)


def evaluate(q, rm, d, actions, rewards, mu, T, episode_offsets, returns, discount, pi=None):
    cols = rows(q, rm, d, actions, rewards, mu, T, pi=pi)
    values, scales, extras = estimates(cols, rewards, episode_offsets, returns, discount)
    return values, scales, dict(extras, **cols)


def bound(n_terms, scales):
    """|device - restatement| <= (number of terms) * 2^-52 * scale: the worst case of reordering an fp64 sum (or a
    composition of affine maps) of that many terms, two roundings of 2^-53 per term"""
    return float(n_terms) * 2.0 ** -52 * np.asarray(scales, dtype=np.float64)
