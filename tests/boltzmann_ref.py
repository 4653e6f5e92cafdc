"""Restatement of Boltzmann.get_action (rl_coach/exploration_policies/boltzmann.py:52-62) with every rounding point written
out — what csrc/explore_dist.hip (rlx_boltzmann_sample) computes per row, fed the same uniform:

  1. x = q / float32(temperature)                       fp32 division (float32 array / Python float)
  2. e = exp(x)                                         fp32 (np.exp here; the device's expf differs by a few ulp)
  3. s = np.sum(e)                                      fp32, numpy's pairwise order (sum_f32 below)
  4. p = e / s                                          fp32 division
  5. p[-1] = float32(1) - np.sum(p[:-1])                fp32, the same order over A - 1 values
  6. np.random.choice(A, p=p): cdf = cumsum of float64(p) in index order; cdf /= cdf[-1];
     action = number of cdf entries <= u (searchsorted side='right'), u the one uniform the call draws.
numpy refuses (ValueError) a p with a NaN or a negative entry; `bad` reports that instead.
"""
import numpy as np

_F = np.float32


def sum_f32(a):
    """np.add.reduce of a contiguous float32 vector, addition by addition: below 8 values a running sum from 0; up to
    128 values eight running sums r[j] over a[j], a[j + 8], ... joined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) +
    (r6 + r7)) with the n % 8 last values added one by one; above 128 the sum of the two halves, the left one
    n / 2 rounded down to a multiple of 8."""
    n = len(a)
    if n < 8:
        res = _F(0.0)
        for v in a:
            res = _F(res + v)
        return res
    if n <= 128:
        r = [_F(a[j]) for j in range(8)]
        i = 8
        while i < n - n % 8:
            r = [_F(r[j] + a[i + j]) for j in range(8)]
            i += 8
        res = _F(_F(_F(r[0] + r[1]) + _F(r[2] + r[3])) + _F(_F(r[4] + r[5]) + _F(r[6] + r[7])))
        for v in a[i:]:
            res = _F(res + v)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _F(sum_f32(a[:n2]) + sum_f32(a[n2:]))


def probabilities(q, temperature, exp=np.exp):
    q = np.asarray(q, dtype=_F)
    e = exp(q / _F(temperature)).astype(_F)
    p = (e / sum_f32(e)).astype(_F)
    p[-1] = _F(1.0) - sum_f32(p[:-1])
    return p


def cdf(p):
    c = np.empty(len(p), dtype=np.float64)
    run = 0.0
    for j, v in enumerate(p):
        run = run + float(v)
        c[j] = run
    return c / c[-1]


def get_action(q, temperature, u):
    """one row -> (action, probabilities float32 [A], bad)"""
    p = probabilities(q, temperature)
    bad = bool((~np.isfinite(p)).any() or (p < 0).any())
    if bad:
        return int(np.argmax(q)), p, True
    return int(np.count_nonzero(cdf(p) <= u)), p, False
