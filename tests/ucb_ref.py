"""numpy restatement of UCB's action values (rl_coach/exploration_policies/ucb.py:76-86), the twin of ucb_egreedy_kernel
(csrc/bootstrapped_dqn.hip), with the arithmetic ORDER written down.

The reference calls np.mean and np.std over axis 0 of a list of K (1, A) fp32 arrays.  numpy reduces that axis head by
head in fp32 (the pairwise summation only applies along a contiguous axis), so per action a:

    s = q[0][a];  s += q[h][a] for h = 1 .. K-1;          mean = s / float32(K)
    d_h = q[h][a] - mean;  acc = d_0 * d_0;  acc += d_h * d_h for h = 1 .. K-1;      std = sqrt(acc / float32(K))
    values = mean + float32(lamb) * std   (TRAIN)         values = mean   (HEATUP, TEST)

every operation rounded to fp32 once (no fused multiply-add).  tests/golden/ucb_chain.npz holds what the reference's own
UCB.get_action produced; `values` must reproduce it bit for bit (tests/test_ucb_chain_ref.py).
The epsilon-greedy choice on the values is EGreedy's, restated in tests/bootstrapped_ref.py (`egreedy`).

  values(q [n, K, A] fp32, lamb, use_std) -> (values [n, A] fp32, std [n, A] fp32 or None)
  same_bits(a, b) -> bool: equal bit for bit, a NaN matching any NaN (IEEE 754 leaves a NaN's sign and payload open, and
      x86 and gfx950 produce different default NaNs from inf - inf)
"""
import numpy as np

from bootstrapped_ref import egreedy  # noqa: F401  (the choice made on the values)

F32 = np.float32


def values(q, lamb, use_std):
    q = np.asarray(q)
    assert q.dtype == F32 and q.ndim == 3
    n, K, A = q.shape
    kf = F32(K)
    with np.errstate(all="ignore"):
        s = q[:, 0].copy()
        for h in range(1, K):
            s = (s + q[:, h]).astype(F32)
        mean = (s / kf).astype(F32)
        if not use_std:
            return mean, None
        d = (q[:, 0] - mean).astype(F32)
        acc = (d * d).astype(F32)
        for h in range(1, K):
            d = (q[:, h] - mean).astype(F32)
            acc = (acc + (d * d).astype(F32)).astype(F32)
        std = np.sqrt((acc / kf).astype(F32)).astype(F32)
        return (mean + (F32(lamb) * std).astype(F32)).astype(F32), std


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))
