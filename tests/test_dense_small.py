"""rlx_dense_small_forward (csrc/dense_small.hip) at its edge: the relu of a narrow head keeps a NaN, as oracle.nn.act does."""
import numpy as np
import pytest

from tests.util import dev_tensor


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2])
def test_relu_head_keeps_a_nan_of_its_row(dev, M):
    """One NaN in x of row 0, N = 1: row 0's output is NaN where oracle.nn.act's is (v > 0 ? v : 0 made it 0), every other
    row keeps the bits of the run without the NaN."""
    import torch
    from coach_amd import _rlx
    from oracle import nn as N
    K = 37
    lib, s_ = _rlx.lib(), _rlx.current_stream()
    rng = np.random.RandomState(M)
    x = rng.randn(M, K).astype(np.float32)
    w = rng.randn(K, 1).astype(np.float32)
    b = np.full(1, 0.5, np.float32)
    if M > 1:
        x[1] = -np.abs(x[1]) * np.sign(w[:, 0])       # row 1 is negative before the relu: its output is the relu's 0

    def run(xh):
        y = torch.full((M, 1), 7.0, dtype=torch.float32, device=dev)
        lib.dense_small_forward(dev_tensor(xh, dev), 0, dev_tensor(w, dev), 0, dev_tensor(b, dev), 0, y, 0, 1, M, K, 1,
                                _rlx.ACT["relu"], s_)
        return y.cpu().numpy()
    clean = run(x)
    xn = x.copy()
    xn[0, 11] = np.nan
    got = run(xn)
    ref = N.act(xn @ w + b, "relu")
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got[0, 0]) and not np.isnan(got[1:]).any()
    assert np.array_equal(got[1:].view(np.uint32), clean[1:].view(np.uint32))
    assert not np.isnan(clean).any() and (M == 1 or clean[1, 0] == 0.0)
