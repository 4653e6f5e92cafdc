"""tests/optim_ref.py against things it does not share code with: a thread-by-thread loop for the summation order, the
float64 sum and the derived bound for its value, the library's own host-side geometry (rlx_adam_step_blocks), a float64
Adam for oracle.optim.AdamTF1.  No GPU."""
import ctypes

import numpy as np
import pytest

import optim_ref as R
from oracle.optim import AdamTF1, mix_weights

F32, F64 = np.float32, np.float64

#             n, blocks: the geometries tests/test_optim_kernels.py runs
GEOMETRIES = [(n, R.adam_blocks(n, 1024)) for n in (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1027)] + \
             [(4093, 1), (4096, 1), (4099, 1), (4100, 1), (3 * 4096 - 5, 3), (40003, 33), (40003, 40)]


def _norm_by_threads(g, blocks):
    """the summation order of optim_ref's docstring, one thread after the other in scalar fp32 arithmetic"""
    g = np.asarray(g, dtype=F32)
    n = g.size
    n4, stride = n >> 2, blocks * 256
    part = []
    for b in range(blocks):
        red = []
        for tid in range(256):
            ss = F32(0)
            i = b * 256 + tid
            while i < n4:
                for k in range(4):
                    ss = F32(ss + F32(g[4 * i + k] * g[4 * i + k]))
                i += stride
            i = 4 * n4 + b * 256 + tid
            if i < n:
                ss = F32(ss + F32(g[i] * g[i]))
            red.append(ss)
        d = 128
        while d:
            for t in range(d):
                red[t] = F32(red[t] + red[t + d])
            d //= 2
        part.append(red[0])
    red = []
    for tid in range(256):
        s = F32(0)
        for i in range(tid, blocks, 256):
            s = F32(s + part[i])
        red.append(s)
    d = 128
    while d:
        for t in range(d):
            red[t] = F32(red[t] + red[t + d])
        d //= 2
    return np.sqrt(red[0]), np.array(part, dtype=F32)


@pytest.mark.parametrize("n,blocks", [(1, 1), (5, 1), (1027, 2), (4099, 1), (4100, 1), (3 * 4096 - 5, 3), (1500, 300)])
def test_norm_f32_adds_in_the_stated_order(n, blocks):
    """(1500, 300): more blocks than the finishing workgroup has threads -> its threads add two partial sums each"""
    g = np.random.RandomState(n).randn(n).astype(F32)
    got, part = R.norm_f32(g, blocks)
    want, want_part = _norm_by_threads(g, blocks)
    assert got.dtype == F32 and part.dtype == F32
    assert np.array_equal(part.view(np.uint32), want_part.view(np.uint32))
    assert F32(got).view(np.uint32) == F32(want).view(np.uint32)


@pytest.mark.parametrize("n,blocks", GEOMETRIES)
def test_norm_f32_is_within_the_derived_bound_of_the_float64_sum(n, blocks):
    for seed in range(3):
        g = (np.random.RandomState(seed * 131 + n).randn(n) * 10.0 ** (seed - 1)).astype(F32)
        got, _ = R.norm_f32(g, blocks)
        exact = R.norm_f64(g)
        rel = abs(F64(got) - exact) / exact
        assert rel <= R.norm_bound(n, blocks), (rel, R.norm_bound(n, blocks))
    # the bound is of the order of the additions on the longest path, not a loose constant
    assert R.norm_bound(n, blocks) < (R.norm_depth(n, blocks) + 4) * R.U24
    assert 17 <= R.norm_depth(n, blocks) <= 4 * 5 + 1 + 8 + 1 + 8


def test_norm_depth_counts_the_longest_path():
    assert R.norm_depth(1, 1) == 1 + 8 + 1 + 8               # no float4, one tail element
    assert R.norm_depth(4096, 1) == 16 + 8 + 1 + 8           # four float4s per thread
    assert R.norm_depth(4099, 1) == 17 + 8 + 1 + 8
    assert R.norm_depth(4100, 1) == 20 + 8 + 1 + 8           # a fifth, strided
    assert R.norm_depth(1500, 300) == 4 + 8 + 2 + 8


def test_norm_f32_nonfinite_as_numpy():
    g = np.random.RandomState(0).randn(1027).astype(F32)
    for bad, check in ((np.nan, np.isnan), (np.inf, np.isposinf), (-np.inf, np.isposinf), (1e20, np.isposinf)):
        h = g.copy()
        h[600] = bad
        with np.errstate(over="ignore", invalid="ignore"):
            numpy_says = np.sqrt(np.sum(h * h, dtype=F32))
        assert check(numpy_says) and check(R.norm_f32(h, 2)[0]), bad
    h = g.copy()
    h[[3, 1026]] = [np.inf, np.nan]
    assert np.isnan(R.norm_f32(h, 2)[0])


@pytest.mark.parametrize("n,ws", [(n, 1024) for n in (1, 3, 4, 1023, 1024, 1027, 262144, 1 << 20, (1 << 20) + 4, 5000000)] +
                         [(4093, 1), (4096, 1), (4099, 1), (4100, 1), (3 * 4096 - 5, 3), (40003, 33), (40003, 4096)])
def test_geometry_is_the_librarys(n, ws):
    """rlx_adam_step_blocks is host code: it answers without a GPU"""
    from coach_amd import _rlx
    b = ctypes.c_int(-1)
    _rlx.lib().adam_step_blocks(n, ws, ctypes.byref(b))
    blocks = R.adam_blocks(n, ws)
    assert b.value == (blocks if R.register_held(n, blocks) else 0)
    assert (n, ws) != (4100, 1) or b.value == 0
    assert (n, ws) != (4099, 1) or b.value == 1


def test_adam_oracle_is_the_fp32_rounding_of_a_float64_adam():
    """three steps of oracle.optim.AdamTF1 against the same update in float64 (its beta powers included): a handful of fp32
    roundings per element and step apart.  m and v are differences of numbers up to |g| ~ 4 and |g|^2 ~ 16: their error is
    a few roundings of THOSE (2^-24 each), hence the absolute terms"""
    rng = np.random.RandomState(3)
    n, lr, b1, b2, eps = 1027, 2.5e-4, 0.9, 0.99, 1e-4
    w32 = rng.randn(n).astype(F32)
    w64, m, v, p1, p2 = w32.astype(F64), np.zeros(n), np.zeros(n), F64(F32(b1)), F64(F32(b2))
    f1, f2, le, ee = F64(F32(b1)), F64(F32(b2)), F64(F32(lr)), F64(F32(eps))
    opt = AdamTF1(n, lr, b1, b2, eps)
    for s in range(3):
        g = rng.randn(n).astype(F32)
        R.step_reference(opt, w32, g, 0.5)
        gs = g.astype(F64) * 0.5
        alpha = le * np.sqrt(1 - p2) / (1 - p1)
        m += (gs - m) * (1 - f1)
        v += (gs * gs - v) * (1 - f2)
        w64 -= m * alpha / (np.sqrt(v) + ee)
        p1, p2 = p1 * f1, p2 * f2
        np.testing.assert_allclose(w32, w64, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(opt.m, m, rtol=1e-6, atol=8 * 4 * R.U24)
        np.testing.assert_allclose(opt.v, v, rtol=1e-6, atol=8 * 16 * R.U24)
        np.testing.assert_allclose([opt.b1p, opt.b2p], [p1, p2], rtol=3e-7)
    assert w32.dtype == F32 and opt.m.dtype == F32 and opt.v.dtype == F32 and type(opt.b1p) is F32


def test_step_reference_mixes_towards_the_new_weights():
    rng = np.random.RandomState(4)
    w, t, g = rng.randn(9).astype(F32), rng.randn(9).astype(F32), rng.randn(9).astype(F32)
    opt, t0 = AdamTF1(9, 1e-3), t.copy()
    R.step_reference(opt, w, g, 1.0, t, 0.005)
    want = F32(0.005) * w + F32(1.0 - 0.005) * t0
    assert np.array_equal(t.view(np.uint32), want.view(np.uint32)) and t.dtype == F32
    t[3] = np.nan
    with np.errstate(invalid="ignore"):
        assert np.isnan(mix_weights(t, w, 1.0)[3])

