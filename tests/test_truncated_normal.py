"""rlx_truncated_normal_sample (csrc/explore_dist.hip, csrc/normal_cdf.hpp) against an fp64 Python evaluation of the same
inverse-CDF formula: ndtr from math.erfc, ndtri by bisection on it — independent of the Cephes rational forms the device
uses."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_ref as N  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
EPS = 2.0 ** -53
# error of the device ndtri on the arguments of U64 against the bisection reference, relative to max(|x|, 1): measured
# 3.6 eps (at the joint exp(-2)), recorded with a margin of 2x
NDTRI_REL = 8 * EPS
# a sample: p = ndtr(a) + u (ndtr(b) - ndtr(a)) carries at most 20 eps of absolute error on the device and as much in
# the reference (erfc good to 5 ulp, three values of at most 1 combined), where p is near 1; z = ndtri(p) multiplies it
# by 1 / phi(z) <= 1 / phi(2.9) = 170 inside the windows below, the standard deviation by <= 0.55:
# 2 * 20 * 170 * 0.55 eps = 3700 eps.  (In a tail p is RELATIVELY accurate, to (5 + 1.5 z^2) eps <= 210 eps at |z| <= 11.7,
# and z moves by p / phi(z) ~ 1 / |z| of that: far below.)
SAMPLE_TOL = 4.1e-13
STREAM = 192                    # RLX_TN_STREAM


def ndtr(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def ndtri(p):
    """the x with ndtr(x) = p, by bisection in the lower tail (p <= 1/2; above, -ndtri(1 - p), 1 - p exact)"""
    if p > 0.5:
        return -ndtri(1.0 - p)
    lo, hi = -40.0, 0.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if ndtr(mid) < p else (lo, mid)
    return 0.5 * (lo + hi)


def sample(m, sd, lo, hi, u):
    """the formula of rlx.h for one element -> (value, refused)"""
    clipped = min(max(m, lo), hi)
    if not sd > 0 or not lo < hi:
        return clipped, True
    a, b = (lo - m) / sd, (hi - m) / sd
    if a > 0:
        qa, qb = ndtr(-a), ndtr(-b)
        z = -ndtri(qa - u * (qa - qb))
    else:
        z = ndtri(ndtr(a) + u * (ndtr(b) - ndtr(a)))
    return min(max(m + sd * z, lo), hi), False


def launch(dev, mean, std, kind, low, high, u=None, draw_state=None, seed=0, rank=0):
    import torch
    from coach_amd import _rlx
    n_env, D = mean.shape
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    out = torch.full((n_env * D + 1,), 7.0, dtype=torch.float32, device=dev)          # + a guard element
    out64 = torch.full((n_env * D + 1,), 7.0, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _rlx.lib().truncated_normal_sample(t(mean, torch.float32), t(std, torch.float32), kind, t(low, torch.float32),
                                       t(high, torch.float32), None if u is None else t(u, torch.float64), draw_state,
                                       seed, rank, n_env, D, out, out64, status, _rlx.current_stream())
    o, o64 = out.cpu().numpy(), out64.cpu().numpy()
    assert o[-1] == 7.0 and o64[-1] == 7.0 and np.array_equal(o[:-1], o64[:-1].astype(F32))
    return o64[:-1].reshape(n_env, D), int(status.item())


_below = lambda x: float(np.nextafter(x, 0.0))
_above = lambda x: float(np.nextafter(x, 1.0))
U64 = [1e-300, 1e-17, 2.0 ** -53, 1.0 - 2.0 ** -53, 0.5, _below(0.5), _above(0.5)] + \
      [f(j) for j in (0.02425, math.exp(-2.0), 1.0 - math.exp(-2.0), math.exp(-32.0)) for f in (_below, float, _above)] + \
      [float(v) for v in np.random.RandomState(7).random_sample(30)] + \
      [float(10.0 ** -k) for k in (1, 2, 3, 5, 8, 12, 20, 40, 80, 120, 160, 200, 240, 280, 307)]


def test_ndtri_through_the_sample_entry(dev):
    """mean 0, std 1, bounds +-40: ndtr(-40) = 0 and ndtr(40) = 1 exactly, so the sample is ndtri(u).  64 fixed u: the
    ends of the range, 1/2, the joints of the three rational forms (exp(-2), 1 - exp(-2), exp(-32)) and 0.02425, each
    with its neighbours, 30 seeded values and a ladder of powers of ten down to 1e-307."""
    assert len(U64) == 64
    u = np.array(U64).reshape(64, 1)
    got, status = launch(dev, np.zeros((64, 1)), [1.0], 0, [-40.0], [40.0], u)
    ref = np.array([ndtri(v) for v in U64])
    # relative to |x| where |x| >= 1, absolute inside: near u = 1/2 only the absolute error means anything (x enters a
    # sample as mean + std x, and neither ndtri nor the bisection resolves u - 1/2 below eps)
    rel = np.abs(got[:, 0] - ref) / np.maximum(np.abs(ref), 1.0)
    print("ndtri: max relative error %.2f eps at u = %r" % (rel.max() / EPS, U64[int(rel.argmax())]))
    assert status == 0 and rel.max() <= NDTRI_REL


WINDOWS = {                     # mean, std, low, high
    "centred": (0.3, 0.5, -1.0, 1.0),
    "far_tail": (0.0, 0.1, 0.9, 1.0),          # a = 9: the upper-tail branch
    "degenerate": (1.4, 0.0, -1.0, 1.0),       # refused: the clipped mean and the status bit
}


@pytest.mark.parametrize("window", sorted(WINDOWS))
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n_env, D", [(1, 1), (3, 2), (65, 3)])
def test_samples_match_the_formula(dev, n_env, D, kind, window):
    m, sd, lo, hi = WINDOWS[window]
    rng = np.random.RandomState(n_env * 10 + D)
    span = hi - lo
    mean = (m + 0.05 * span * rng.uniform(-1, 1, (n_env, D))).astype(F32)
    full = (sd * (1 + 0.1 * rng.uniform(-1, 1, (n_env, D)))).astype(F32)
    std = [full[0, :1], full[0], full][kind]
    low, high = (lo + 0.01 * np.arange(D)).astype(F32), (hi - 0.01 * np.arange(D)).astype(F32)
    u = rng.random_sample((n_env, D))
    got, status = launch(dev, mean, std, kind, low, high, u)
    sd_of = lambda e, d: float(full[0, 0] if kind == 0 else full[0, d] if kind == 1 else full[e, d])
    ref = [[sample(float(mean[e, d]), sd_of(e, d), float(low[d]), float(high[d]), u[e, d]) for d in range(D)]
           for e in range(n_env)]
    want = np.array([[v for v, _ in row] for row in ref])
    assert status == (2 if window == "degenerate" else 0)             # RLX_EXPLORE_STATUS_BAD_WINDOW
    assert (got >= low).all() and (got <= high).all()
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print("truncated normal %s kind %d %dx%d: max error %.3g" % (window, kind, n_env, D, err.max()))
    assert err.max() <= SAMPLE_TOL


def _device_uniforms(draw, n, seed, rank):
    el = np.arange(n, dtype=np.uint64)
    words = N.philox4x32_10(el, np.full(n, STREAM), np.full(n, draw & 0xFFFFFFFF),
                            np.full(n, (draw >> 32) ^ N.NOISE_TAG), seed, rank)
    return N.uniforms(*words)[0]


def test_device_draws_follow_the_counter_and_the_philox_twin(dev):
    import torch
    n_env, D, seed, rank = 200, 3, 11, 2                              # 600 elements: three workgroups share the ticket
    mean = np.zeros((n_env, D), dtype=F32)
    state = torch.tensor([5, 0], dtype=torch.int64, device=dev)
    runs = []
    for start in (5, 6, 5, (1 << 33) + 1):
        state.copy_(torch.tensor([start, 0], dtype=torch.int64))
        got, status = launch(dev, mean, [0.5], 0, [-1.0] * D, [1.0] * D, None, state, seed, rank)
        assert status == 0 and state.cpu().tolist() == [start + 1, 0]          # advanced once, the ticket back at zero
        u = _device_uniforms(start, n_env * D, seed, rank)
        want = np.array([sample(0.0, 0.5, -1.0, 1.0, v)[0] for v in u]).reshape(n_env, D)
        assert np.abs(got - want).max() <= SAMPLE_TOL
        runs.append(got)
    assert np.array_equal(runs[0], runs[2]) and not np.array_equal(runs[0], runs[1])


def test_a_replayed_graph_draws_new_samples(dev):
    import torch
    from coach_amd import _rlx
    n_env, D = 100, 3
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    mean, std = torch.zeros(n_env, D, dtype=torch.float32, device=dev), t([0.5], torch.float32)
    low, high = t([-1.0] * D, torch.float32), t([1.0] * D, torch.float32)
    out, status = torch.zeros(n_env, D, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    state = torch.zeros(2, dtype=torch.int64, device=dev)
    call = lambda: _rlx.lib().truncated_normal_sample(mean, std, 0, low, high, None, state, 3, 0, n_env, D, out, None,
                                                      status, _rlx.current_stream())
    eager = []
    for _ in range(4):                                                # draws 0 .. 3, launch by launch
        call()
        eager.append(out.cpu().numpy().copy())
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()                                                        # (warm)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    state.zero_()
    for k in range(4):
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), eager[k])
    assert not np.array_equal(eager[0], eager[1]) and state.cpu().tolist() == [4, 0]
