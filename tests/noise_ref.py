"""numpy twin of csrc/noise.hip (rlx_normal_fill): Philox4x32-10 + one Box-Muller pair per call with the same
correctly rounded float64 operations in the same order, so every value agrees bit for bit with the device.  numpy's
elementwise float64 + - * / sqrt are IEEE operations and are never fused, which is what makes the restatement exact.

normal_fill(events, stream0, n_streams, n, seed, rank, scale) -> float64 [len(events)][n_streams][n]."""
import numpy as np

NOISE_TAG = 0x4E4F4953                 # counter word 3 = event high word ^ NOISE_TAG
STREAM_TD3, STREAM_SAC0, STREAM_ACT = 0, 1, 4
_M32 = np.uint64(0xFFFFFFFF)

_LN2_HI = 0.6931471803691238
_LN2_LO = 1.9082149292705877e-10
_SQRT2 = 1.4142135623730951
_ATANH = [0.043478260869565216, 0.047619047619047616, 0.05263157894736842, 0.058823529411764705,
          0.06666666666666667, 0.07692307692307693, 0.09090909090909091, 0.1111111111111111, 0.14285714285714285,
          0.2, 0.3333333333333333, 1.0]
_SIN = [6.0669357311061955e-12, -6.688035109811468e-10, 5.692172921967927e-08, -3.598843235212085e-06,
        0.00016044118478735983, -0.004681754135318688, 0.07969262624616705, -0.6459640975062463,
        1.5707963267948966]
_COS = [-5.294400200734623e-13, 6.565963114979473e-11, -6.386603083791852e-09, 4.710874778818172e-07,
        -2.5202042373060607e-05, 0.0009192602748394266, -0.02086348076335296, 0.25366950790104803,
        -1.2337005501361697, 1.0]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """uint32-valued arrays (any broadcastable shapes) -> the four output words as uint64 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _M32 for k in (k0, k1))
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32)
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def uniforms(x, y, z, w):
    """the two 53-bit uniforms of one Philox call: u1 in (0, 1], and the integer m2 of u2 = m2 2^-53 in [0, 1)."""
    m1 = ((x >> np.uint64(5)) << np.uint64(26)) | (y >> np.uint64(6))
    m2 = ((z >> np.uint64(5)) << np.uint64(26)) | (w >> np.uint64(6))
    return (m1 + np.uint64(1)).astype(np.float64) * 2.0 ** -53, m2


def ln_unit(u):
    """ln u for u in [2^-53, 1]: exponent extraction + 2 atanh((m - 1) / (m + 1)), m in [sqrt 1/2, sqrt 2)."""
    u = np.asarray(u, dtype=np.float64)
    b = u.view(np.uint64)
    e = ((b >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    m = ((b & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m >= _SQRT2
    m = np.where(big, m * 0.5, m)
    e = e + big
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    p = np.full_like(s, _ATANH[0])
    for c in _ATANH[1:]:
        p = p * s2 + c
    lm = (s + s) * p
    de = e.astype(np.float64)
    return de * _LN2_HI + (lm + de * _LN2_LO)


def _poly(coef, f2):
    p = np.full_like(f2, coef[0])
    for c in coef[1:]:
        p = p * f2 + c
    return p


def cos_sin_turn(m2):
    """cos and sin of 2 pi u2, u2 = m2 2^-53: quadrant k and reduced quarter turn f in [-1/2, 1/2) split exactly."""
    k = (m2 + np.uint64(1 << 50)) >> np.uint64(51)
    f = (m2.astype(np.int64) - (k << np.uint64(51)).astype(np.int64)).astype(np.float64) * 2.0 ** -51
    f2 = f * f
    s = f * _poly(_SIN, f2)
    c = _poly(_COS, f2)
    q = (k & np.uint64(3)).astype(np.int64)
    cz = np.select([q == 0, q == 1, q == 2], [c, -s, -c], s)
    sz = np.select([q == 0, q == 1, q == 2], [s, c, -s], -c)
    return cz, sz


def box_muller(x, y, z, w):
    u1, m2 = uniforms(x, y, z, w)
    r = np.sqrt(-2.0 * ln_unit(u1))
    cz, sz = cos_sin_turn(m2)
    return r * cz, r * sz


def normal_fill(events, stream0, n_streams, n, seed, rank, scale=1.0):
    """float64 [len(events)][n_streams][n]: what rlx_normal_fill writes for these event indices."""
    ev = np.asarray(events, dtype=np.uint64).reshape(-1)
    pairs = (n + 1) // 2
    p = np.arange(pairs, dtype=np.uint64)[None, None, :]
    s = (stream0 + np.arange(n_streams, dtype=np.uint64))[None, :, None]
    lo = (ev & _M32)[:, None, None]
    hi = ((ev >> np.uint64(32)) ^ np.uint64(NOISE_TAG))[:, None, None]
    shape = (ev.size, n_streams, pairs)
    words = philox4x32_10(np.broadcast_to(p, shape), np.broadcast_to(s, shape), np.broadcast_to(lo, shape),
                          np.broadcast_to(hi, shape), seed, rank)
    z0, z1 = box_muller(*words)
    out = np.empty((ev.size, n_streams, 2 * pairs))
    out[..., 0::2] = z0 * scale
    out[..., 1::2] = z1 * scale
    return out[..., :n]
