"""The device noise generator's CPU side (noise_source = "device"): the numpy twin tests/noise_ref.py of
csrc/noise.hip is a standard normal generator (distribution, independence of lags / streams / ranks / events), its
Box-Muller transform agrees with a high-precision one on the same uniforms, its streams never meet the synthetic
environment's, and the C ABI / agent parameter reject bad values before any device work.  Deterministic: no flakes."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_ref as R  # noqa: E402


def _big_sample():
    # 2^22 values: 64 events x 2^16 of stream 0, seed 7, rank 0
    return R.normal_fill(np.arange(64), 0, 1, 1 << 16, 7, 0).ravel()


def test_distribution_is_standard_normal():
    from scipy import stats
    z = _big_sample()
    n = z.size
    assert n == 1 << 22
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / n)
    ks = stats.kstest(z, "norm")
    assert ks.statistic < 1.95 / np.sqrt(n), ks                     # (1.95 / sqrt n: the 0.1 % point of the KS law)
    for k in (3.0, 4.0):
        p = 2 * stats.norm.sf(k)
        frac = np.mean(np.abs(z) > k)
        assert abs(frac - p) < 5 * np.sqrt(p * (1 - p) / n), (k, frac, p)
    assert np.isfinite(z).all()


def _corr_ok(a, b):
    a, b = a - a.mean(), b - b.mean()
    c = float(np.dot(a, b) / np.sqrt(np.dot(a, a) * np.dot(b, b)))
    assert abs(c) < 5 / np.sqrt(a.size), c


def test_no_correlation_across_lags_streams_ranks_events():
    n = 1 << 18
    base = R.normal_fill([5], 0, 5, n, 7, 0)[0]                      # five streams of one event
    _corr_ok(base[0][:-1], base[0][1:])                              # lag 1 (within and across pairs)
    _corr_ok(base[0][0::2], base[0][1::2])                           # the two halves of every Box-Muller pair
    for s in range(1, 5):
        _corr_ok(base[0], base[s])                                   # streams
    _corr_ok(base[0], R.normal_fill([5], 0, 1, n, 7, 1)[0, 0])       # ranks
    _corr_ok(base[0], R.normal_fill([6], 0, 1, n, 7, 0)[0, 0])       # consecutive events
    _corr_ok(base[0], R.normal_fill([5 + (1 << 32)], 0, 1, n, 7, 0)[0, 0])   # events that share the low word
    _corr_ok(base[0], R.normal_fill([5], 0, 1, n, 8, 0)[0, 0])       # seeds


def test_streams_never_meet_the_synthetic_environment():
    """Key (seed, rank) of the noise against key (seed, env id) of csrc/synth_env.hip with seed = seed and env id = rank:
    the counters differ in their last word (synth_env: the stream, 0 or 1; noise: event high word ^ tag), so no output
    block of one is ever an output block of the other.  Checked on the words themselves too."""
    from oracle.synth_env import philox4x32_10 as synth_philox
    seed, rank = 9, 3
    # noise counters: pairs 0..255, streams 0..4, events 0..63 and near 2^32
    p, s, ev = np.meshgrid(np.arange(256, dtype=np.uint64), np.arange(5, dtype=np.uint64),
                           np.r_[np.arange(64), (1 << 32) - 1, 1 << 32].astype(np.uint64), indexing="ij")
    c3 = (ev >> np.uint64(32)) ^ np.uint64(R.NOISE_TAG)
    assert not np.isin(c3, [0, 1]).any()
    nw = np.stack(R.philox4x32_10(p, s, ev & np.uint64(0xFFFFFFFF), c3, seed, rank), -1).reshape(-1, 4)
    # synthetic environment blocks of env `rank`: episodes 0..15, steps 0..63, blocks 0..31, streams 0 / 1
    e, t, j, st = np.meshgrid(np.arange(16), np.arange(64), np.arange(32), np.arange(2), indexing="ij")
    sw = synth_philox(e.ravel().astype(np.uint32), t.ravel().astype(np.uint32), j.ravel().astype(np.uint32),
                      st.ravel().astype(np.uint32), np.uint32(seed), np.uint32(rank))
    sw = np.stack([np.asarray(w, dtype=np.uint64) for w in sw], -1).reshape(-1, 4)
    key = lambda w: (w[:, 0] << np.uint64(32) | w[:, 1]) * np.uint64(0x9E3779B97F4A7C15) ^ (w[:, 2] << np.uint64(32) | w[:, 3])
    assert not np.isin(key(nw), key(sw)).any()


def test_transform_matches_high_precision_box_muller():
    """10^6 pairs: the twin's z0 / z1 against sqrt(-2 ln u1) (cos, sin)(2 pi u2) evaluated in 72-bit arithmetic on the
    same uniforms, |dz| <= 4 ulp of r (relative to r: z passes through zero)."""
    from mpmath import libmp as L
    n = 10 ** 6
    w = R.philox4x32_10(np.arange(n, dtype=np.uint64), 2, 3, R.NOISE_TAG, 7, 0)
    u1, m2 = R.uniforms(*w)
    z0, z1 = R.box_muller(*w)
    prec, rnd = 72, L.round_nearest
    m2_, u1_ = m2.tolist(), u1.tolist()
    r_ref, c_ref, s_ref = np.empty(n), np.empty(n), np.empty(n)
    minus2 = L.from_int(-2)
    for i in range(n):
        r = L.mpf_sqrt(L.mpf_mul(L.mpf_log(L.from_float(u1_[i]), prec, rnd), minus2, prec, rnd), prec, rnd)
        c, s = L.mpf_cos_sin_pi(L.from_man_exp(m2_[i], -52), prec, rnd)          # pi m2 2^-52 = 2 pi u2
        r_ref[i] = L.to_float(r)
        c_ref[i] = L.to_float(L.mpf_sub(L.mpf_mul(r, c, prec, rnd), L.from_float(float(z0[i])), prec, rnd))
        s_ref[i] = L.to_float(L.mpf_sub(L.mpf_mul(r, s, prec, rnd), L.from_float(float(z1[i])), prec, rnd))
    ulp = np.spacing(np.maximum(r_ref, np.finfo(np.float64).tiny))
    worst = max(np.max(np.abs(c_ref) / ulp), np.max(np.abs(s_ref) / ulp))
    assert worst <= 4.0, worst
    assert u1.min() > 0 and u1.max() <= 1.0 and m2.max() < 1 << 53


def test_pinned_values():
    np.testing.assert_array_equal(R.normal_fill([0], 0, 1, 4, 0, 0)[0, 0],
                                  [0.265621850532413, -0.9914590564650066, -1.1945540077668118, -1.2104790599177293])
    np.testing.assert_array_equal(R.normal_fill([7, 1 << 40], 1, 3, 3, 11, 2, 0.2)[:, :, 1],
                                  [[0.05207624778850544, 0.25752952490114195, -0.0405087337830266],
                                   [-0.0698451888259609, -0.09154891435728697, -0.1874857324348303]])
    np.testing.assert_array_equal(R.normal_fill([(1 << 32) - 1], 4, 1, 5, 0xFFFFFFFF, 0)[0, 0],
                                  [-0.5810562281725523, -1.2610273922664164, -0.5727300821695482, -0.2800604612345248,
                                   -0.32177613905907854])


def test_layout_and_scale():
    a = R.normal_fill([3, 4], 1, 3, 7, 5, 0)
    assert a.shape == (2, 3, 7)
    np.testing.assert_array_equal(a[1, 2], R.normal_fill([4], 3, 1, 7, 5, 0)[0, 0])     # out[event][stream][n]
    np.testing.assert_array_equal(a[0, 0, :6], R.normal_fill([3], 1, 1, 6, 5, 0)[0, 0])   # a prefix of a longer fill
    np.testing.assert_array_equal(R.normal_fill([3], 1, 1, 7, 5, 0, 0.2)[0, 0], 0.2 * a[0, 0])


def test_normal_fill_is_declared_exported_and_validates():
    from coach_amd import _rlx
    lib = _rlx.lib()
    assert "rlx_normal_fill" in _rlx.parse_header()
    assert lib.raw("rlx_abi_version")() == 11 == _rlx.ABI_VERSION
    fake = ctypes.c_void_p(0x1000)            # never dereferenced: validation fails first
    with pytest.raises(_rlx.RlxError, match="null pointer"):
        lib.normal_fill(None, fake, 1, 0, 1, 8, 0, 0, 1.0, None)
    with pytest.raises(_rlx.RlxError, match="null pointer"):
        lib.normal_fill(fake, None, 1, 0, 1, 8, 0, 0, 1.0, None)
    for n, n_events in ((0, 1), (-3, 1), (8, 0)):
        with pytest.raises(_rlx.RlxError, match="bad sizes"):
            lib.normal_fill(fake, fake, n_events, 0, 1, n, 0, 0, 1.0, None)
    for s0, ns in ((-1, 1), (0, 0), (4, 2), (5, 1), (0, 6)):
        with pytest.raises(_rlx.RlxError, match="bad stream range"):
            lib.normal_fill(fake, fake, 1, s0, ns, 8, 0, 0, 1.0, None)


@pytest.mark.parametrize("agent", ["td3", "sac"])
def test_bogus_noise_source_raises_before_device_work(agent):
    if agent == "td3":
        from coach_amd.agents.td3_agent import TD3Agent as C, TD3AgentParameters as P
    else:
        from coach_amd.agents.soft_actor_critic_agent import SoftActorCriticAgent as C, \
            SoftActorCriticAgentParameters as P
    p = P()
    assert p.algorithm.noise_source is None
    p.algorithm.noise_source = "bogus"
    with pytest.raises(ValueError, match="noise_source"):
        C(p, None, device="cpu")                  # no environment, no device: the check comes first


def test_noise_source_default_follows_the_class_attribute():
    from coach_amd.agents.td3_agent import TD3AgentParameters
    from coach_amd.agents.vector_agent import VectorOffPolicyAgent
    assert VectorOffPolicyAgent.NOISE_SOURCE == "host"

    class Probe(VectorOffPolicyAgent):
        def __init__(self, ap):
            self.ap = ap
    p = TD3AgentParameters()
    assert Probe(p)._resolve_noise_source() == "host"
    try:
        VectorOffPolicyAgent.NOISE_SOURCE = "device"
        assert Probe(p)._resolve_noise_source() == "device"
        p.algorithm.noise_source = "host"
        assert Probe(p)._resolve_noise_source() == "host"
    finally:
        VectorOffPolicyAgent.NOISE_SOURCE = "host"
