"""The exploration kernels of csrc/explore.hip, each called by name on inputs that sit on its decision boundaries, against
oracle/explore.py -- numpy's own cumsum / searchsorted, isclose / argmax and float64 arithmetic.  The results are integers
or float64-evaluated, so every assertion is an equality; the one exception is the probabilities that
rlx_softmax_categorical_sample returns, held to the counted bound of tests/head_loss_ref.softmax.  Every launch covers all
its envs at once; pitched inputs carry NaN in their padding columns, pitched outputs a sentinel."""
import numpy as np
import pytest

import head_loss_ref as R
from coach_amd._rlx import RlxError
from oracle import explore as E

F32, F64 = np.float32, np.float64
SENT = F32(-777.25)
WIDTHS = [1, 2, 6, 18]


def _d(x, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _h(t):
    return t.cpu().numpy()


def _ints(n, dev):
    return _d(np.full(n, -7, dtype=np.int32), dev)


def _pitched(a, ld):
    out = np.full((a.shape[0], ld), np.nan, dtype=F32)
    out[:, :a.shape[1]] = a
    return out


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


# ------------------------------------------------------------------------------------------------ categorical draws
def _cdf(p):
    """the cdf np.random.choice builds (numpy mtrand.pyx): p.astype(float64).cumsum(), divided by its last entry"""
    cdf = np.asarray(p, dtype=F64).cumsum(axis=-1)
    return cdf / cdf[..., -1:]


def _prob_rows(n_env, A, rng):
    """random rows, and in turn: leading zeros, trailing zeros, un-normalised (sum 0.5, sum 3), one-hot"""
    p = rng.dirichlet(np.ones(A), n_env)
    k = np.arange(n_env)
    if A >= 3:
        p[k % 6 == 1, :A // 3] = 0
        p[k % 6 == 2, -(A // 3):] = 0
    p = p / p.sum(axis=1, keepdims=True)
    p[k % 6 == 3] *= 0.5
    p[k % 6 == 4] *= 3.0
    hot = k % 6 == 5
    p[hot] = np.eye(A)[rng.randint(0, A, n_env)][hot]
    return p.astype(F32)


def _uniform_variants(p, rng):
    """[(name, u [n_env])]: 0, the largest double below 1, every cdf[j] exactly, the double just below every cdf[j], random"""
    n_env, A = p.shape
    cdf = _cdf(p)
    out = [("zero", np.zeros(n_env)), ("below_one", np.full(n_env, np.nextafter(1.0, 0.0)))]
    for j in range(A):
        out.append(("cdf[%d]" % j, cdf[:, j].copy()))
        out.append(("below_cdf[%d]" % j, np.maximum(np.nextafter(cdf[:, j], 0.0), 0.0)))
    out.append(("random", rng.random_sample(n_env)))
    return out


def _expected_choice(p, u, A):
    """oracle.explore.categorical_choice; searchsorted(side='right') answers A where u reaches the last cdf entry, 1.0 --
    no np.random draw does, and the kernel clamps it to A - 1"""
    want = np.empty(len(u), dtype=np.int32)
    for e in range(len(u)):
        a = E.categorical_choice(p[e], u[e])
        if a == A:
            assert u[e] == 1.0
            a = A - 1
        want[e] = a
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("A", WIDTHS)
@pytest.mark.parametrize("n_env", [1, 63, 64, 65, 130])
def test_categorical_sample(rlx, dev, n_env, A, pad):
    """rlx_categorical_sample == np.random.choice's searchsorted(side='right') on the float64 cdf, for u = 0, the largest
    double below 1, every cdf[j] EXACTLY (the answer is then j + 1: `u < cdf[j]` is strict; A - 1 by the kernel's clamp when
    cdf[j] is 1) and the double just below it (the answer is at most j), and random draws; probability rows with leading
    and trailing zeros, sums of 0.5 and 3, and one-hot rows."""
    rng = np.random.RandomState(n_env * 64 + A * 2 + pad)
    p = _prob_rows(n_env, A, rng)
    pd = _d(_pitched(p, A + pad), dev)
    cdf = _cdf(p)
    for name, u in _uniform_variants(p, rng):
        acts = _ints(n_env, dev)
        rlx.categorical_sample(pd, A + pad, _d(u, dev), n_env, A, acts, 0)
        want = _expected_choice(p, u, A)
        got = _h(acts)
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:5], got[got != want][:5], want[got != want][:5])
        if name.startswith("cdf["):
            j = int(name[4:-1])
            assert np.all((want > j) | (cdf[:, j] == 1.0))
        if name.startswith("below_cdf["):
            assert np.all((want <= int(name[10:-1])) | (cdf[:, int(name[10:-1])] == 0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("spread", [1.0, 80.0])
@pytest.mark.parametrize("A", WIDTHS)
@pytest.mark.parametrize("n_env", [1, 63, 64, 65, 130])
def test_softmax_categorical_sample(rlx, dev, n_env, A, spread):
    """rlx_softmax_categorical_sample: probs_out against the float64 softmax at head_loss_ref.softmax's counted bound
    (logits spread over +-1 and +-80), with ld = A + 3 (NaN) and ld_out = A + 2 (sentinel kept); the action equals
    oracle.explore.categorical_choice on the kernel's OWN fp32 probabilities, for u = 0, just below 1, random, and -- in a
    second round of launches -- exactly on and just below every entry of the cdf of those probabilities; probs_out = NULL
    gives the same actions."""
    rng = np.random.RandomState(n_env * 64 + A)
    z = rng.uniform(-spread, spread, (n_env, A)).astype(F32)
    z[0, 0], z[0, -1] = spread, -spread
    zd = _d(_pitched(z, A + 3), dev)
    ref, units = R.softmax(z)

    def launch(u, with_probs):
        acts = _ints(n_env, dev)
        probs = _d(np.full((n_env, A + 2), SENT, dtype=F32), dev) if with_probs else None
        rlx.softmax_categorical_sample(zd, A + 3, _d(u, dev), n_env, A, probs, A + 2, acts, 0)
        return _h(acts), (None if probs is None else _h(probs))

    _, probs = launch(rng.random_sample(n_env), True)
    p = probs[:, :A]
    assert np.array_equal(_bits(probs[:, A:]), _bits(np.full((n_env, 2), SENT, dtype=F32)))
    err = np.abs(p.astype(F64) - ref)
    assert np.all(np.isfinite(p)) and np.all(err <= R.U24 * units), (err / (R.U24 * units)).max()
    for name, u in _uniform_variants(p, rng):
        want = _expected_choice(p, u, A)
        got, again = launch(u, True)
        assert np.array_equal(_bits(again), _bits(probs)), name
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:5])
        alone, none = launch(u, False)
        assert none is None and np.array_equal(alone, want), name


# ------------------------------------------------------------------------------------------------ rlx_egreedy
def _step_to_boundary(mx):
    """(inside, outside): the fp32 value below mx that np.isclose(x, mx) still accepts -- |x - mx| <= 1e-8 + 1e-5 |mx| as
    numpy evaluates it on fp32 operands -- and the next fp32 value below it, which it rejects"""
    mx = F32(mx)
    with np.errstate(all="ignore"):
        x = F32(mx - (F32(1e-8) + F32(1e-5) * np.abs(mx)))
        while not np.isclose(x, mx):
            x = np.nextafter(x, mx)
        while np.isclose(np.nextafter(x, F32(-np.inf)), mx):
            x = np.nextafter(x, F32(-np.inf))
    out = np.nextafter(x, F32(-np.inf))
    assert x < mx and np.isclose(x, mx) and not np.isclose(out, mx)
    return x, out


EGREEDY_KINDS = ["random", "duplicates", "inside", "outside", "tie_zero", "u_equals_eps", "explores", "inf", "minus_inf", "nan",
                 "nan_first"]


def _egreedy_case(n_env, A, eps, rng):
    q = rng.randn(n_env, A).astype(F32)
    u = rng.uniform(0.31, 1.0, n_env)                        # greedy for eps 0.3 unless a kind says otherwise
    tie = rng.random_sample((n_env, A))
    ra = np.full(n_env, 12345, dtype=np.int32)               # must never come out of a greedy env
    kinds = np.array(EGREEDY_KINDS)[np.arange(n_env) % len(EGREEDY_KINDS)]
    maxima = [1000.0, -1000.0, 1e-3, 0.0]
    for e, kind in enumerate(kinds):
        top = rng.randint(0, A)
        mx = F32(maxima[e % 4])
        inside, outside = _step_to_boundary(mx)
        if kind == "duplicates":
            q[e, rng.randint(0, A, 3)] = q[e].max() + F32(1)
        elif kind in ("inside", "outside") and A >= 2:
            other = (top + 1 + rng.randint(0, A - 1)) % A
            q[e] = np.minimum(q[e], 0) + mx - F32(abs(float(mx)) + 1.0)
            q[e, top], q[e, other] = mx, (inside if kind == "inside" else outside)
            tie[e, top], tie[e, other] = 0.25, 0.75          # the other entry wins exactly when it is close
        elif kind == "tie_zero":
            tie[e, q[e].argmax()] = 0.0                      # every product is 0: argmax answers 0
        elif kind == "u_equals_eps":
            u[e] = eps                                       # `<` is strict: greedy
        elif kind == "explores":
            u[e], ra[e] = 0.0, rng.randint(0, A)
        elif kind == "inf" and A >= 3:
            q[e] = 1.0
            q[e, [A - 2, A - 1]] = np.inf                    # [1, ..., inf, inf]
        elif kind == "minus_inf":
            q[e] = -np.inf
        elif kind == "nan" and A >= 2:
            q[e, A // 2] = np.nan                            # [1, nan, 3]: max is NaN, nothing is close, argmax 0
            q[e, -1] = q[e, 0] + F32(2)
        elif kind == "nan_first":
            q[e, 0] = np.nan
    return q, u, ra, tie, kinds


@pytest.mark.gpu
@pytest.mark.parametrize("eps", [0.3, 0.0, 1.0])
@pytest.mark.parametrize("A", [1, 3, 6, 18])
@pytest.mark.parametrize("n_env", [1, 63, 64, 65, 200])
def test_egreedy(rlx, dev, n_env, A, eps):
    """rlx_egreedy, ONE launch for all envs, q with ld = A + 3 (NaN padding), == oracle.explore.egreedy_choice (numpy's own
    isclose and argmax) env by env: exact duplicates of the maximum; an entry one fp32 step inside and one step outside
    isclose's 1e-8 + 1e-5 |max| at max = 1000, -1000, 1e-3 and 0, holding the larger tie draw; a tie draw of exactly 0 on
    the only close entry; explore_u == epsilon (greedy: the test is `<`); epsilon 0 and 1; random_act honoured on
    exploring envs only (greedy envs carry 12345 there); rows [1, .., inf, inf], all -inf, and with a NaN."""
    rng = np.random.RandomState(n_env * 64 + A)
    q, u, ra, tie, kinds = _egreedy_case(n_env, A, eps, rng)
    if eps == 1.0:
        ra = rng.randint(0, A, n_env).astype(np.int32)       # every env explores (u < 1)
    acts = _ints(n_env, dev)
    rlx.egreedy(_d(_pitched(q, A + 3), dev), A + 3, _d(u, dev), _d(ra, dev), _d(tie, dev), float(eps), n_env, A, acts, 0)
    with np.errstate(all="ignore"):
        want = np.array([E.egreedy_choice(q[e], u[e], ra[e], tie[e], eps) for e in range(n_env)], dtype=np.int32)
    got = _h(acts)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(e), kinds[e], q[e].tolist(), int(got[e]), int(want[e])) for e in bad[:4]]
    explores = u < eps
    assert np.array_equal(want[explores], ra[explores]) and np.all((want[~explores] >= 0) & (want[~explores] < A))
    if eps == 0.3 and A >= 3:                                # the cases are what their names say (conditions on the inputs)
        for e in range(min(n_env, len(EGREEDY_KINDS))):
            with np.errstate(all="ignore"):
                close = np.isclose(q[e], q[e].max())
            if kinds[e] == "inside":
                assert close.sum() == 2 and want[e] == np.flatnonzero(tie[e] == 0.75)[0]
            elif kinds[e] == "outside":
                assert close.sum() == 1 and want[e] == np.flatnonzero(tie[e] == 0.25)[0]
            elif kinds[e] == "inf":
                assert close.tolist() == [False] * (A - 2) + [True, True] and want[e] >= A - 2
            elif kinds[e] == "minus_inf":
                assert close.all() and want[e] == tie[e].argmax()
            elif kinds[e] in ("nan", "nan_first"):
                assert not close.any() and want[e] == 0
            elif kinds[e] == "u_equals_eps":
                assert u[e] == eps and want[e] != 12345
            elif kinds[e] == "explores":
                assert want[e] == ra[e]


# ------------------------------------------------------------------------------------------------ rlx_argmax_rows
@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n_cols", WIDTHS)
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65])
def test_argmax_rows(rlx, dev, n_rows, n_cols, pad):
    """rlx_argmax_rows == np.argmax row by row: ties (the first index wins), +0 against -0 in both orders (equal: the
    first), a NaN in column 0 and in a later column (numpy answers the first NaN), rows of -inf, -inf next to a finite
    value; ld = n_cols and n_cols + 3 with NaN padding."""
    rng = np.random.RandomState(n_rows * 64 + n_cols)
    v = rng.randn(n_rows, n_cols).astype(F32)
    for r in range(n_rows):
        kind = r % 9
        hi = v[r].max() + F32(1)
        if kind == 1:
            v[r, rng.randint(0, n_cols, 3)] = hi                       # ties
        elif kind == 2:
            v[r] = -np.abs(v[r]) - 1
            v[r, 0], v[r, -1] = 0.0, -0.0
        elif kind == 3:
            v[r] = -np.abs(v[r]) - 1
            v[r, 0], v[r, -1] = -0.0, 0.0
        elif kind == 4:
            v[r, 0] = np.nan
        elif kind == 5:
            v[r, -1] = np.nan
            v[r, n_cols // 2] = np.nan
        elif kind == 6:
            v[r] = -np.inf
        elif kind == 7:
            v[r] = -np.inf
            v[r, -1] = -3.0
        elif kind == 8:
            v[r] = hi                                                  # all equal
    out = _ints(n_rows, dev)
    rlx.argmax_rows(_d(_pitched(v, n_cols + pad), dev), n_cols + pad, n_rows, n_cols, out, 0)
    want = np.argmax(v, axis=1).astype(np.int32)
    got = _h(out)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(r), v[r].tolist(), int(got[r]), int(want[r])) for r in bad[:4]]
    if n_rows >= 9 and n_cols >= 2:                                    # numpy's rule is what the docstring says
        assert want[2] == 0 and want[3] == 0 and want[4] == 0 and want[5] == n_cols // 2 and want[6] == 0 and \
            want[7] == n_cols - 1 and want[8] == 0


# ------------------------------------------------------------------------------------------------ rlx_gaussian_action
@pytest.mark.gpu
@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("n_env,D", [(1, 1), (85, 3), (64, 4), (257, 1), (1, 257)])
def test_gaussian_action(rlx, dev, n_env, D, per_sample, bounded):
    """rlx_gaussian_action == float32(oracle.explore.gaussian_action) BIT FOR BIT (the kernel evaluates mean + std * z and
    the clip in float64, csrc/explore.hip is built without contraction, and the cast rounds once): per-dimension and
    per-sample std, with and without bounds, 1 / 255 / 256 / 257 elements (one block is 256 threads), a dimension with
    low == high, draws of |z| = 40."""
    rng = np.random.RandomState(n_env * 8 + D + 2 * per_sample + bounded)
    mean = rng.randn(n_env, D).astype(F32)
    std = rng.uniform(0.05, 2.0, (n_env, D) if per_sample else D).astype(F32)
    z = rng.standard_normal((n_env, D))
    z.reshape(-1)[::7] = 40.0
    z.reshape(-1)[3::11] = -40.0
    low = -rng.uniform(0.5, 2.0, D).astype(F32)
    high = rng.uniform(0.5, 2.0, D).astype(F32)
    low[-1] = high[-1] = F32(0.3)                                       # low == high
    out = _d(np.full((n_env, D), SENT, dtype=F32), dev)
    rlx.gaussian_action(_d(mean, dev), None if per_sample else _d(std, dev), _d(std, dev) if per_sample else None, _d(z, dev),
                        _d(low, dev) if bounded else None, _d(high, dev) if bounded else None, n_env, D, out, 0)
    want = E.gaussian_action(mean, std, z, low if bounded else None, high if bounded else None).astype(F32)
    got = _h(out)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (bad.sum(), got[bad][:4], want[bad][:4])
    if bounded:
        assert np.all(got[:, -1] == F32(0.3)) and np.all(got >= low) and np.all(got <= high)
    else:
        assert np.abs(got).max() > 2.0 or n_env * D == 1


@pytest.mark.gpu
@pytest.mark.parametrize("per_sample", [False, True])
def test_gaussian_action_keeps_a_nan_mean(rlx, dev, per_sample):
    """np.clip keeps a NaN (clip_action_to_space, spaces.py:379): a diverged actor's NaN mean, a NaN std and a NaN draw
    come out as NaN and not as the lower bound; every other element keeps the bits of the run without them"""
    n_env, D = 5, 3
    rng = np.random.RandomState(per_sample)
    mean = rng.randn(n_env, D).astype(F32)
    std = rng.uniform(0.05, 2.0, (n_env, D) if per_sample else D).astype(F32)
    z = rng.standard_normal((n_env, D))
    low, high = -rng.uniform(0.5, 2.0, D).astype(F32), rng.uniform(0.5, 2.0, D).astype(F32)
    clean = E.gaussian_action(mean, std, z, low, high).astype(F32)
    mean[1, 2] = np.nan
    z[3, 0] = np.nan
    z[4, 1] = 40.0
    want = E.gaussian_action(mean, std, z, low, high).astype(F32)
    isnan = np.zeros((n_env, D), dtype=bool)
    isnan[1, 2] = isnan[3, 0] = True
    assert np.array_equal(np.isnan(want), isnan) and want[4, 1] == high[1]
    out = _d(np.full((n_env, D), SENT, dtype=F32), dev)
    rlx.gaussian_action(_d(mean, dev), None if per_sample else _d(std, dev), _d(std, dev) if per_sample else None, _d(z, dev),
                        _d(low, dev), _d(high, dev), n_env, D, out, 0)
    got = _h(out)
    assert np.array_equal(np.isnan(got), isnan), got
    assert np.array_equal(_bits(got[~isnan]), _bits(want[~isnan]))
    keep = ~isnan
    keep[4, 1] = False
    assert np.array_equal(_bits(got[keep]), _bits(clean[keep]))


@pytest.mark.gpu
def test_gaussian_action_needs_both_bounds_or_neither(rlx, dev):
    x, z = _d(np.zeros((4, 2), dtype=F32), dev), _d(np.zeros((4, 2)), dev)
    std, bound = _d(np.ones(2, dtype=F32), dev), _d(np.ones(2, dtype=F32), dev)
    out = _d(np.zeros((4, 2), dtype=F32), dev)
    with pytest.raises(RlxError):
        rlx.gaussian_action(x, std, None, z, bound, None, 4, 2, out, 0)
    with pytest.raises(RlxError):
        rlx.gaussian_action(x, std, None, z, None, bound, 4, 2, out, 0)
