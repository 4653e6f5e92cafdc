"""The head-loss kernels of csrc/losses.hip, each called by name at the batch sizes where its code path changes (one
wave, the block size stepping at 64, the 1024-thread cap where the stride loop starts), with pitched buffers and every
optional argument on and off, against the float64 restatement tests/head_loss_ref.py.

Every comparison is either bit for bit or |got - float64| <= 2^-24 * units, `units` being the bound head_loss_ref counts
from the kernel's chain of fp32 operations (see its docstrings; nothing here is measured).  Inputs with a pitch carry NaN in
their padding columns, outputs a sentinel that must come back unchanged.  Every test prints the largest share of its
bound that it used (`pytest -s`) before it asserts."""
import functools

import numpy as np
import pytest

import head_loss_ref as R
from coach_amd._rlx import RlxError

F32, F64 = np.float32, np.float64
U24 = R.U24
SENT = F32(-777.25)
PAD = 5
BATCHES = [1, 63, 64, 65, 1024, 1025, 2049]
SMALL_BATCHES = [1, 65, 1024]
WIDTHS = [1, 2, 6, 18]


def _d(x, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _h(t):
    return t.cpu().numpy()


def _sent(shape, dev):
    return _d(np.full(shape, SENT, dtype=F32), dev)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


def _same_bits(got, want, what):
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: got %r want %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def _within(got, ref, units, what):
    """|got - ref| <= 2^-24 units, element by element; where units is 0 the value is owed exactly"""
    got, ref, units = np.asarray(got, dtype=F32).astype(F64), np.asarray(ref, dtype=F64), np.asarray(units, dtype=F64)
    assert got.shape == ref.shape == units.shape, (what, got.shape, ref.shape, units.shape)
    assert np.all(np.isfinite(got)), what
    err = np.abs(got - ref)
    share = np.where(err > 0, err / np.maximum(U24 * units, 1e-300), 0.0)
    print("SHARE %s %.3f" % (what, share.max() if share.size else 0.0))
    assert np.all(err <= U24 * units), "%s: %.3f of the counted bound at %s (got %r, float64 %r)" % (
        what, share.max(), np.unravel_index(share.argmax(), share.shape), got.reshape(-1)[share.argmax()],
        ref.reshape(-1)[share.argmax()])


def _pitched(a, ld):
    """[B, n] -> [B, ld] with NaN in the padding columns"""
    out = np.full((a.shape[0], ld), np.nan, dtype=F32)
    out[:, :a.shape[1]] = a
    return out


def _pad_untouched(buf, n, what):
    if buf.shape[1] > n:
        _same_bits(buf[:, n:], np.full((buf.shape[0], buf.shape[1] - n), SENT, dtype=F32), what + ": padding columns")


# ------------------------------------------------------------------------------------------------ rlx_regression_loss
@functools.lru_cache(maxsize=None)
def _regression_case(B, D):
    out, target, w = R.huber_case(np.random.RandomState(B * 32 + D), B, D)
    refs = {(kind, weighted, lw, gs): R.regression_loss(out, target, w if weighted else None, kind, lw, gs)
            for kind in ("mse", "huber") for weighted, lw, gs in ((True, 1.0, 1.0), (False, 1.0, 1.0), (True, 0.5, 0.75))}
    return out, target, w, refs


def _run_regression(rlx, dev, out, target, w, B, D, kind, lw, gs, pad, want_grad=True, want_loss=True):
    ld = D + pad
    g = _sent((B, ld), dev) if want_grad else None
    l = _sent((1,), dev) if want_loss else None
    rlx.regression_loss(_d(_pitched(out, ld), dev), ld, _d(_pitched(target, ld), dev), ld, None if w is None else _d(w, dev),
                        B, D, {"mse": 0, "huber": 1}[kind], lw, gs, g, ld, l, 0)
    return (None if g is None else _h(g)), (None if l is None else _h(l))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mse", "huber"])
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("B", BATCHES)
def test_regression_loss(rlx, dev, B, D, kind):
    """loss and gradient against head_loss_ref.regression_loss at its counted bounds (loss: (D + 6 + sum_depth(B)) units of
    mean |w| row; gradient: 5 units), on head_loss_ref.huber_case -- errors of exactly +-1, one fp32 step inside and
    outside, and 0 on the first elements --, contiguous and with ld = D + 5 on out, target and grad (NaN / sentinel
    padding), importance weights on and off, loss_weight 0.5 with grad_scale 0.75, and each output alone (bit for bit what
    the joint launch wrote)."""
    out, target, w, refs = _regression_case(B, D)
    for weighted, lw, gs in ((True, 1.0, 1.0), (False, 1.0, 1.0), (True, 0.5, 0.75)):
        ref = refs[(kind, weighted, lw, gs)]
        for pad in (0, PAD):
            tag = "regression[%d,%d,%s,w%d,lw%g,pad%d]" % (B, D, kind, weighted, lw, pad)
            g, l = _run_regression(rlx, dev, out, target, w if weighted else None, B, D, kind, lw, gs, pad)
            _pad_untouched(g, D, tag)
            _within(g[:, :D], ref["grad"], ref["grad_units"], tag + " grad")
            _within(l, [ref["loss"]], [ref["loss_units"]], tag + " loss")
            if weighted and pad:
                g1, none = _run_regression(rlx, dev, out, target, w, B, D, kind, lw, gs, pad, want_loss=False)
                assert none is None
                _same_bits(g1, g, tag + " grad alone")
                none, l1 = _run_regression(rlx, dev, out, target, w, B, D, kind, lw, gs, pad, want_grad=False)
                assert none is None
                _same_bits(l1, l, tag + " loss alone")
    if kind == "huber" and B in (1, 64, 1024):
        # the planted edges: the gradient factor is the error itself up to |e| = 1 and +-1 beyond, exactly (grad_scale = B,
        # a power of two: the product with it and the division by B are exact)
        k = min(B * D, len(R.HUBER_EDGES))
        g, _ = _run_regression(rlx, dev, out, target, None, B, D, kind, 1.0, float(B), 0, want_loss=False)
        _same_bits(g.reshape(-1)[:k], np.clip(np.array(R.HUBER_EDGES[:k], dtype=F32), F32(-1), F32(1)), "huber edges")


# ------------------------------------------------------------------------------------------------ rlx_softmax
def _softmax_rows(B, n, spread, seed):
    rng = np.random.RandomState(seed)
    z = rng.uniform(-spread, spread, (B, n)).astype(F32)
    z[0, 0], z[0, -1] = spread, -spread                    # both ends in one row (one value when n = 1)
    k = np.arange(B)
    z[k % 5 == 1] = F32(rng.uniform(-spread, spread))      # all-equal rows
    if n > 1:
        z[k % 5 == 2, 1:] = -np.inf                        # -inf next to a finite maximum
        z[k % 5 == 3, 0] = -np.inf
    return z


@pytest.mark.gpu
@pytest.mark.parametrize("spread", [1.0, 80.0, 1e4])
@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("B", [1, 63, 64, 65, 129])
def test_softmax(rlx, dev, B, n, spread):
    """rlx_softmax on rows spread over +-1, +-80 and +-1e4 (a softmax without the maximum subtracted overflows from 89
    on), all-equal rows, rows with -inf next to a finite maximum, n = 1; contiguous and pitched (NaN / sentinel padding).
    Every result is finite and within head_loss_ref.softmax's counted bound (|d_j| + sum_k p_k |d_k| + 2 EXPF + n units of
    p_j, floored at the smallest normal number); every row sums to 1 within (n + 2) 2^-24."""
    z = _softmax_rows(B, n, spread, B * 64 + n)
    p, units = R.softmax(z)
    for pad in (0, PAD):
        tag = "softmax[%d,%d,%g,pad%d]" % (B, n, spread, pad)
        out = _sent((B, n + pad), dev)
        rlx.softmax(_d(_pitched(z, n + pad), dev), n + pad, B, n, out, n + pad, 0)
        got = _h(out)
        _pad_untouched(got, n, tag)
        _within(got[:, :n], p, units, tag)
        assert np.all(got[:, :n] >= 0)
        assert np.all(np.abs(got[:, :n].astype(F64).sum(axis=1) - 1.0) <= (n + 2) * U24), tag
        assert np.all(got[:, :n][np.isneginf(z)] == 0)
        equal = np.all(z == z[:, :1], axis=1)
        _same_bits(got[:, :n][equal], np.full((equal.sum(), n), F32(1) / F32(n), dtype=F32), tag + " all-equal rows")


# ------------------------------------------------------------------------------------------------ discrete PPO head
@functools.lru_cache(maxsize=None)
def _discrete_case(B, n):
    c = R.ppo_discrete_case(np.random.RandomState(B * 32 + n), B, n, 0.2)
    refs = {(beta, gs): R.ppo_discrete_loss(c["logits"], c["actions"], c["advantages"], c["old_probs"], 0.2, beta, None, gs)
            for beta, gs in ((0.01, 1.0), (0.0, 1.0), (0.05, 0.5))}
    v_rng = np.random.RandomState(B * 32 + n + 1)
    v, vt = v_rng.randn(B).astype(F32), v_rng.randn(B).astype(F32)
    return c, refs, v, vt


def _run_discrete(rlx, dev, c, B, n, beta, gs, pad, outputs=("dlogits", "scalars", "ratio", "clipped"), device_scale=False,
                  clip_eps=0.2, value=None):
    """one launch of rlx_ppo_discrete_loss, or of rlx_ppo_discrete_value_losses when value = (v, v_target)"""
    ld = n + pad
    bufs = dict(dlogits=_sent((B, ld), dev), scalars=_sent((4,), dev), ratio=_sent((B,), dev), clipped=_sent((B,), dev))
    bufs = {k: (b if k in outputs else None) for k, b in bufs.items()}
    status = _d(np.zeros(1, dtype=np.int32), dev)
    eps, scale = (2 * clip_eps, _d(np.array([0.5], dtype=F32), dev)) if device_scale else (clip_eps, None)
    head = (_d(_pitched(c["logits"][:, :n], ld), dev), ld, _d(c["actions"], dev), _d(c["advantages"], dev),
            _d(_pitched(c["old_probs"][:, :n], ld), dev), ld, B, n, eps, beta, gs, bufs["dlogits"], ld, bufs["scalars"],
            bufs["ratio"], bufs["clipped"], status)
    if value is None:
        rlx.ppo_discrete_loss(*head, scale, 0)
    else:
        bufs["dv"], bufs["v_loss"] = _sent((B,), dev), _sent((1,), dev)
        rlx.ppo_discrete_value_losses(*head, _d(value[0], dev), _d(value[1], dev), bufs["dv"], bufs["v_loss"], scale, 0)
    got = {k: _h(b) for k, b in bufs.items() if b is not None}
    got["status"] = int(_h(status)[0])
    return got


def _check_discrete(got, ref, n, tag, rows=None):
    rows = slice(None) if rows is None else rows
    if "dlogits" in got:
        _within(got["dlogits"][:, :n][rows], ref["dlogits"][rows], ref["dlogits_units"][rows], tag + " dlogits")
    if "scalars" in got:
        _within(got["scalars"], ref["scalars"], ref["scalars_units"], tag + " scalars")
    for k in ("ratio", "clipped"):
        if k in got:
            _within(got[k][rows], ref[k][rows], ref[k + "_units"][rows], tag + " " + k)


@pytest.mark.gpu
@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("B", BATCHES)
def test_ppo_discrete_loss(rlx, dev, B, n):
    """rlx_ppo_discrete_loss on head_loss_ref.ppo_discrete_case (every ratio 1e-3 clear of the clip bounds; the four
    gradient-routing quadrants and both signs inside the band present from 6 rows on, asserted on the CPU by
    tests/test_head_loss_ref.py): ratio, clipped ratio, the four scalars and dlogits within the bounds counted in
    head_loss_ref.ppo_discrete_loss.  Contiguous and ld = n + 5 on logits, old_probs and dlogits (NaN / sentinel
    padding); beta 0 / 0.01; grad_scale 0.5 with beta 0.05; the clip range as 0.4 x a device scalar 0.5 against the host
    value 0.2; every output alone and absent.  Rows whose gradient is cut (ratio beyond the bound on the advantage's side)
    owe exactly the entropy term: with beta 0 their dlogits are exactly 0."""
    c, refs, _, _ = _discrete_case(B, n)
    for beta, gs in ((0.01, 1.0), (0.0, 1.0), (0.05, 0.5)):
        ref = refs[(beta, gs)]
        for pad in (0, PAD):
            for device_scale in (False, True):
                tag = "ppo_discrete[%d,%d,beta%g,pad%d,dev%d]" % (B, n, beta, pad, device_scale)
                got = _run_discrete(rlx, dev, c, B, n, beta, gs, pad, device_scale=device_scale)
                assert got["status"] == 0
                _pad_untouched(got["dlogits"], n, tag)
                _check_discrete(got, ref, n, tag)
                if beta == 0.0:
                    assert not got["dlogits"][:, :n][~ref["passes"]].any(), tag
                    cut = ~ref["passes"]
                    assert cut.any() or B < R.MIN_QUADRANT_ROWS or n < 2
    ref = refs[(0.01, 1.0)]
    full = _run_discrete(rlx, dev, c, B, n, 0.01, 1.0, PAD)
    for k in ("dlogits", "scalars", "ratio", "clipped"):
        alone = _run_discrete(rlx, dev, c, B, n, 0.01, 1.0, PAD, outputs=(k,))
        assert set(alone) == {k, "status"}
        _same_bits(alone[k], full[k], k + " alone")
        _check_discrete(alone, ref, n, "ppo_discrete[%d,%d] %s alone" % (B, n, k))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 4])
def test_ppo_discrete_loss_on_the_clip_boundary(rlx, dev, n):
    """All-zero logits against uniform old probabilities over 2 and 4 actions, clip_eps = 0: lo = hi = 1 and the ratio is
    1.  First: the kernel's ratio_out is exactly 1.0f (the construction holds).  Then s1 == s2, tf.minimum gives the
    gradient to the unclipped branch, and the gradient is the pass-through one, -adv / B ([j = a] - 1 / n), for advantage
    +1, -1 and 0 alike -- within the counted bound of head_loss_ref, whose float64 ratio is exactly 1 as well."""
    B = 6
    c = dict(logits=np.zeros((B, n), dtype=F32), old_probs=np.full((B, n), 1.0 / n, dtype=F32),
             actions=(np.arange(B) % n).astype(np.int32), advantages=np.array([1, -1, 0, 1, -1, 0], dtype=F32))
    ref = R.ppo_discrete_loss(c["logits"], c["actions"], c["advantages"], c["old_probs"], 0.0, 0.0)
    assert np.all(ref["ratio"] == 1.0) and ref["lo"] == ref["hi"] == 1.0 and ref["passes"].all()
    got = _run_discrete(rlx, dev, c, B, n, 0.0, 1.0, 0, clip_eps=0.0)
    _same_bits(got["ratio"], np.ones(B, dtype=F32), "ratio_out is exactly 1")
    _same_bits(got["clipped"], np.ones(B, dtype=F32), "clipped ratio")
    onehot = np.arange(n)[None, :] == c["actions"][:, None]
    want = -c["advantages"].astype(F64)[:, None] / B * (onehot - 1.0 / n)
    np.testing.assert_allclose(ref["dlogits"], want, rtol=1e-14, atol=0)
    _within(got["dlogits"], ref["dlogits"], ref["dlogits_units"], "pass-through gradient")
    assert np.all((got["dlogits"] != 0) == (c["advantages"] != 0)[:, None])
    _within(got["scalars"], ref["scalars"], ref["scalars_units"], "scalars")


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["above", "below"])
def test_ppo_discrete_loss_tie_of_the_fp32_products(rlx, dev, side):
    """tf.minimum(s1, s2) gives the gradient to s1 = ratio * adv where s1 <= s2 -- a comparison of the two fp32 PRODUCTS.
    Inside the band s1 == s2 because the factors are equal, and both routes pass the gradient; the only tie that the `<=`
    decides is one between products of different factors that round to the same number.  Built here with the smallest
    denormal as the advantage: ratio = 1.3 against hi = 1.2 and adv = +2^-149 (0.7 against lo = 0.8 and adv = -2^-149)
    -- 1.3 and 1.2 (0.7 and 0.8) times one unit both round to one unit.  Asserted first, in numpy fp32 on the kernel's own
    ratio and clipped ratio: the construction holds (the ratio is outside the band, the products are equal).  Then the
    gradient is the pass-through one: -adv ratio ([j = a] - p_j) with B = 1, beta = 0 is -+2^-149 times a factor of
    magnitude 0.8, which rounds to one unit: dlogits = [-adv, +adv] bit for bit.  (In exact arithmetic the products
    differ and the gradient is cut: head_loss_ref says 0 -- the kernel owes TensorFlow's fp32 comparison, not that.)"""
    tiny = np.nextafter(F32(0), F32(1))
    target, adv = (1.3, tiny) if side == "above" else (0.7, -tiny)
    p_new = np.array([[0.2, 0.8]])
    c = dict(logits=np.log(p_new).astype(F32), actions=np.zeros(1, dtype=np.int32), advantages=np.array([adv], dtype=F32),
             old_probs=np.array([[0.2 / target, 1 - 0.2 / target]], dtype=F32))
    ref = R.ppo_discrete_loss(c["logits"], c["actions"], c["advantages"], c["old_probs"], 0.2, 0.0)
    assert not ref["passes"][0] and not ref["dlogits"].any()
    got = _run_discrete(rlx, dev, c, 1, 2, 0.0, 1.0, 0)
    _within(got["ratio"], ref["ratio"], ref["ratio_units"], "ratio")
    ratio, clipped = F32(got["ratio"][0]), F32(got["clipped"][0])
    assert clipped == (F32(1) + F32(0.2) if side == "above" else F32(1) - F32(0.2)) and ratio != clipped
    assert ratio * adv == clipped * adv == adv                       # the fp32 products tie
    _same_bits(got["dlogits"], np.array([[-adv, adv]], dtype=F32), "pass-through gradient on the tie")


@pytest.mark.gpu
@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("B", BATCHES)
def test_ppo_discrete_value_losses(rlx, dev, B, n):
    """rlx_ppo_discrete_value_losses: the PPO head against head_loss_ref.ppo_discrete_loss and the value head against
    head_loss_ref.regression_loss (mean squared error, one column, weight 1, the same grad_scale), each at its counted
    bound, pitched; and bit for bit what the two separate launches write."""
    c, refs, v, vt = _discrete_case(B, n)
    beta, gs = 0.05, 0.5
    ref = refs[(beta, gs)]
    vref = R.regression_loss(v[:, None], vt[:, None], None, "mse", 1.0, gs)
    tag = "ppo_value[%d,%d]" % (B, n)
    got = _run_discrete(rlx, dev, c, B, n, beta, gs, PAD, device_scale=True, value=(v, vt))
    assert got["status"] == 0
    _pad_untouched(got["dlogits"], n, tag)
    _check_discrete(got, ref, n, tag)
    _within(got["dv"], vref["grad"][:, 0], vref["grad_units"][:, 0], tag + " dvalues")
    _within(got["v_loss"], [vref["loss"]], [vref["loss_units"]], tag + " value loss")
    head = _run_discrete(rlx, dev, c, B, n, beta, gs, PAD, device_scale=True)
    for k in ("dlogits", "scalars", "ratio", "clipped"):
        _same_bits(got[k], head[k], k + " of the joint launch")
    dv, vl = _run_regression(rlx, dev, v[:, None], vt[:, None], None, B, 1, "mse", 1.0, gs, 0)
    _same_bits(got["dv"], dv[:, 0], "dvalues of the joint launch")
    _same_bits(got["v_loss"], vl, "value loss of the joint launch")


@pytest.mark.gpu
@pytest.mark.parametrize("bad_action", [-1, "n"])
@pytest.mark.parametrize("B,n", [(65, 6), (1025, 2)])
def test_ppo_discrete_value_losses_rejects_a_bad_action(rlx, dev, B, n, bad_action):
    """One action index outside [0, n): bit 0 of status is set, the row writes nothing (its dlogits row, ratio and
    clipped ratio keep the sentinel), and every other row and the value head are what they are without it.  PINNED from
    ppo_discrete_scalars: the three batch sums skip the rejected row but are still multiplied by 1 / batch -- the scalars
    are sums over the valid rows divided by B, not by B - 1 (for the entropy the two differ by far more than the bound, asserted)."""
    c, refs, v, vt = _discrete_case(B, n)
    c = dict(c)
    bad = B // 2
    c["actions"] = c["actions"].copy()
    c["actions"][bad] = n if bad_action == "n" else bad_action
    beta, gs = 0.05, 0.5
    ref = R.ppo_discrete_loss(c["logits"], c["actions"], c["advantages"], c["old_probs"], 0.2, beta, None, gs)
    assert ref["valid"].sum() == B - 1 and not ref["valid"][bad]
    got = _run_discrete(rlx, dev, c, B, n, beta, gs, PAD, value=(v, vt))
    assert got["status"] & 1
    tag = "ppo_value_bad[%d,%d]" % (B, n)
    _check_discrete(got, ref, n, tag, rows=ref["valid"])
    other = ref["scalars"][1] * B / (B - 1)           # (on the entropy: a sum of positive terms, never small)
    assert abs(other - ref["scalars"][1]) > 4 * U24 * ref["scalars_units"][1]
    for k in ("ratio", "clipped"):
        _same_bits(got[k][bad], SENT, k + " of the rejected row")
    _same_bits(got["dlogits"][bad], np.full(n + PAD, SENT, dtype=F32), "dlogits of the rejected row")
    _pad_untouched(got["dlogits"], n, tag)
    vref = R.regression_loss(v[:, None], vt[:, None], None, "mse", 1.0, gs)
    _within(got["dv"], vref["grad"][:, 0], vref["grad_units"][:, 0], tag + " dvalues")
    _within(got["v_loss"], [vref["loss"]], [vref["loss_units"]], tag + " value loss")


# ------------------------------------------------------------------------------------------------ continuous PPO head
@functools.lru_cache(maxsize=None)
def _continuous_case(B, A):
    c = R.ppo_continuous_case(np.random.RandomState(B * 32 + A), B, A, 0.2)
    refs = {(beta, gs): R.ppo_continuous_loss(c["mean"], c["log_std"], c["actions"], c["advantages"], c["old_mean"],
                                              c["old_std"], 0.2, beta, None, gs) for beta, gs in ((0.01, 1.0), (0.05, 0.5))}
    return c, refs


def _run_continuous(rlx, dev, c, B, A, beta, gs, pad, outputs=("grads", "scalars", "ratio", "clipped"), device_scale=False):
    ld = A + pad
    bufs = dict(dmean=_sent((B, ld), dev), dlog_std=_sent((A,), dev), scalars=_sent((4,), dev), ratio=_sent((B,), dev),
                clipped=_sent((B,), dev))
    keep = set(outputs) | ({"dmean", "dlog_std"} if "grads" in outputs else set())
    bufs = {k: (b if k in keep else None) for k, b in bufs.items()}
    eps, scale = (0.4, _d(np.array([0.5], dtype=F32), dev)) if device_scale else (0.2, None)
    rlx.ppo_continuous_loss(_d(_pitched(c["mean"][:, :A], ld), dev), ld, _d(c["log_std"], dev), _d(c["actions"], dev),
                            _d(c["advantages"], dev), _d(_pitched(c["old_mean"][:, :A], ld), dev),
                            _d(_pitched(c["old_std"][:, :A], ld), dev), ld, B, A, eps, beta, gs, bufs["dmean"], ld,
                            bufs["dlog_std"], bufs["scalars"], bufs["ratio"], bufs["clipped"], scale, 0)
    return {k: _h(b) for k, b in bufs.items() if b is not None}


def _check_continuous(got, ref, A, tag):
    if "dmean" in got:
        _within(got["dmean"][:, :A], ref["dmean"], ref["dmean_units"], tag + " dmean")
        _within(got["dlog_std"], ref["dlog_std"], ref["dlog_std_units"], tag + " dlog_std")
    for k in ("scalars", "ratio", "clipped"):
        if k in got:
            _within(got[k], ref[k], ref[k + "_units"], tag + " " + k)


@pytest.mark.gpu
@pytest.mark.parametrize("A", WIDTHS)
@pytest.mark.parametrize("B", SMALL_BATCHES)
def test_ppo_continuous_loss(rlx, dev, B, A):
    """rlx_ppo_continuous_loss on head_loss_ref.ppo_continuous_case (ratios 1e-3 clear of the clip bounds, the four
    routing quadrants present from 6 rows on): ratio, clipped ratio, scalars, dmean and dlog_std within the bounds counted
    in head_loss_ref.ppo_continuous_loss.  Contiguous and ld = A + 5 on mean, old_mean, old_std and dmean (NaN / sentinel
    padding); grad_scale 0.5 with beta 0.05; the clip range as a device scalar; each output alone (the two gradients go
    together).  A row whose gradient is cut owes a dmean row of exact zeros."""
    c, refs = _continuous_case(B, A)
    for beta, gs in ((0.01, 1.0), (0.05, 0.5)):
        ref = refs[(beta, gs)]
        for pad in (0, PAD):
            for device_scale in (False, True):
                tag = "ppo_continuous[%d,%d,beta%g,pad%d,dev%d]" % (B, A, beta, pad, device_scale)
                got = _run_continuous(rlx, dev, c, B, A, beta, gs, pad, device_scale=device_scale)
                _pad_untouched(got["dmean"], A, tag)
                _check_continuous(got, ref, A, tag)
                assert not got["dmean"][:, :A][~ref["passes"]].any(), tag
    full = _run_continuous(rlx, dev, c, B, A, 0.01, 1.0, PAD)
    for k in ("grads", "scalars", "ratio", "clipped"):
        alone = _run_continuous(rlx, dev, c, B, A, 0.01, 1.0, PAD, outputs=(k,))
        assert set(alone) == ({"dmean", "dlog_std"} if k == "grads" else {k})
        for name in alone:
            _same_bits(alone[name], full[name], name + " alone")


@pytest.mark.gpu
def test_single_workgroup_losses_refuse_more_than_1024_rows(rlx, dev):
    """rlx_ppo_continuous_loss and rlx_ac_critic_losses hold one row per thread of one workgroup: 1025 rows are an error
    (and so is a single gradient output of the continuous head), not a silent truncation."""
    B, A = 1025, 2
    z = _d(np.zeros((B, A), dtype=F32), dev)
    one = _d(np.ones((B, A), dtype=F32), dev)
    vec, ls = _d(np.zeros(B, dtype=F32), dev), _d(np.zeros(A, dtype=F32), dev)
    with pytest.raises(RlxError):
        rlx.ppo_continuous_loss(z, A, ls, z, vec, z, one, A, B, A, 0.2, 0.0, 1.0, None, A, None, _sent((4,), dev), None, None,
                                None, 0)
    with pytest.raises(RlxError):
        rlx.ppo_continuous_loss(z, A, ls, z, vec, z, one, A, 64, A, 0.2, 0.0, 1.0, _sent((64, A), dev), A, None, None, None,
                                None, None, 0)
    done = _d(np.zeros(B, dtype=np.uint8), dev)
    with pytest.raises(RlxError):
        rlx.ac_critic_losses(vec, None, vec, done, 0.99, 0, 0, 0.0, 0.0, vec, 1, B, 1.0, None, _sent((B,), dev),
                             _sent((B,), dev), _sent((2,), dev), 0)
    with pytest.raises(RlxError):
        rlx.ac_critic_losses(vec, None, vec, done, 0.99, 0, 0, 0.0, 0.0, vec, 5, 64, 1.0, None, _sent((B,), dev),
                             _sent((B,), dev), _sent((6,), dev), 0)


# ------------------------------------------------------------------------------------------------ rlx_ac_critic_losses
AC_OPTIONS = [(T, twin, want_min, has_clip, nonzero, lw)
              for T, twin, want_min, has_clip, nonzero, lw in
              ((1, False, False, False, False, 1.0), (2, True, True, True, False, 1.0), (3, True, False, False, True, 0.5),
               (4, False, True, True, True, 0.5), (2, True, True, False, False, 0.5), (1, False, True, True, False, 1.0))]


@pytest.mark.gpu
@pytest.mark.parametrize("T,twin,want_min,has_clip,nonzero,lw", AC_OPTIONS)
@pytest.mark.parametrize("B", SMALL_BATCHES)
def test_ac_critic_losses(rlx, dev, B, T, twin, want_min, has_clip, nonzero, lw):
    """rlx_ac_critic_losses against head_loss_ref.ac_critic_losses, 1 to 4 streams, q_next2 / q_min_out / the clip / the
    terminal-discount flag on and off, loss_weight 1 and 0.5:
      q_min_out   bit for bit (a selection; ties and +-0 go to q_next1)
      td_targets  the float64 target rounded once: within (1 + 2^-20) 2^-24 |y| -- one rounding, the cast; the 2^-20
                  covers the last float64 bit, which a contracted r + d q may round differently from numpy
      dq, loss    head_loss_ref.regression_loss's counted bounds AT THE DEVICE'S OWN td_targets; total: the streams'
                  units + T sum |loss_t|.  Rows that are terminal, clipped on either side and tied are all present
                  from 65 rows on (asserted)."""
    rng = np.random.RandomState(B * 8 + T)
    q1, q2 = (2 * rng.randn(B)).astype(F32), (2 * rng.randn(B)).astype(F32)
    k = np.arange(B)
    q2[k % 4 == 1] = q1[k % 4 == 1]
    q1[k % 16 == 3], q2[k % 16 == 3] = 0.0, -0.0
    rew = rng.randn(B).astype(F32)
    done = (k % 3 == 0).astype(np.uint8)
    q = rng.randn(T, B).astype(F32)
    clip = (-1.5, 1.5)
    exact = R.ac_critic_losses(q1, q2 if twin else None, rew, done, 0.99, q, lw, clip if has_clip else None, nonzero)
    if B >= 65 and has_clip:
        assert (exact["y"] == clip[0]).any() and (exact["y"] == clip[1]).any() and (np.abs(exact["y"]) < 1.5).any()
    qmin = _sent((B,), dev) if want_min else None
    y, dq, loss = _sent((B,), dev), _sent((T, B), dev), _sent((T + 1,), dev)
    rlx.ac_critic_losses(_d(q1, dev), _d(q2, dev) if twin else None, _d(rew, dev), _d(done, dev), 0.99, int(nonzero),
                         int(has_clip), clip[0], clip[1], _d(q, dev), T, B, lw, qmin, y, dq, loss, 0)
    tag = "ac_critic[%d,%d,%d,%d,%d,%d]" % (B, T, twin, want_min, has_clip, nonzero)
    if want_min:
        _same_bits(_h(qmin), exact["q_min"], "q_min_out")
    y_dev = _h(y)
    _within(y_dev, exact["y"], (1 + 2.0 ** -20) * exact["y_units"], tag + " td_targets")
    if not nonzero:
        term = done.astype(bool)
        _same_bits(y_dev[term], np.clip(rew[term], F32(clip[0]), F32(clip[1])) if has_clip else rew[term], "terminal targets")
    ref = R.ac_critic_losses(q1, q2 if twin else None, rew, done, 0.99, q, lw, clip if has_clip else None, nonzero,
                             td_targets=y_dev)
    _within(_h(dq), ref["dq"], ref["dq_units"], tag + " dq")
    got_loss = _h(loss)
    _within(got_loss[:T], ref["loss"], ref["loss_units"], tag + " loss")
    _within(got_loss[T:], [ref["total"]], [ref["total_units"]], tag + " total")


@pytest.mark.gpu
@pytest.mark.parametrize("nonzero", [False, True])
def test_ac_critic_losses_keeps_a_nan_target(rlx, dev, nonzero):
    """a diverged target critic: np.clip keeps the NaN (the reference's np.minimum(np.maximum())), so that row's target and
    gradient and every loss are NaN and not clip_low; +-inf is clipped to the bound; the other rows keep their bits"""
    B, T, clip = 65, 2, (-1.5, 1.5)
    rng = np.random.RandomState(B + nonzero)
    q1, q2 = (2 * rng.randn(B)).astype(F32), (2 * rng.randn(B)).astype(F32)
    rew, done, q = rng.randn(B).astype(F32), (np.arange(B) % 3 == 0).astype(np.uint8), rng.randn(T, B).astype(F32)
    done[[7, 20]] = 0
    q1[7], q2[7], q2[20], q1[30], q2[30], q1[31], q2[31] = np.nan, np.nan, np.nan, np.inf, np.inf, -np.inf, -np.inf
    done[[30, 31]] = 0
    with np.errstate(invalid="ignore"):
        want = R.ac_critic_losses(q1, q2, rew, done, 0.99, q, 1.0, clip, nonzero)
    # q2[20] = NaN: q_min = q1 <= q2 ? q1 : q2 takes the NaN in the kernel and in the reference's np.where
    isnan = np.zeros(B, dtype=bool)
    isnan[[7, 20]] = True
    assert np.array_equal(np.isnan(want["y"]), isnan) and want["y"][30] == clip[1] and want["y"][31] == clip[0]
    y, dq, loss = _sent((B,), dev), _sent((T, B), dev), _sent((T + 1,), dev)
    rlx.ac_critic_losses(_d(q1, dev), _d(q2, dev), _d(rew, dev), _d(done, dev), 0.99, int(nonzero), 1, clip[0], clip[1],
                         _d(q, dev), T, B, 1.0, None, y, dq, loss, 0)
    y_dev, dq_dev = _h(y), _h(dq)
    assert np.array_equal(np.isnan(y_dev), isnan), y_dev
    _within(y_dev[~isnan], want["y"][~isnan], (1 + 2.0 ** -20) * want["y_units"][~isnan], "finite targets")
    _same_bits(y_dev[[30, 31]], np.array([clip[1], clip[0]], dtype=F32), "infinite targets are clipped")
    assert np.array_equal(np.isnan(dq_dev), np.broadcast_to(isnan, (T, B)))
    assert np.isnan(_h(loss)).all()
