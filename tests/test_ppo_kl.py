"""The PPO-penalty head launches of csrc/ppo_kl.hip (rlx_ppo_kl_discrete_loss, rlx_ppo_kl_continuous_loss) and
rlx_ppo_kl_coefficient_update, called by name, against the float64 restatement tests/ppo_kl_ref.py.

Every comparison is either bit for bit or |got - float64| <= 2^-24 * units, `units` being the bound the restatement counts
from the kernel's chain of fp32 operations (nothing here is measured).  Batch sizes: one row, one wave and its
neighbours, several waves, an odd size, the 1024-row cap; 1025 rows are refused.  Inputs with a pitch carry NaN in their
padding columns, outputs a sentinel that must come back unchanged.  For every shape one case has its KL mean below
kl_cutoff and one above it (ppo_kl_ref.kl_penalty asserts the side, with a margin of 10 % of the cutoff).

The discrete launch shares rlx_losses::ppo_discrete_row with rlx_ppo_discrete_loss: without the KL terms it is that
kernel bit for bit.  The continuous launch RESTATES ppo_continuous_loss_kernel's arithmetic (that kernel's products are
left to FMA contraction, csrc/ppo_kl.hip's are not), so against rlx_ppo_continuous_loss the bar is the counted bound."""
import functools

import numpy as np
import pytest

import head_loss_ref as H
import ppo_kl_ref as R
from coach_amd._rlx import RlxError

F32, F64 = np.float32, np.float64
U24 = R.U24
SENT = F32(-777.25)
PAD = 5
BATCHES = [1, 2, 63, 64, 65, 128, 257, 1024]
N_ACTIONS = [1, 2, 6, 18]
ACTION_DIMS = [1, 3, 17, 32]
KLC, HIGH = 0.1, 1000.0                              # a kl_coefficient; high_kl_penalty_coefficient's default (ppo_agent.py:117)
SETTINGS = ((0.0, 1.0), (0.01, 0.5))                 # (beta_entropy, grad_scale)
SIDES = ("below", "above")


def _d(x, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _h(t):
    return None if t is None else t.cpu().numpy()


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
    out = np.full((a.shape[0], ld), np.nan, dtype=F32)
    out[:, :a.shape[1]] = a
    return out


def _pad_untouched(buf, n, what):
    if buf.shape[1] > n:
        _same_bits(buf[:, n:], np.full((buf.shape[0], buf.shape[1] - n), SENT, dtype=F32), what + ": padding columns")


ACC0 = np.array([0.5, -1.25, 3.0, 7.0], dtype=F32)


def _acc_after(acc0, scalars):
    s = np.asarray(scalars, dtype=F32)
    return (acc0 + np.array([s[2], s[1], s[3], 1.0], dtype=F32)).astype(F32)


# ------------------------------------------------------------------------------------------------ discrete
def _run_discrete(rlx, dev, case, n, pad, beta, gs, klc, cutoff, high, use_kl, want="gsra"):
    """-> dict(g [B, ld], s [5], r [B], a [4], status) of one launch; outputs not in `want` are absent (None)"""
    B, ld = case["logits"].shape[0], n + pad
    g = _sent((B, ld), dev) if "g" in want else None
    s = _sent((5,), dev) if "s" in want else None
    r = _sent((B,), dev) if "r" in want else None
    a = _d(ACC0.copy(), dev) if "a" in want else None
    status = _d(np.zeros(1, dtype=np.int32), dev)
    rlx.ppo_kl_discrete_loss(_d(_pitched(case["logits"][:, :n], ld), dev), ld, _d(case["actions"].astype(np.int32), dev),
                             _d(case["advantages"], dev), _d(_pitched(case["old_probs"][:, :n], ld), dev), ld, B, n, beta,
                             gs, _d(np.array([klc], dtype=F32), dev), float(cutoff), high, int(use_kl), g, ld, s, r,
                             status, a, 0)
    return dict(g=_h(g), s=_h(s), r=_h(r), a=_h(a), status=int(_h(status)[0]))


@functools.lru_cache(maxsize=None)
def _discrete_refs(B, n):
    case = R.discrete_case(B * 64 + n, B, n)
    refs = {}
    for beta, gs in SETTINGS:
        for side in SIDES:
            cutoff = R.cutoff_for(case["kl_mean"], side)
            ref = R.ppo_kl_discrete_loss(case["logits"], case["actions"], case["advantages"], case["old_probs"], beta,
                                         KLC, cutoff, HIGH, True, gs)
            assert ref["side"] == side and ref["valid"].all()
            refs[(beta, gs, side)] = (cutoff, ref)
    return case, refs


def _check_discrete(out, ref, n, tag):
    _pad_untouched(out["g"], n, tag)
    _within(out["g"][:, :n], ref["dlogits"], ref["dlogits_units"], tag + " dlogits")
    _within(out["r"], ref["ratio"], ref["ratio_units"], tag + " ratio")
    _within(out["s"], ref["scalars"], ref["scalars_units"], tag + " scalars")
    _same_bits(out["a"], _acc_after(ACC0, out["s"]), tag + " accumulate")


@pytest.mark.gpu
@pytest.mark.parametrize("n", N_ACTIONS)
@pytest.mark.parametrize("B", BATCHES)
def test_discrete_loss(rlx, dev, B, n):
    """gradient, ratio, the five scalars and the accumulate buffer against ppo_kl_ref.ppo_kl_discrete_loss at its counted
    bounds: KL mean below and above the cutoff, beta 0 / grad_scale 1 and beta 0.01 / grad_scale 0.5, contiguous and with
    ld = n + 5 (NaN / sentinel padding); each output alone, and all absent, bit for bit what the joint launch wrote."""
    case, refs = _discrete_refs(B, n)
    for (beta, gs, side), (cutoff, ref) in refs.items():
        for pad in (0, PAD):
            tag = "kl_discrete[%d,%d,b%g,gs%g,%s,pad%d]" % (B, n, beta, gs, side, pad)
            out = _run_discrete(rlx, dev, case, n, pad, beta, gs, KLC, cutoff, HIGH, True)
            assert out["status"] == 0
            _check_discrete(out, ref, n, tag)
            if pad and beta and side == "above":
                for key in "gsra":
                    alone = _run_discrete(rlx, dev, case, n, pad, beta, gs, KLC, cutoff, HIGH, True, want=key)
                    assert all(alone[k] is None for k in "gsra" if k != key) and alone["status"] == 0
                    _same_bits(alone[key], out[key], tag + " %s alone" % key)
                assert _run_discrete(rlx, dev, case, n, pad, beta, gs, KLC, cutoff, HIGH, True, want="")["status"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", N_ACTIONS)
@pytest.mark.parametrize("B", BATCHES)
def test_discrete_without_kl_is_the_clipped_head_unclipped(rlx, dev, B, n):
    """use_kl_regularization = 0: dlogits, ratio and scalars[0..2] are rlx_ppo_discrete_loss's bit for bit at a clip range
    that never binds (both kernels call rlx_losses::ppo_discrete_row); scalars[3] = surrogate - beta entropy in the same
    expression, so it is bit-identical too; c = 0.  For every grad_scale: the row function applies it in both kernels."""
    import torch
    case, _ = _discrete_refs(B, n)
    for beta, gs in SETTINGS + ((0.01, 0.3),):           # 0.3: a scale whose product rounds
        out = _run_discrete(rlx, dev, case, n, PAD, beta, gs, KLC, 0.02, HIGH, False)
        ld = n + PAD
        g, s, r = _sent((B, ld), dev), _sent((4,), dev), _sent((B,), dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        rlx.ppo_discrete_loss(_d(_pitched(case["logits"], ld), dev), ld, _d(case["actions"].astype(np.int32), dev),
                              _d(case["advantages"], dev), _d(_pitched(case["old_probs"], ld), dev), ld, B, n,
                              R.NO_CLIP, beta, gs, g, ld, s, r, None, status, None, 0)
        tag = "kl_discrete_off[%d,%d,b%g]" % (B, n, beta)
        _same_bits(out["g"], _h(g), tag + " dlogits")
        _same_bits(out["r"], _h(r), tag + " ratio")
        _same_bits(out["s"][:4], _h(s), tag + " scalars")
        _same_bits(out["s"][4:], [0.0], tag + " c")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 4, 16])
def test_discrete_identical_policies(rlx, dev, n):
    """new policy = old policy = uniform over a power-of-two number of actions (z = 0, old = 1 / n: every intermediate is
    exact, log(1 / n) = -log(n) by the symmetry of log2): KL exactly 0, c exactly kl_coefficient, and the KL term adds
    exactly 0 to every gradient row (the gradient equals the one without KL regularisation)."""
    B = 65
    rng = np.random.RandomState(n)
    case = dict(logits=np.zeros((B, n), dtype=F32), old_probs=np.full((B, n), 1.0 / n, dtype=F32),
                actions=rng.randint(0, n, B).astype(np.int32), advantages=rng.randn(B).astype(F32))
    on = _run_discrete(rlx, dev, case, n, 0, 0.01, 1.0, 0.7, 0.02, HIGH, True)
    off = _run_discrete(rlx, dev, case, n, 0, 0.01, 1.0, 0.7, 0.02, HIGH, False)
    _same_bits(on["s"][2:3], [0.0], "KL")
    _same_bits(on["s"][4:], [F32(0.7)], "c")
    assert np.array_equal(on["g"], off["g"]) and np.all(np.isfinite(on["g"]))
    _same_bits(on["r"], np.ones(B, dtype=F32), "ratio")


@pytest.mark.gpu
def test_discrete_old_policy_from_softmax(rlx, dev):
    """old probabilities = rlx_softmax of the same logits (what the target actor hands out right after sync()): in every
    row whose fp32 probabilities sum to exactly 1 the KL gradient row p_j - old_j / sum(old) is exactly 0 -- phase C forms
    p_j by rlx_softmax's expression -- so the gradient row equals the one without KL regularisation."""
    B, n = 257, 6
    rng = np.random.RandomState(5)
    z = rng.randn(B, n).astype(F32)
    probs = _sent((B, n), dev)
    rlx.softmax(_d(z, dev), n, B, n, probs, n, 0)
    po = _h(probs)
    so = np.zeros(B, dtype=F32)
    for j in range(n):
        so = (so + po[:, j]).astype(F32)
    exact = so == F32(1.0)
    assert exact.sum() >= 8
    case = dict(logits=z, old_probs=po, actions=rng.randint(0, n, B).astype(np.int32), advantages=rng.randn(B).astype(F32))
    on = _run_discrete(rlx, dev, case, n, 0, 0.0, 1.0, 0.7, 0.02, HIGH, True)
    off = _run_discrete(rlx, dev, case, n, 0, 0.0, 1.0, 0.7, 0.02, HIGH, False)
    assert np.array_equal(on["g"][exact], off["g"][exact])


@pytest.mark.gpu
@pytest.mark.parametrize("B,n", [(65, 6), (1024, 18), (2, 1)])
def test_discrete_action_out_of_range(rlx, dev, B, n):
    """actions -1 and n: status bit 0 is set, the rows' gradient and ratio are exactly 0, and every other value is the
    restatement's under the same rule (the rejected rows add nothing, the means divide by B)."""
    case, _ = _discrete_refs(B, n)
    case = dict(case, actions=case["actions"].copy())
    case["actions"][0] = n
    case["actions"][B // 2 + (B > 2)] = -1
    bad = (case["actions"] < 0) | (case["actions"] >= n)
    kl = float(H.ppo_discrete_loss(case["logits"], case["actions"], case["advantages"], case["old_probs"], R.NO_CLIP,
                                   0.0)["scalars"][2])
    for side in SIDES:
        cutoff = R.cutoff_for(kl, side)
        ref = R.ppo_kl_discrete_loss(case["logits"], case["actions"], case["advantages"], case["old_probs"], 0.01, KLC,
                                     cutoff, HIGH, True, 0.5)
        assert ref["side"] == side and not ref["valid"][bad].any() and ref["valid"][~bad].all()
        out = _run_discrete(rlx, dev, case, n, PAD, 0.01, 0.5, KLC, cutoff, HIGH, True)
        assert out["status"] == 1
        _same_bits(out["g"][bad, :n], np.zeros((bad.sum(), n), dtype=F32), "rejected gradient rows")
        _same_bits(out["r"][bad], np.zeros(bad.sum(), dtype=F32), "rejected ratios")
        _check_discrete(out, ref, n, "kl_discrete_rejected[%d,%d,%s]" % (B, n, side))


@pytest.mark.gpu
@pytest.mark.parametrize("B,n", [(1025, 6), (64, 19), (64, 0)])
def test_discrete_refusals(rlx, dev, B, n):
    """more than 1024 rows, more than 18 actions, no action: the library's error, and nothing is written"""
    m = max(n, 1)
    case = dict(logits=np.zeros((B, m), dtype=F32), old_probs=np.full((B, m), 1.0 / m, dtype=F32),
                actions=np.zeros(B, dtype=np.int32), advantages=np.ones(B, dtype=F32))
    import torch
    g, s, r, a = _sent((B, m), dev), _sent((5,), dev), _sent((B,), dev), _sent((4,), dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(RlxError, match="rlx_ppo_kl_discrete_loss"):
        rlx.ppo_kl_discrete_loss(_d(case["logits"], dev), m, _d(case["actions"], dev), _d(case["advantages"], dev),
                                 _d(case["old_probs"], dev), m, B, n, 0.0, 1.0, _d(np.array([KLC], dtype=F32), dev), 0.02,
                                 HIGH, 1, g, m, s, r, status, a, 0)
    torch.cuda.synchronize()
    for buf in (g, s, r, a):
        assert np.all(_h(buf) == SENT)
    assert int(_h(status)[0]) == 0


# ------------------------------------------------------------------------------------------------ continuous
def _run_continuous(rlx, dev, case, A, pad, beta, gs, klc, cutoff, high, use_kl, want="glsra"):
    """-> dict(g dmean [B, ld], l dlog_std [A], s [5], r [B], a [4]) of one launch"""
    B, ld = case["mean"].shape[0], A + pad
    g = _sent((B, ld), dev) if "g" in want else None
    l = _sent((A,), dev) if "l" in want else None
    s = _sent((5,), dev) if "s" in want else None
    r = _sent((B,), dev) if "r" in want else None
    a = _d(ACC0.copy(), dev) if "a" in want else None
    rlx.ppo_kl_continuous_loss(_d(_pitched(case["mean"][:, :A], ld), dev), ld, _d(case["log_std"], dev),
                               _d(case["actions"], dev), _d(case["advantages"], dev),
                               _d(_pitched(case["old_mean"][:, :A], ld), dev), _d(_pitched(case["old_std"][:, :A], ld), dev),
                               ld, B, A, beta, gs, _d(np.array([klc], dtype=F32), dev), float(cutoff), high, int(use_kl),
                               g, ld, l, s, r, a, 0)
    return dict(g=_h(g), l=_h(l), s=_h(s), r=_h(r), a=_h(a))


@functools.lru_cache(maxsize=None)
def _continuous_refs(B, A):
    case = R.continuous_case(B * 64 + A, B, A)
    refs = {}
    for beta, gs in SETTINGS:
        for side in SIDES:
            cutoff = R.cutoff_for(case["kl_mean"], side)
            ref = R.ppo_kl_continuous_loss(case["mean"], case["log_std"], case["actions"], case["advantages"],
                                           case["old_mean"], case["old_std"], beta, KLC, cutoff, HIGH, True, gs)
            assert ref["side"] == side
            refs[(beta, gs, side)] = (cutoff, ref)
    return case, refs


def _check_continuous(out, ref, A, tag):
    _pad_untouched(out["g"], A, tag)
    _within(out["g"][:, :A], ref["dmean"], ref["dmean_units"], tag + " dmean")
    _within(out["l"], ref["dlog_std"], ref["dlog_std_units"], tag + " dlog_std")
    _within(out["r"], ref["ratio"], ref["ratio_units"], tag + " ratio")
    _within(out["s"], ref["scalars"], ref["scalars_units"], tag + " scalars")
    _same_bits(out["a"], _acc_after(ACC0, out["s"]), tag + " accumulate")


@pytest.mark.gpu
@pytest.mark.parametrize("A", ACTION_DIMS)
@pytest.mark.parametrize("B", BATCHES)
def test_continuous_loss(rlx, dev, B, A):
    """as test_discrete_loss, for the Gaussian head: dmean, dlog_std, ratio, scalars and accumulate"""
    case, refs = _continuous_refs(B, A)
    for (beta, gs, side), (cutoff, ref) in refs.items():
        for pad in (0, PAD):
            tag = "kl_continuous[%d,%d,b%g,gs%g,%s,pad%d]" % (B, A, beta, gs, side, pad)
            out = _run_continuous(rlx, dev, case, A, pad, beta, gs, KLC, cutoff, HIGH, True)
            _check_continuous(out, ref, A, tag)
            if pad and beta and side == "above":
                for key in "glsra":
                    alone = _run_continuous(rlx, dev, case, A, pad, beta, gs, KLC, cutoff, HIGH, True, want=key)
                    assert all(alone[k] is None for k in "glsra" if k != key)
                    _same_bits(alone[key], out[key], tag + " %s alone" % key)
                _run_continuous(rlx, dev, case, A, pad, beta, gs, KLC, cutoff, HIGH, True, want="")


@pytest.mark.gpu
@pytest.mark.parametrize("B,A", [(1, 1), (65, 3), (257, 17), (1024, 32)])
def test_continuous_without_kl_against_the_clipped_head(rlx, dev, B, A):
    """use_kl_regularization = 0 against rlx_ppo_continuous_loss at a clip range that never binds.  The arithmetic is
    restated, not shared, so the bar is the counted bound: each kernel lies within its own bound of the same float64
    value, hence the two within the sum of the bounds."""
    case, _ = _continuous_refs(B, A)
    beta, gs = 0.01, 0.5
    out = _run_continuous(rlx, dev, case, A, 0, beta, gs, KLC, 0.02, HIGH, False)
    g, l, s, r = _sent((B, A), dev), _sent((A,), dev), _sent((4,), dev), _sent((B,), dev)
    rlx.ppo_continuous_loss(_d(case["mean"], dev), A, _d(case["log_std"], dev), _d(case["actions"], dev),
                            _d(case["advantages"], dev), _d(case["old_mean"], dev), _d(case["old_std"], dev), A, B, A,
                            R.NO_CLIP, beta, gs, g, A, l, s, r, None, None, 0)
    new = R.ppo_kl_continuous_loss(case["mean"], case["log_std"], case["actions"], case["advantages"], case["old_mean"],
                                   case["old_std"], beta, KLC, 0.02, HIGH, False, gs)
    old = H.ppo_continuous_loss(case["mean"], case["log_std"], case["actions"], case["advantages"], case["old_mean"],
                                case["old_std"], R.NO_CLIP, beta, None, gs)
    tag = "kl_continuous_off[%d,%d]" % (B, A)
    _within(out["g"], _h(g).astype(F64), new["dmean_units"] + old["dmean_units"], tag + " dmean")
    _within(out["l"], _h(l).astype(F64), new["dlog_std_units"] + old["dlog_std_units"], tag + " dlog_std")
    _within(out["r"], _h(r).astype(F64), new["ratio_units"] + old["ratio_units"], tag + " ratio")
    _within(out["s"][:4], _h(s).astype(F64), new["scalars_units"][:4] + old["scalars_units"], tag + " scalars")
    _same_bits(out["s"][4:], [0.0], tag + " c")


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 3, 32])
def test_continuous_identical_policies(rlx, dev, A):
    """old = new with log_std = 0 (exp(0) = 1, old_std = 1: sd and sd_old are the same fp32 number): every row's KL term
    is log(1) + x / (2 x) - 0.5 = 0 exactly, so KL = 0 and c = kl_coefficient exactly; the ratio is exactly 1."""
    B = 65
    rng = np.random.RandomState(A)
    mu = rng.randn(B, A).astype(F32)
    case = dict(mean=mu, log_std=np.zeros(A, dtype=F32), actions=(mu + rng.randn(B, A)).astype(F32),
                advantages=rng.randn(B).astype(F32), old_mean=mu.copy(), old_std=np.ones((B, A), dtype=F32))
    out = _run_continuous(rlx, dev, case, A, 0, 0.0, 1.0, 0.7, 0.02, HIGH, True)
    _same_bits(out["s"][2:3], [0.0], "KL")
    _same_bits(out["s"][4:], [F32(0.7)], "c")
    _same_bits(out["r"], np.ones(B, dtype=F32), "ratio")


@pytest.mark.gpu
@pytest.mark.parametrize("B,A", [(1025, 3), (64, 33), (64, 0)])
def test_continuous_refusals(rlx, dev, B, A):
    """more than 1024 rows, more than 32 action dimensions, none: the library's error, and nothing is written"""
    import torch
    m = max(A, 1)
    z, one = np.zeros((B, m), dtype=F32), np.ones((B, m), dtype=F32)
    g, l, s, r, a = _sent((B, m), dev), _sent((m,), dev), _sent((5,), dev), _sent((B,), dev), _sent((4,), dev)
    with pytest.raises(RlxError, match="rlx_ppo_kl_continuous_loss"):
        rlx.ppo_kl_continuous_loss(_d(z, dev), m, _d(np.zeros(m, dtype=F32), dev), _d(z, dev),
                                   _d(np.ones(B, dtype=F32), dev), _d(z, dev), _d(one, dev), m, B, A, 0.0, 1.0,
                                   _d(np.array([KLC], dtype=F32), dev), 0.02, HIGH, 1, g, m, l, s, r, a, 0)
    torch.cuda.synchronize()
    for buf in (g, l, s, r, a):
        assert np.all(_h(buf) == SENT)


# ------------------------------------------------------------------------------------------------ the coefficient
def _update(rlx, dev, sums, target, coef):
    c, kl = _d(np.array([coef], dtype=F32), dev), _sent((1,), dev)
    rlx.ppo_kl_coefficient_update(_d(np.asarray(sums, dtype=F32), dev), float(target), c, kl, 0)
    return _h(c)[0], _h(kl)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("target", [0.01, 0.02, 0.003, 0.1])
def test_coefficient_update_thresholds(rlx, dev, target):
    """the mean KL on, one fp32 step inside and one outside both thresholds float32(1.3 target) / float32(0.7 target),
    and well away from them: coefficient and mean bit for bit the restatement's.  (The epoch holds 4 minibatches, so the
    fp32 sums 4 x are exact and the mean is x.)  float32(1.3 * 0.01) is not float32(1.3 * float32(0.01)): the entry point
    takes the target as a double."""
    hi, lo = F32(1.3 * target), F32(0.7 * target)
    up, down = F32(np.inf), F32(-np.inf)
    kls = [hi, np.nextafter(hi, up), np.nextafter(hi, down), lo, np.nextafter(lo, up), np.nextafter(lo, down),
           F32(target), F32(3 * target), F32(0.1 * target), F32(0.0)]
    moved = set()
    for coef in (F32(0.1), F32(0.1) * F32(1.5), F32(1.0) / F32(3.0)):
        for kl in kls:
            sums = np.array([F32(4) * kl, 2.5, -1.0, 4.0], dtype=F32)
            want_c, want_kl = R.kl_coefficient_update(sums, target, coef)
            got_c, got_kl = _update(rlx, dev, sums, target, coef)
            _same_bits([got_c], [want_c], "coefficient at KL %r" % kl)
            _same_bits([got_kl], [want_kl], "mean KL")
            moved.add(int(np.sign(float(want_c) - float(coef))))
    assert moved == {-1, 0, 1}
    c, _ = _update(rlx, dev, [4 * float(hi), 0, 0, 4], target, 0.1)               # ON the threshold: unchanged (strict >)
    _same_bits([c], [F32(0.1)], "on the upper threshold")


@pytest.mark.gpu
def test_coefficient_update_without_mean_output(rlx, dev):
    c = _d(np.array([0.1], dtype=F32), dev)
    rlx.ppo_kl_coefficient_update(_d(np.array([1.0, 0, 0, 4], dtype=F32), dev), 0.01, c, None, 0)
    _same_bits(_h(c), [F32(0.1) * F32(1.5)], "coefficient")


@pytest.mark.gpu
def test_accumulate_over_launches_and_update(rlx, dev):
    """accumulate after k launches = the fp32 sums of the k scalar sets added in launch order (ppo_kl_ref.accumulate); the
    coefficient update then reads that buffer on the device."""
    B, n, k = 64, 6, 4
    acc = _d(np.zeros(4, dtype=F32), dev)
    klc = _d(np.array([KLC], dtype=F32), dev)
    status = _d(np.zeros(1, dtype=np.int32), dev)
    sets = []
    for i in range(k):
        case = R.discrete_case(1000 + i, B, n)
        s = _sent((5,), dev)
        rlx.ppo_kl_discrete_loss(_d(case["logits"], dev), n, _d(case["actions"].astype(np.int32), dev),
                                 _d(case["advantages"], dev), _d(case["old_probs"], dev), n, B, n, 0.01, 1.0, klc, 0.02,
                                 HIGH, 1, None, n, s, None, status, acc, 0)
        sets.append(_h(s))
    want = R.accumulate(sets)
    _same_bits(_h(acc), want, "accumulate")
    assert want[3] == k
    kl = _sent((1,), dev)
    rlx.ppo_kl_coefficient_update(acc, 0.01, klc, kl, 0)
    want_c, want_kl = R.kl_coefficient_update(want, 0.01, KLC)
    _same_bits(_h(klc), [want_c], "coefficient")
    _same_bits(_h(kl), [want_kl], "mean KL")


# ------------------------------------------------------------------------------------------------ captured graph
@pytest.mark.gpu
def test_graph_replay_follows_the_coefficient(rlx, dev):
    """a captured launch replayed after the device scalar kl_coefficient changed gives a fresh launch's results with the
    new value, bit for bit"""
    import torch
    from coach_amd import _rlx
    B, n = 65, 6
    case, refs = _discrete_refs(B, n)
    cutoff = refs[(0.01, 0.5, "above")][0]
    logits, old = _d(case["logits"], dev), _d(case["old_probs"], dev)
    actions, adv = _d(case["actions"].astype(np.int32), dev), _d(case["advantages"], dev)
    klc = _d(np.array([KLC], dtype=F32), dev)
    g, s, r = _sent((B, n), dev), _sent((5,), dev), _sent((B,), dev)
    status = _d(np.zeros(1, dtype=np.int32), dev)

    def launch():
        rlx.ppo_kl_discrete_loss(logits, n, actions, adv, old, n, B, n, 0.01, 0.5, klc, float(cutoff), HIGH, 1, g, n, s, r,
                                 status, None, _rlx.current_stream())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                             # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for value in (KLC, 0.15, 2.5):
        klc.fill_(value)
        for buf in (g, s, r):
            buf.fill_(float(SENT))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [_h(b).copy() for b in (g, s, r)]
        fresh = _run_discrete(rlx, dev, case, n, 0, 0.01, 0.5, value, cutoff, HIGH, True)
        for got, key in zip(replayed, "gsr"):
            _same_bits(got, fresh[key], "replay with kl_coefficient %g: %s" % (value, key))
        _same_bits(replayed[1][4:], [F32(F32(value) + F32(2) * F32(HIGH) * max(F32(0), replayed[1][2] - cutoff))], "c")


@pytest.mark.gpu
def test_coefficient_update_on_the_recorded_sequences(rlx, dev, golden):
    """tests/golden/ppo_kl.npz: the reference's PPOAgent on prescribed KL fetches, three training phases per case.  The
    last epoch's fetches accumulated as the head launch accumulates them (fp32, in minibatch order), then the device
    update: mean KL and coefficient after every phase bit for bit the reference's, the coefficient carried on the device
    from phase to phase."""
    fx = golden("ppo_kl")
    for k in range(int(fx["n_cases"])):
        p = "c%d_" % k
        klc, kl = _d(np.array([fx["initial_coefficient"]], dtype=F32), dev), _sent((1,), dev)
        for phase in range(3):
            sums, _, _ = R.epoch_means(fx[p + "kl"][phase], fx[p + "entropy"][phase])
            rlx.ppo_kl_coefficient_update(_d(sums, dev), float(fx[p + "target_kl"]), klc, kl, 0)
            _same_bits(_h(kl), fx[p + "kl_mean"][phase:phase + 1], "case %d phase %d: mean KL" % (k, phase))
            _same_bits(_h(klc), fx[p + "coefficient"][phase + 1:phase + 2], "case %d phase %d: coefficient" % (k, phase))


@pytest.mark.gpu
def test_coefficient_update_with_nothing_accumulated(rlx, dev):
    """a count of 0 (the update called before any minibatch, or right after a reset): the coefficient is kept and the mean
    KL written is 0, not 0 / 0"""
    c, kl = _update(rlx, dev, [0.0, 0.0, 0.0, 0.0], 0.01, 0.7)
    _same_bits([c], [F32(0.7)], "coefficient")
    _same_bits([kl], [F32(0.0)], "mean KL")
