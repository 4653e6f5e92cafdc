"""The small kernels between the network passes (csrc/actor_critic.hip, the dueling merge of csrc/targets.hip, the norm
and clip of csrc/optim.hip, rlx_act_backward of csrc/gemm.hip), each called by name on inputs chosen to reach its
branches, against the float64 restatement tests/glue_ref.py.

Three kinds of tolerance appear, and each assertion says which one it uses:
  * bit for bit, where the kernel owes it (copies, selections, one fp32 operation, files built without contraction);
  * derived: a bound that follows from the number formats and the operation count, for either rounding order of a
    product-sum that the compiler may or may not contract to an FMA;
  * measured: the worst ulp distance / the smallest integer constant seen on the MI355X over exactly the inputs of the
    test, plus the stated margin -- the figure and its inputs are in the docstring next to the assertion.
Every test prints its figures (`pytest -s`) before it asserts."""
import os
import re

import numpy as np
import pytest

import glue_ref as R

F32, F64 = np.float32, np.float64
U23, U24 = 2.0 ** -23, 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid_cap_elements():
    """elements one trip of a grid-stride kernel covers: kMaxStreamBlocks (csrc/rlx_common.hpp) x 256 threads."""
    text = open(os.path.join(ROOT, "coach_amd", "csrc", "rlx_common.hpp")).read()
    cus = int(re.search(r"constexpr int kCUs = (\d+);", text).group(1))
    per = int(re.search(r"constexpr int kMaxStreamBlocks = kCUs \* (\d+);", text).group(1))
    return cus * per * 256


CAP = _grid_cap_elements()


def _d(x, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _h(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


def _assert_same_bits(got, want, what=""):
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: got %r want %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def _measured(name, value):
    print("MEASURED %s %.6g" % (name, value))


# ------------------------------------------------------------------------------------------------ rlx_copy_2d
#          rows, cols, src_ld, dst_ld, src_off, dst_off
COPY_CASES = [(1, 1, 1, 1, 0, 0),
              (7, 37, 37, 37, 0, 0),            # 259 elements: not a multiple of the 256-thread block
              (7, 37, 50, 37, 0, 0),            # src_ld > cols
              (7, 37, 37, 45, 0, 0),            # dst_ld > cols
              (64, 6, 23, 29, 17, 6),           # a column block of a wider row on both sides (the critic's concat / slice)
              (1031, 513, 520, 517, 3, 2)]      # 528903 elements: the grid-stride loop takes a second trip


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, -1.0, 0.37])
@pytest.mark.parametrize("case", COPY_CASES)
def test_copy_2d(rlx, dev, case, scale):
    """dst[r][c] = scale * src[r][c] is one fp32 multiply: bit for bit equal to np.float32(scale) * src, which is also the
    float64 reference rounded once.  Everything of dst outside the rows x cols block (the padding columns of dst_ld >
    cols, the elements before the offset base pointer) keeps its sentinel."""
    rows, cols, src_ld, dst_ld, src_off, dst_off = case
    if case == COPY_CASES[-1]:
        assert rows * cols > CAP
    rng = np.random.RandomState(rows * 131 + cols)
    src = rng.randn(src_off + rows * src_ld).astype(F32)
    src[rng.rand(src.size) < 0.05] = 0.0
    dst = np.full(dst_off + rows * dst_ld, -777.25, dtype=F32)
    sd, dd = _d(src, dev), _d(dst, dev)
    rlx.copy_2d(sd.data_ptr() + 4 * src_off, src_ld, dd.data_ptr() + 4 * dst_off, dst_ld, rows, cols, scale, 0)
    block = src[src_off:].reshape(rows, src_ld)[:, :cols]
    want = dst.copy()
    want[dst_off:].reshape(rows, dst_ld)[:, :cols] = F32(scale) * block
    _assert_same_bits(_h(dd), want, "copy_2d")
    _assert_same_bits(want[dst_off:].reshape(rows, dst_ld)[:, :cols], R.copy_2d(block, scale).astype(F32), "reference")


# ------------------------------------------------------------------------------------------------ rlx_axpby
AXPBY_FORMS = ["out_of_place", "out_is_x", "out_is_y", "y_none_b0", "y_none_b1", "a0_b1"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", AXPBY_FORMS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, CAP + 3])
def test_axpby(rlx, dev, n, form):
    """out = a x + b y (y may be NULL: the kernel then adds 0 whatever b is).  actor_critic.hip is built with the
    compiler's default contraction, so a x + b y may be one multiply and an FMA or two multiplies and an add; for either
    order |got - exact| <= 2^-23 (|a x| + |b y|): at most two roundings, each of half an ulp of a value no larger than
    |a x| + |b y|.  DERIVED, not measured.  The in-place forms are what nn/networks.py and
    architectures/hip_architecture.py call (out == x); out == y is not used today and is held to the same bound."""
    rng = np.random.RandomState(n % 1000 + len(form))
    x, y = rng.randn(n).astype(F32), rng.randn(n).astype(F32)
    a, b = (0.0, 1.0) if form == "a0_b1" else (0.37, 0.0) if form == "y_none_b0" else (0.37, 1.0) if form == "y_none_b1" \
        else (0.37, -1.25)
    xd, yd = _d(x, dev), _d(y, dev)
    out = _d(np.full(n, -777.25, dtype=F32), dev)
    if form == "out_is_x":
        out = xd
    elif form == "out_is_y":
        out = yd
    rlx.axpby(out, a, xd, b, None if form.startswith("y_none") else yd, n, 0)
    ref, mag = R.axpby(a, x, b, None if form.startswith("y_none") else y)
    err = np.abs(_h(out).astype(F64) - ref)
    _measured("axpby_err_over_bound[%s,%d]" % (form, n), (err / np.maximum(U23 * mag, 1e-300)).max())
    assert np.all(err <= U23 * mag), err.max()
    if form not in ("out_is_x", "out_is_y"):
        _assert_same_bits(_h(xd), x, "x untouched")
    if form != "out_is_y":
        _assert_same_bits(_h(yd), y, "y untouched")


# ------------------------------------------------------------------------------------------------ rlx_exp_rows
EXP_ROWS_WORST_ULP = 0.55   # measured on the MI355X, see test_exp_rows


@pytest.mark.gpu
@pytest.mark.parametrize("batch,A", [(1, 1), (5, 1), (37, 7), (3, 64), (129, 17)])
def test_exp_rows(rlx, dev, batch, A):
    """out[b][a] = exp(log_std[a]) against float64 exp, log_std spread over [-20, 2] with both ends present.
    MEASURED on the MI355X over these five shapes (seeds as below): worst distance 0.548 ulp, at batch 3 x A 64
    (EXP_ROWS_WORST_ULP = 0.55); asserted: at most that plus 1 ulp."""
    rng = np.random.RandomState(batch * 100 + A)
    ls = rng.uniform(-20.0, 2.0, A).astype(F32)
    ls[0] = -20.0
    ls[-1] = 2.0 if A > 1 else ls[-1]
    out = _d(np.full((batch, A), -777.25, dtype=F32), dev)
    rlx.exp_rows(_d(ls, dev), out, batch, A, 0)
    d = R.ulp_distance(_h(out), R.exp_rows(ls, batch))
    _measured("exp_rows_ulp[%d,%d]" % (batch, A), d.max())
    assert d.max() <= EXP_ROWS_WORST_ULP + 1, d.max()


# ------------------------------------------------------------------------------------------------ rlx_min_pair
def _min_pair_inputs(n):
    rng = np.random.RandomState(n)
    q1, q2 = rng.randn(n).astype(F32), rng.randn(n).astype(F32)
    tie = rng.rand(n) < 0.25
    q2[tie] = q1[tie]                                        # ties: the gradient is q1's
    k = np.arange(n)
    q1[k % 7 == 3], q2[k % 7 == 3] = 0.0, -0.0               # +0 vs -0 compare equal: q1's +0 comes out
    q1[k % 7 == 5], q2[k % 7 == 5] = -0.0, 0.0               # ... and q1's -0 here
    if n >= 257:                                             # a NaN of either stream is the minimum (np.minimum keeps it):
        q1[14] = np.nan                                      # of q1 alone: value and gradient are q1's
        q2[22] = np.nan                                      # of q2 alone: q2's
        q1[30] = q2[30] = np.nan                             # of both: q1's
    return q1, q2


@pytest.mark.gpu
@pytest.mark.parametrize("outputs", ["min", "g1", "g2", "all"])
@pytest.mark.parametrize("n", [1, 257, 1000, 1003])
def test_min_pair(rlx, dev, n, outputs):
    """min, and the gradient of its sum scaled by grad_scale, bit for bit (selections, no arithmetic): the tie rule
    (q1 == q2 gives the gradient and the value to q1, so the sign of a zero is q1's); each output pointer alone (the
    other two NULL) and all three together."""
    q1, q2 = _min_pair_inputs(n)
    gs = 1.0 / n
    want = dict(zip(("min", "g1", "g2"), R.min_pair(q1, q2, gs)))
    names = ("min", "g1", "g2") if outputs == "all" else (outputs,)
    bufs = {k: _d(np.full(n, -777.25, dtype=F32), dev) for k in names}
    rlx.min_pair(_d(q1, dev), _d(q2, dev), bufs.get("min"), bufs.get("g1"), bufs.get("g2"), gs, n, 0)
    for k in names:
        _assert_same_bits(_h(bufs[k]), want[k], k)
    if "g1" in bufs and "g2" in bufs:
        assert np.all((_h(bufs["g1"]) != 0) ^ (_h(bufs["g2"]) != 0))
        assert np.all(_h(bufs["g1"])[q1 == q2] == F32(gs))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257, 1000, 1003])
def test_sac_min_targets(rlx, dev, n):
    """rlx_min_pair's three outputs bit for bit, and value_targets = min - logprob: ONE fp32 subtraction, so it equals
    the float64 difference rounded once -- bit for bit as well."""
    q1, q2 = _min_pair_inputs(n)
    logp = (np.random.RandomState(n + 1).randn(n) * 3).astype(F32)
    gs = 1.0 / n
    m, vt, g1, g2 = R.sac_min_targets(q1, q2, logp, gs)
    o = [_d(np.full(n, -777.25, dtype=F32), dev) for _ in range(4)]
    rlx.sac_min_targets(_d(q1, dev), _d(q2, dev), _d(logp, dev), gs, n, o[0], o[1], o[2], o[3], 0)
    for got, want, what in zip(o, (m, vt.astype(F32), g1, g2), ("min", "value_targets", "g1", "g2")):
        _assert_same_bits(_h(got), want, what)


# ------------------------------------------------------------------------------------------------ dueling merge
def _dueling_inputs(B, A, offset):
    rng = np.random.RandomState(B * 64 + A)
    return rng.randn(B).astype(F32), (rng.randn(B, A) + offset).astype(F32)


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0.0, 1e4])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("A", [1, 2, 6, 18, 51])
def test_dueling_combine(rlx, dev, A, B, offset):
    """q = V + (A - mean A).  targets.hip is built with contraction off and one thread adds a row in index order, so
    the result is bit for bit the numpy fp32 restatement that adds in index order; and it is within
    A 2^-24 (|v| + sum |adv|) of the float64 value (DERIVED: A - 1 additions of partial sums no larger than sum |adv|,
    then a division, a subtraction and an addition, each rounding a value no larger than |v| + sum |adv|).  offset
    1e4: the advantages share a large constant that the mean subtraction cancels."""
    v, adv = _dueling_inputs(B, A, offset)
    q = _d(np.full((B, A), -777.25, dtype=F32), dev)
    rlx.dueling_combine(_d(v, dev), _d(adv, dev), B, A, q, 0)
    _assert_same_bits(_h(q), R.dueling_combine_f32(v, adv), "q")
    bound = A * U24 * (np.abs(v.astype(F64)) + np.abs(adv.astype(F64)).sum(axis=1))[:, None]
    err = np.abs(_h(q).astype(F64) - R.dueling_combine(v, adv))
    _measured("dueling_fwd_err_over_bound[%d,%d,%g]" % (A, B, offset), (err / bound).max())
    assert np.all(err <= bound), (err / bound).max()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dense", "one_hot", "dense_offset"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("A", [1, 2, 6, 18, 51])
def test_dueling_combine_backward(rlx, dev, A, B, kind):
    """dV = sum_a dq, dAdv = dq - mean_a dq: bit for bit the index-order fp32 restatement, and within
    A 2^-24 sum |dq| of float64 (DERIVED as for the forward).  one_hot: one non-zero per row, the DQN loss's gradient
    (dV is then that entry exactly)."""
    rng = np.random.RandomState(B * 64 + A + 7)
    dq = rng.randn(B, A).astype(F32)
    if kind == "one_hot":
        keep = rng.randint(0, A, B)
        dq = np.where(np.arange(A)[None, :] == keep[:, None], dq, F32(0)).astype(F32)
    elif kind == "dense_offset":
        dq = (dq + F32(1e4)).astype(F32)
    dv, dadv = _d(np.full(B, -777.25, dtype=F32), dev), _d(np.full((B, A), -777.25, dtype=F32), dev)
    rlx.dueling_combine_backward(_d(dq, dev), B, A, dv, dadv, 0)
    s32, d32 = R.dueling_combine_backward_f32(dq)
    _assert_same_bits(_h(dv), s32, "dV")
    _assert_same_bits(_h(dadv), d32, "dAdv")
    s64, d64 = R.dueling_combine_backward(dq)
    bound = A * U24 * np.abs(dq.astype(F64)).sum(axis=1)
    assert np.all(np.abs(_h(dv).astype(F64) - s64) <= bound)
    assert np.all(np.abs(_h(dadv).astype(F64) - d64) <= bound[:, None])
    if kind == "one_hot":
        _assert_same_bits(_h(dv), dq[np.arange(B), keep], "dV of a one-hot row")


# ------------------------------------------------------------------------------------------------ norm and clip
GLOBAL_NORM_WORST_ULP = 0.5    # measured on the MI355X, see test_global_norm
assert (GLOBAL_NORM_WORST_ULP + 1) * U23 <= 1e-5      # no looser than tests/test_nn.py's rtol


@pytest.mark.gpu
@pytest.mark.parametrize("workspace", [1024, 3, 1])
@pytest.mark.parametrize("n", [1, 255, 257, 1024 * 256 + 3])
def test_global_norm(rlx, dev, n, workspace):
    """sqrt(sum x^2) against float64.  workspace 3 and 1 are smaller than the natural number of partial sums (one per
    256 elements, at most 1024) for n = 1024 * 256 + 3, workspace 1 for n = 257 as well: the `parts > workspace_floats`
    clamp is taken; the workspace beyond the partials in use keeps its sentinel.
    MEASURED on the MI355X over these twelve cases (unit normal x, seeds as below): worst distance 0.496 ulp of the
    norm, at n = 257 with a workspace of 3 (GLOBAL_NORM_WORST_ULP = 0.5); asserted: at most that plus 1 ulp = 1.8e-7
    relative, inside the 1e-5 of tests/test_nn.py."""
    rng = np.random.RandomState(n % 997 + workspace)
    x = rng.randn(n).astype(F32)
    ws = _d(np.full(1024 + 8, -777.25, dtype=F32), dev)
    norm = _d(np.full(1, -777.25, dtype=F32), dev)
    rlx.global_norm(_d(x, dev), n, norm, ws, workspace, 0)
    parts = min((n + 255) // 256, 1024, workspace)
    _assert_same_bits(_h(ws)[parts:], np.full(1024 + 8 - parts, -777.25, dtype=F32), "workspace beyond the partials")
    d = R.ulp_distance(_h(norm), R.global_norm(x))
    _measured("global_norm_ulp[%d,%d]" % (n, workspace), d.max())
    assert d.max() <= GLOBAL_NORM_WORST_ULP + 1, d.max()


def _clip(rlx, dev, g, norm, clip):
    gd = _d(g, dev)
    rlx.clip_by_global_norm(gd, g.size, _d(np.array([norm], dtype=F32), dev), float(clip), 0)
    return _h(gd)


def _device_norm(rlx, dev, g):
    norm, ws = _d(np.zeros(1, dtype=F32), dev), _d(np.zeros(1024, dtype=F32), dev)
    rlx.global_norm(_d(g, dev), g.size, norm, ws, 1024, 0)
    return F32(_h(norm)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1000, 1024 * 256 + 3])
@pytest.mark.parametrize("case", ["below", "equal", "far_above", "above", "zero"])
def test_clip_by_global_norm_finite(rlx, dev, case, n):
    """grads *= clip * min(1 / norm, 1 / clip) with the norm rlx_global_norm wrote.  optim.hip is built with contraction
    off: for every finite norm the result is bit for bit numpy fp32 evaluating that expression in that order.
      below      norm < clip: the scale is clip * (1 / clip), exactly 1 for the clip values used here (40, or a power
                 of two above a larger norm; checked on the CPU first), and the gradient buffer is unchanged bit for bit
      equal      clip == norm exactly: the scale is norm * (1 / norm), 1 up to its two roundings -- within one ulp of g
      far_above  norm >> clip: the clipped gradient's norm, recomputed in float64, is clip up to the relative error of
                 the device norm (GLOBAL_NORM_WORST_ULP + 1 ulp) and four more roundings (1 / norm, the product with
                 clip, the product with g, float32(clip))
      above      norm = 1.7 clip
      zero       an all-zero gradient with norm 0: 1 / 0 = inf loses the min, the scale is 1, the buffer stays zero"""
    rng = np.random.RandomState(n % 997)
    g = np.zeros(n, dtype=F32) if case == "zero" else rng.randn(n).astype(F32)
    norm = _device_norm(rlx, dev, g)
    roomy = F32(40.0) if norm < 40 else F32(2.0) ** np.ceil(np.log2(norm) + 1)
    clip = {"below": roomy, "equal": norm, "far_above": F32(0.5), "above": norm / F32(1.7),
            "zero": F32(40.0)}[case]
    clip = F32(clip)
    got = _clip(rlx, dev, g, norm, clip)
    _assert_same_bits(got, R.clip_by_global_norm_f32(g, norm, clip), "the kernel's expression in numpy fp32")
    assert np.all(np.isfinite(got))
    if case in ("below", "zero"):
        assert clip * (F32(1) / clip) == F32(1)          # a condition on the test's clip value, not on the kernel
        assert norm < clip
        _assert_same_bits(got, g, "unchanged")
    elif case == "equal":
        assert np.all(np.abs(got - g) <= np.spacing(np.abs(g)))
    else:
        assert norm > clip
        new = R.global_norm(got)
        rel = abs(new - float(clip)) / float(clip)
        _measured("clip_norm_rel[%s,%d]" % (case, n), rel)
        assert rel <= (GLOBAL_NORM_WORST_ULP + 1 + 4) * U23, rel
        err = np.abs(got.astype(F64) - R.clip_by_global_norm(g, norm, clip))
        assert np.all(err <= 4 * U24 * np.abs(g.astype(F64)) * float(clip) / float(norm))


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["nan", "inf"])
def test_clip_by_global_norm_non_finite(rlx, dev, norm):
    """PINNED: tf.clip_by_global_norm's minimum(1 / norm, 1 / clip) is (y < x) ? y : x, so a NaN norm makes every gradient
    NaN -- the reference's behaviour and oracle/agents.py:205-210's (Python's min keeps a NaN first argument), and what
    include/rlx.h promises; the kernel used fminf, which drops the NaN and passed the buffer through unscaled.  An
    infinite norm gives a scale of 0: finite entries become zeros of their own sign (an infinite entry would give NaN)."""
    rng = np.random.RandomState(3)
    g = rng.randn(1000).astype(F32)
    got = _clip(rlx, dev, g, F32(norm), F32(40.0))
    if norm == "nan":
        assert np.all(np.isnan(got))
        assert np.all(np.isnan(R.clip_by_global_norm(g, F32(norm), 40.0)))
    else:
        _assert_same_bits(got, g * F32(0), "scale 0")
        _assert_same_bits(got, R.clip_by_global_norm_f32(g, F32(norm), F32(40.0)), "numpy fp32")


# ------------------------------------------------------------------------------------------------ rlx_act_backward
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257, CAP + 5])
@pytest.mark.parametrize("kind", ["none", "relu", "tanh"])
def test_act_backward(rlx, dev, kind, n):
    """dy *= act'(y) in place, act' written through the activation's output.  none and relu multiply by exactly 1 or 0:
    bit for bit (relu: y = +0, -0 and negative denormals give 0 -- of dy's sign --, a positive denormal gives dy).
    tanh: dy (1 - y^2); gemm.hip may contract 1 - y y to an FMA, so DERIVED |got - exact| <= 2^-23 |dy|: 1 - y^2 <= 1
    is rounded once (FMA) or twice (y^2 <= 1, then the difference), each at most 2^-25 absolute, and the product with
    dy once more -- 2^-24 |dy| (2^-1 + 2^-1 + 1) < 2^-23 |dy|.  y = +-1 exactly gives 0."""
    from coach_amd import _rlx
    rng = np.random.RandomState(n % 991 + len(kind))
    dy = rng.randn(n).astype(F32)
    y = np.tanh(rng.randn(n) * 2).astype(F32) if kind == "tanh" else np.maximum(rng.randn(n), 0).astype(F32)
    special = [0.0, -0.0, 1e-40, -1e-40, 1.0, -1.0, 1.4e-45, -1.4e-45]
    for i, s in enumerate(special):
        y[i::64][:max(1, n // 640)] = F32(s)
    dyd = _d(dy, dev)
    rlx.act_backward(dyd, _d(y, dev), n, _rlx.ACT[kind], 0)
    got = _h(dyd)
    if kind == "none":
        _assert_same_bits(got, dy, "identity")
    elif kind == "relu":
        _assert_same_bits(got, dy * np.where(y > 0, F32(1), F32(0)), "relu")
    else:
        err = np.abs(got.astype(F64) - R.act_backward(dy, y, kind))
        assert np.all(err <= U23 * np.abs(dy.astype(F64))), (err / np.abs(dy)).max()
        assert np.all(got[np.abs(y) == 1] == 0)


# ------------------------------------------------------------------------------------------------ SACPolicyHead
# measured on the MI355X, see test_sac_policy_head / test_sac_policy_head_backward
SAC_ACT_WORST_ULP = 1.31
SAC_LOGP_C_T = 4
SAC_LOGP_C_G = 4
SAC_BWD_C = 4
SAC_SHAPES = [(B, A) for A in (1, 3, 17, 64) for B in (1, 63, 65, 256)]
CATEGORY_SHAPE_MIN_B = 63            # the shares (a)-(f) are asserted for every shape with at least this many rows


def logp_bound(fwd, c_t=SAC_LOGP_C_T, c_g=SAC_LOGP_C_G):
    """per row: sum_a c_t 2^-24 (2|t| + 1) / (1 - t^2 + eps)  +  c_g 2^-24 sum_a (z^2 / 2 + |ls| + 0.92)"""
    return c_t * U24 * fwd["logp_t_unit"] + c_g * U24 * fwd["logp_g_unit"]


def assert_categories(fwd, B):
    """A condition on the INPUTS, from the reference alone: each of (a) interior, (b) below -20, (c) above 2, (d) exactly
    -20 and exactly 2, (e) |raw| in [4, 9], (f) |raw| > 10 holds at least 5% of the elements."""
    if B < CATEGORY_SHAPE_MIN_B:
        return
    shares = R.sac_head_categories(fwd)
    for k in ("interior", "below", "above", "near_sat", "saturated"):
        assert shares[k] >= R.CATEGORY_MIN_SHARE, (k, shares)
    assert shares["lo_bound"] + shares["hi_bound"] >= R.CATEGORY_MIN_SHARE and shares["lo_bound"] > 0 and \
        shares["hi_bound"] > 0, shares


def _head_forward(rlx, dev, x, normals, B, A, ld, names):
    size = dict(mean=(B, A), log_std=(B, A), raw=(B, A), act=(B, A), logp=(B,))
    bufs = {k: _d(np.full(size[k], -777.25, dtype=F32), dev) for k in names}
    rlx.sac_policy_head(_d(x, dev), ld, _d(normals, dev), B, A, bufs.get("mean"), bufs.get("log_std"), bufs.get("raw"),
                        bufs.get("act"), bufs.get("logp"), 0)
    return {k: _h(v) for k, v in bufs.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("B,A", SAC_SHAPES)
def test_sac_policy_head(rlx, dev, B, A, pad):
    """SACPolicyHead forward on glue_ref.sac_head_case: log-std inside, below, above and exactly on [-20, 2], samples in
    the interior, near saturation and saturated (shares asserted on the CPU first), ld = 2A and 2A + 5, all five outputs
    together and each alone (the others NULL: bit for bit what the joint launch wrote).
      mean, log_std   bit for bit (a copy; a clip)
      raw             DERIVED |got - exact| <= 2^-23 (|mu| + |sd e|): expf within an ulp, the product and the sum (or one
                      FMA) each round a value no larger than |mu| + |sd e|
      act             ulp distance to float64 tanh of the device's own raw.  MEASURED on the MI355X over all 32 cases:
                      worst 1.305 ulp, at B 256 x A 64, ld = 2A + 5 (SAC_ACT_WORST_ULP = 1.31); asserted <= that + 1.
                      |act| <= 1 everywhere
      logp            against the float64 log-probability OF THE DEVICE'S raw (sac_head.py:91 evaluates log_prob at the
                      sampled fp32 tensor; raw itself is held to its own bound above), per row within logp_bound():
                      the squash term's condition number times c_t, the Gaussian terms' magnitude times c_g.
                      MEASURED on the MI355X over all 32 cases with c_t = c_g = c: the worst row needs c = 1.49 (B 256 x
                      A 1, ld = 2A), so the smallest integers are c_t = c_g = 2; doubled for another summation order:
                      SAC_LOGP_C_T = SAC_LOGP_C_G = 4.  On the plain rows the worst error seen is 4.5e-7 max(1, |logp|).  tests/test_glue_ref.py asserts that this bound
                      stays below 1e-5 max(1, |logp|) on the plain rows."""
    ld = 2 * A + pad
    x, normals, plain = R.sac_head_case(np.random.RandomState(B * 1000 + A * 10 + pad), B, A, ld)
    exact = R.sac_head_forward(x, normals, A)
    assert_categories(exact, B)
    names = ("mean", "log_std", "raw", "act", "logp")
    got = _head_forward(rlx, dev, x, normals, B, A, ld, names)
    for k in names:                                     # each output alone
        alone = _head_forward(rlx, dev, x, normals, B, A, ld, (k,))
        _assert_same_bits(alone[k], got[k], k + " alone")
    _assert_same_bits(got["mean"], x[:, :A], "mean")
    _assert_same_bits(got["log_std"], np.clip(x[:, A:2 * A], F32(-20), F32(2)), "log_std")
    _assert_same_bits(got["log_std"], exact["log_std"].astype(F32), "log_std reference")
    err = np.abs(got["raw"].astype(F64) - exact["raw"])
    _measured("sac_raw_err_over_bound[%d,%d,%d]" % (B, A, pad), (err / (U23 * exact["raw_mag"])).max())
    assert np.all(err <= U23 * exact["raw_mag"]), (err / (U23 * exact["raw_mag"])).max()
    at = R.sac_head_forward(x, normals, A, raw=got["raw"])           # downstream of the device's own sample
    d = R.ulp_distance(got["act"], at["act"])
    _measured("sac_act_ulp[%d,%d,%d]" % (B, A, pad), d.max())
    assert d.max() <= SAC_ACT_WORST_ULP + 1, d.max()
    assert np.all(np.abs(got["act"]) <= 1)
    lerr = np.abs(got["logp"].astype(F64) - at["logp"])
    unit = U24 * (at["logp_t_unit"] + at["logp_g_unit"])
    _measured("sac_logp_c[%d,%d,%d]" % (B, A, pad), (lerr / unit).max())
    if plain.any():
        _measured("sac_logp_plain_rel[%d,%d,%d]" % (B, A, pad), (lerr[plain] / np.maximum(1, np.abs(at["logp"][plain]))).max())
    bound = logp_bound(at)
    assert np.all(lerr <= bound), (lerr / bound).max()


BWD_COMBOS = [(lw, aw, acc) for lw in (0.0, 1.0) for aw in (False, True) for acc in (0, 1)]


def _head_backward(rlx, dev, x, normals, B, A, ld, ld_grad, lw, aw, scale, prefill, acc):
    d_out = _d(prefill, dev)
    rlx.sac_policy_head_backward(_d(x, dev), ld, _d(normals, dev), B, A, lw, None if aw is None else _d(aw, dev), scale,
                                 d_out, ld_grad, acc, 0)
    return _h(d_out)


@pytest.mark.gpu
@pytest.mark.parametrize("lw,with_aw,acc", BWD_COMBOS)
@pytest.mark.parametrize("B,A", SAC_SHAPES)
def test_sac_policy_head_backward(rlx, dev, B, A, lw, with_aw, acc):
    """SACPolicyHead backward on the same input categories, ld = 2A + 5 and ld_grad = 2A + 3 (the padding columns of the
    gradient keep their sentinel), logp_weight 0 / 1, action_weights NULL / random, accumulate 0 / 1 onto a RANDOM
    d_out.
    Exact:   d_ls is exactly 0 (accumulate: d_out is exactly what it was) wherever log_std lies below -20 or above 2;
             exactly on -20 and on 2 it is not, wherever the reference gradient stands clear of its error bound (and,
             when it is accumulated, of the spacing of the sum it is added to);
             d_mu is bit for bit what the kernel gives when the log-std input is already clipped.
    Bounded: elsewhere |got - float64| <= SAC_BWD_C 2^-24 unit, unit = glue_ref.sac_head_backward's first-order error
             model (the condition number 1 / (1 - t^2 + eps) enters squared through 2 t u / (u + eps)), plus one rounding
             of the accumulated sum.  MEASURED on the MI355X over all 128 cases: the worst element needs a constant of
             0.98 for d_mu and 1.61 for d_ls (B 63 x A 64, logp_weight 1, no action_weights, accumulate), so the
             smallest integer is 2; doubled: SAC_BWD_C = 4."""
    ld, ld_grad = 2 * A + 5, 2 * A + 3
    rng = np.random.RandomState(B * 1000 + A * 10 + int(lw) * 4 + with_aw * 2 + acc)
    x, normals, plain = R.sac_head_case(rng, B, A, ld)
    assert_categories(R.sac_head_forward(x, normals, A), B)
    aw = rng.randn(B, A).astype(F32) if with_aw else None
    scale = -1.0 if not acc else -0.75
    prefill = rng.randn(B, ld_grad).astype(F32) if acc else np.full((B, ld_grad), -777.25, dtype=F32)
    prefill[:, 2 * A:] = -777.25
    ref = R.sac_head_backward(x, normals, A, lw, aw, scale)
    got = _head_backward(rlx, dev, x, normals, B, A, ld, ld_grad, lw, aw, scale, prefill, acc)
    _assert_same_bits(got[:, 2 * A:], prefill[:, 2 * A:], "padding columns of d_mu_logsig")
    base = prefill[:, :2 * A].astype(F64) if acc else np.zeros((B, 2 * A))
    g_mu, g_ls = got[:, :A], got[:, A:2 * A]
    clipped = ref["below"] | ref["above"]
    want_clipped = prefill[:, A:2 * A][clipped] if acc else np.zeros(clipped.sum(), dtype=F32)
    _assert_same_bits(g_ls[clipped], want_clipped, "d_ls where the clip is active")
    clear = ref["on_bound"] & (np.abs(ref["d_ls"]) > SAC_BWD_C * U24 * ref["ls_unit"] + 4 * U24 * np.abs(base[:, A:] + ref["d_ls"]))
    assert np.all(g_ls[clear] != prefill[:, A:2 * A][clear] if acc else g_ls[clear] != 0)
    if lw and B >= CATEGORY_SHAPE_MIN_B:
        assert clear.any()                                 # -logp_weight / B is always there
    xc = x.copy()
    xc[:, A:2 * A] = np.clip(x[:, A:2 * A], F32(-20), F32(2))
    unclipped = _head_backward(rlx, dev, xc, normals, B, A, ld, ld_grad, lw, aw, scale, prefill, acc)
    _assert_same_bits(g_mu, unclipped[:, :A], "d_mu does not see the clip")
    for what, g, r, unit, b in (("d_mu", g_mu, ref["d_mu"], ref["mu_unit"], base[:, :A]),
                                ("d_ls", g_ls, ref["d_ls"], ref["ls_unit"], base[:, A:])):
        err = np.abs(g.astype(F64) - (b + r))
        one = U24 * (unit + np.abs(b + r)) + 1e-45
        _measured("sac_bwd_c[%s,%d,%d,%g,%d,%d]" % (what, B, A, lw, with_aw, acc), (err / one).max())
        bound = SAC_BWD_C * U24 * unit + U24 * np.abs(b + r) + 1e-45
        assert np.all(err <= bound), (what, (err / bound).max())
