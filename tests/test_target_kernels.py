"""csrc/targets.hip, every entry point called by name and compared with tests/targets_ref.py: rlx_dqn_targets,
rlx_dqn_head_loss, rlx_dqn_head_loss_backward, rlx_ac_td_targets, rlx_td3_smooth_actions, rlx_ac_merge_inputs and
rlx_sac_value_targets.

targets.hip is built without contraction, so the row arithmetic is the reference's sequence of correctly rounded operations:
targets, |TD errors|, dQ and the fp32 loss are compared BIT FOR BIT (a NaN where the reference has a NaN).  The loss is also
held to the derived bound of its summation order against the float64 mean (targets_ref.loss_bound), and dW, db, dx of the
one-launch form to order-independent bounds of the float64 products (targets_ref.head_backward).  Nothing is measured.

Every buffer a kernel writes is the interior of a guarded allocation filled with 0xA5 (test_frontend_kernels.Guarded): the
guards, the padding of pitched rows, the rows of a refused action and every input must hold the bytes they held.

Not covered, because no comparison of outputs can see it: that the one-launch form writes dQ, the TD errors and the loss
ONCE (only its first workgroup does).  Every workgroup computes the same rows, so a second writer would store the same bits.

The one comparison left out: dq[b][a_b] of a row that is both Huber and NaN-error: the kernels' clamp gives -1
there, numpy's clip gives NaN, and the reference framework's own gradient is not established.  The NaN loss is pinned."""
import ctypes
import itertools

import numpy as np
import pytest

import targets_ref as R
from test_frontend_kernels import FILL, Guarded, same_bits

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DISCOUNT = 0.99
NAN, INF = np.nan, np.inf


def _measured(name, value):
    print("MEASURED %s %.6g" % (name, value))


def _tdtype(dt):
    import torch
    return {np.dtype(F32): torch.float32, np.dtype(F64): torch.float64, np.dtype(np.int32): torch.int32,
            np.dtype(np.uint8): torch.uint8}[np.dtype(dt)]


def _sentinel(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, dtype=np.uint8).view(dtype).reshape(shape)


class Inputs(object):
    """guarded device copies of the arrays a call reads; unchanged() holds every byte of them to what was sent"""

    def __init__(self, dev, **arrays):
        self.sent, self.g = {}, {}
        for k, a in arrays.items():
            if a is None:
                continue
            a = np.ascontiguousarray(a)
            self.sent[k] = a
            self.g[k] = Guarded(a.nbytes, dev, _tdtype(a.dtype), init=a.ravel())

    def __getitem__(self, k):
        return self.g[k].t if k in self.g else None

    def unchanged(self):
        for k, g in self.g.items():
            assert np.array_equal(g.numpy().view(np.uint8), self.sent[k].ravel().view(np.uint8)), "input %s was written" % k
            g.check_guards()


def _out(shape, dtype, dev):
    return Guarded(int(np.prod(shape)) * np.dtype(dtype).itemsize, dev, _tdtype(dtype))


def _pitch(m, ld, pad=NAN):
    out = np.full((m.shape[0], ld), pad, dtype=m.dtype)
    out[:, :m.shape[1]] = m
    return out


# ------------------------------------------------------------------------------------------------ row contents

class Rows(object):
    """A batch for the three DQN entry points: random finite rows, and from row 1 on the planted ones (as many as fit;
    row 0 always stays an ordinary row).  nonfinite: +-inf in q_next under done (0 * inf = NaN) and NaN in the selector row.
    ddqn: a separate selector; otherwise the target net selects and the selector rows below are rows of q_next."""

    def __init__(self, B, A, seed, nonfinite=False, ddqn=False, bad_actions=True):
        rng = np.random.RandomState(1000 * seed + 31 * B + A)
        self.B, self.A, self.ddqn = B, A, ddqn
        self.q = rng.randn(B, A).astype(F32)
        self.q_next = rng.randn(B, A).astype(F32)
        self.q_sel = rng.randn(B, A).astype(F32) if ddqn else None
        self.actions = rng.randint(0, A, size=B).astype(np.int32)
        self.rewards = (2 * rng.randn(B)).astype(F32)
        self.dones = (rng.rand(B) < 0.3).astype(np.uint8)
        self.weights = rng.rand(B) + 0.1
        sel = self.q_sel if ddqn else self.q_next
        self.planted = {}

        def selector(b, vals):                        # not done: the selected column reaches the target
            row = np.full(max(A, len(vals)), -5.0, dtype=F32)
            row[:len(vals)] = vals
            sel[b], self.dones[b] = row[:A], 0

        def first(b):
            sel[b], self.dones[b] = -1.0, 0
            sel[b, 0] = 7.0

        def last(b):
            sel[b], self.dones[b] = -1.0, 0
            sel[b, A - 1] = 7.0

        def done(v):
            def f(b):
                self.dones[b] = v
            return f

        def big(b):                                   # 1e8 + 0.99 * 1e-3 in float64, rounded once
            self.rewards[b], self.dones[b] = 1e8, 0
            self.q_next[b] = 1e-3
            self.q[b, self.actions[b]] = 1e-3

        def boundary(b):
            # y64 = 1 + 0.99 * v lies just above the middle of [1, 1 + 2^-23]: fp32(y64) = 1 + 2^-23, so e = q - y32 is
            # -2^-23, while a difference taken in float64 and rounded afterwards is about -2^-24
            v = F32(2.0 ** -24 / DISCOUNT)
            while 1.0 + DISCOUNT * F64(v) <= 1.0 + 2.0 ** -24:
                v = np.nextafter(v, F32(1))
            self.rewards[b], self.dones[b] = 1.0, 0
            self.q_next[b] = v
            if ddqn:
                sel[b] = 0.0
            self.q[b, self.actions[b]] = 1.0
            y64 = 1.0 + DISCOUNT * F64(v)
            assert F32(y64) == F32(1 + 2.0 ** -23) and F32(1.0 - y64) != F32(1) - F32(y64)

        def unit_error(sign):
            def f(b):                                 # done: y = 2 exactly; q = 3 or 1: |e| is exactly 1
                self.rewards[b], self.dones[b] = 2.0, 1
                self.q[b, self.actions[b]] = 2.0 + sign
            return f

        def weight(v):
            def f(b):
                self.weights[b] = v
                assert F64(F32(v)) != v
            return f

        def action(v):
            def f(b):
                self.actions[b] = v
            return f

        def inf_done(v, d):
            def f(b):
                self.q_next[b], self.dones[b] = v, d
            return f

        plant = [("tie", lambda b: selector(b, [2, 2, 1])), ("zeros+-", lambda b: selector(b, [0.0, -0.0, -1])),
                 ("zeros-+", lambda b: selector(b, [-0.0, 0.0, -1])), ("first", first), ("last", last),
                 ("done0", done(0)), ("done1", done(1)), ("done255", done(255)), ("big", big), ("boundary", boundary),
                 ("e=+1", unit_error(1.0)), ("e=-1", unit_error(-1.0)), ("w=0.1", weight(0.1)), ("w=1/3", weight(1.0 / 3.0))]
        if bad_actions:
            plant += [("a=-1", action(-1)), ("a=A", action(A))]
        if nonfinite:
            plant = [("+inf,done", inf_done(INF, 1)), ("-inf,done", inf_done(-INF, 255)),
                     ("nan mid", lambda b: selector(b, [1, NAN, 3])), ("nan first", lambda b: selector(b, [NAN, 3, NAN]))] + plant
        for i, (name, f) in enumerate(plant):
            if 1 + i >= B:
                break
            f(1 + i)
            self.planted[name] = 1 + i
        self._ref = {}

    def ref(self, huber, weighted, grad_scale):
        """the reference, computed once per variant and shared by every layout that variant runs in"""
        key = (huber, weighted, grad_scale)
        if key not in self._ref:
            r = R.dqn_head_loss(self.q, self.q_next, self.q_sel, self.actions, self.rewards, self.dones,
                                self.weights if weighted else None, DISCOUNT, huber, grad_scale)
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            # the generator's promise: few rows are left out of the dq comparison, and an ordinary row is always there
            assert r["nan_huber"].sum() <= 4
            assert (r["valid"] & np.isfinite(r["td_errors"])).any()
            self._ref[key] = r
        return self._ref[key]


def _taken(c, rows):
    return rows, c.actions[rows]


# ------------------------------------------------------------------------------------------------ rlx_dqn_targets

@pytest.mark.parametrize("nonfinite", [False, True], ids=["finite", "nonfinite"])
@pytest.mark.parametrize("A", [1, 2, 5, 18])
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_dqn_targets(rlx, dev, B, A, nonfinite):
    for ddqn, with_errors in itertools.product((False, True), (False, True)):
        c = Rows(B, A, 1, nonfinite=nonfinite, ddqn=ddqn)
        want_tt, want_err, want_status = R.dqn_targets(c.q_next, c.q_sel, c.q, c.actions, c.rewards, c.dones, DISCOUNT)
        i = Inputs(dev, q_next=c.q_next, q_sel=c.q_sel, actions=c.actions, rewards=c.rewards, dones=c.dones)
        tt = Guarded(c.q.nbytes, dev, _tdtype(F32), init=c.q.ravel())
        err = _out(B, F64, dev)
        st = Guarded(4, dev, _tdtype(np.int32), init=np.zeros(1, dtype=np.int32))
        rlx.dqn_targets(i["q_next"], i["q_sel"], tt.t, i["actions"], i["rewards"], i["dones"], DISCOUNT, B, A,
                        err.t if with_errors else None, st.t, 0)
        what = (B, A, ddqn, with_errors)
        assert same_bits(tt.numpy().reshape(B, A), want_tt), what
        ok = (c.actions >= 0) & (c.actions < A)
        exp_err = _sentinel(B, F64)
        if with_errors:
            exp_err[ok] = want_err[ok]
        assert same_bits(err.numpy(), exp_err), what
        assert int(st.numpy()[0]) == want_status, what
        if nonfinite and B > 4 and A >= 2:
            b = c.planted["nan mid"]                  # the first NaN of the selector row wins: column 1
            assert np.isnan(want_tt[b, c.actions[b]]) != ddqn
        i.unchanged()
        for g in (tt, err, st):
            g.check_guards()


# ------------------------------------------------------------------------------------------------ rlx_dqn_head_loss

def _layouts(A):
    """name -> (ld_q, ld_next, ld_dq, ld_targets): contiguous; A + 5 on every matrix; four different pitches"""
    return {"contiguous": (A, A, A, A), "pitched": (A + 5,) * 4, "mixed": (A + 2, A + 5, A + 1, A + 3)}


def _run_head_loss(rlx, dev, c, huber, weighted, gs, layout, null):
    """one launch of rlx_dqn_head_loss, everything it writes compared with the reference.  -> |loss error| / bound"""
    B, A = c.B, c.A
    r = c.ref(huber, weighted, gs)
    ld_q, ld_next, ld_dq, ld_t = layout
    i = Inputs(dev, q=_pitch(c.q, ld_q), q_next=_pitch(c.q_next, ld_next),
               q_sel=None if c.q_sel is None else _pitch(c.q_sel, ld_next), actions=c.actions, rewards=c.rewards,
               dones=c.dones, weights=c.weights if weighted else None)
    dq, tt = _out((B, ld_dq), F32, dev), _out((B, ld_t), F32, dev)
    err, loss = _out(B, F64, dev), _out(1, F32, dev)
    st = Guarded(4, dev, _tdtype(np.int32), init=np.zeros(1, dtype=np.int32))
    rlx.dqn_head_loss(i["q"], ld_q, i["q_next"], i["q_sel"], ld_next, i["actions"], i["rewards"], i["dones"], i["weights"],
                      DISCOUNT, B, A, huber, gs, dq.t, ld_dq, None if null == "td_errors" else err.t,
                      None if null == "td_targets" else tt.t, ld_t, None if null == "loss" else loss.t, st.t, 0)
    what = (B, A, huber, weighted, gs, layout, null)
    ok = r["valid"]
    # rows of a refused action and the padding keep the sentinel (rlx.h: the row's dq is left unwritten)
    exp_dq, exp_tt, exp_err = _sentinel((B, ld_dq), F32), _sentinel((B, ld_t), F32), _sentinel(B, F64)
    exp_dq[ok, :A] = r["dq"][ok]
    got_dq = dq.numpy().reshape(B, ld_dq).copy()
    left_out = _taken(c, np.nonzero(r["nan_huber"])[0])
    got_dq[left_out] = 0
    exp_dq[left_out] = 0
    assert same_bits(got_dq, exp_dq), ("dq",) + what
    if null != "td_targets":
        exp_tt[ok, :A] = r["td_targets"][ok]
    assert same_bits(tt.numpy().reshape(B, ld_t), exp_tt), ("td_targets",) + what
    if null != "td_errors":
        exp_err[ok] = r["td_errors"][ok]
    assert same_bits(err.numpy(), exp_err), ("td_errors",) + what
    assert int(st.numpy()[0]) == r["status"], what
    ratio = 0.0
    if null == "loss":
        assert same_bits(loss.numpy(), _sentinel(1, F32)), what
    else:
        got = loss.numpy()
        assert same_bits(got, np.array([r["loss_f32"]], dtype=F32)), ("loss", got, r["loss_f32"]) + what
        if np.isfinite(r["loss_f64"]):
            ratio = abs(F64(got[0]) - r["loss_f64"]) / r["loss_bound"]
            assert ratio <= 1.0, ("loss", got, r["loss_f64"], r["loss_bound"]) + what
        else:
            assert np.isnan(r["loss_f64"]) and np.isnan(got[0]), what
    i.unchanged()
    for g in (dq, tt, err, loss, st):
        g.check_guards()
    return ratio


VARIANTS = list(itertools.product((0, 1), (False, True), (1.0, 0.37)))      # huber, weighted, grad_scale
NULLS = [None, "td_errors", "td_targets", "loss"]


@pytest.mark.parametrize("A", [1, 3, 4, 18])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 100, 1000, 1024])
def test_dqn_head_loss_finite(rlx, dev, B, A):
    """block sizes 64 .. 1024, batches that leave the upper tree entries at zero; every layout x Huber / MSE x weights x
    grad_scale, each optional output alone NULL in turn; the loss bit for bit and inside its derived bound"""
    worst = 0.0
    for ddqn in (False, True):
        c = Rows(B, A, 2, ddqn=ddqn)
        pairs = itertools.product(VARIANTS, sorted(_layouts(A).items()))
        for n, ((huber, weighted, gs), (name, layout)) in enumerate(pairs):
            worst = max(worst, _run_head_loss(rlx, dev, c, huber, weighted, gs, layout, NULLS[(n + ddqn) % 4]))
    _measured("dqn_loss_err_over_bound[B=%d,A=%d]" % (B, A), worst)


@pytest.mark.parametrize("ddqn", [False, True], ids=["dqn", "ddqn"])
@pytest.mark.parametrize("B,A", [(32, 3), (64, 4), (100, 18), (24, 1)])
def test_dqn_head_loss_nonfinite_rows(rlx, dev, B, A, ddqn):
    """0 * inf under done and a NaN in the selector row: the row's target, error and the batch's loss are NaN (DQN); with
    a separate selector (DDQN) the target stays finite and is read at the NaN's column"""
    c = Rows(B, A, 3, nonfinite=True, ddqn=ddqn)
    for n, ((huber, weighted, gs), (name, layout)) in enumerate(itertools.product(VARIANTS, sorted(_layouts(A).items()))):
        _run_head_loss(rlx, dev, c, huber, weighted, gs, layout, NULLS[n % 3])
    r = c.ref(1, True, 1.0)
    assert np.isnan(r["loss_f32"])
    b = c.planted["nan mid"]
    if A >= 2:
        want = c.rewards[b] + (0.0 if c.dones[b] else 1.0) * DISCOUNT * F64(c.q_next[b, 1])
        assert same_bits(np.array([r["td_targets"][b, c.actions[b]]]), np.array([F32(want)]))
        assert np.isnan(want) != ddqn


def _buffers_for_refusal(dev, B, A):
    c = Rows(B, A, 4)
    i = Inputs(dev, q=c.q, q_next=c.q_next, actions=c.actions, rewards=c.rewards, dones=c.dones, weights=c.weights)
    outs = dict(dq=_out((B, A), F32, dev), tt=_out((B, A), F32, dev), err=_out(B, F64, dev), loss=_out(1, F32, dev),
                st=Guarded(4, dev, _tdtype(np.int32), init=np.zeros(1, dtype=np.int32)))
    return c, i, outs


def _untouched(i, outs):
    import torch
    torch.cuda.synchronize()
    i.unchanged()
    for k, g in outs.items():
        w = g.whole.cpu().numpy()
        assert (w[:g.lo] == FILL).all() and (w[g.hi:] == FILL).all(), k
        assert (w[g.lo:g.hi] == (0 if k == "st" else FILL)).all(), "%s changed although the call was refused" % k


@pytest.mark.parametrize("which", ["B=1025", "ld_q", "ld_next", "ld_dq", "ld_targets"])
def test_dqn_head_loss_refusals(rlx, dev, which):
    from coach_amd._rlx import RlxError
    B, A = (1025, 3) if which == "B=1025" else (8, 3)
    c, i, o = _buffers_for_refusal(dev, B, A)
    ld = {k: A - 1 if which == k else A for k in ("ld_q", "ld_next", "ld_dq", "ld_targets")}
    with pytest.raises(RlxError, match="bad sizes"):
        rlx.dqn_head_loss(i["q"], ld["ld_q"], i["q_next"], None, ld["ld_next"], i["actions"], i["rewards"], i["dones"],
                          i["weights"], DISCOUNT, B, A, 1, 1.0, o["dq"].t, ld["ld_dq"], o["err"].t, o["tt"].t,
                          ld["ld_targets"], o["loss"].t, o["st"].t, 0)
    _untouched(i, o)


# ------------------------------------------------------------------------------------------------ rlx_dqn_head_loss_backward

def _lower_output(rng, B, K, lower):
    """the lower layer's output: anything (none), >= 0 with exact zeros (relu), inside (-1, 1) (tanh)"""
    z = rng.randn(B, K)
    return {0: z, 1: np.maximum(z, 0), 2: np.tanh(z)}[lower].astype(F32)


def _run_head_bwd(rlx, dev, c, K, lower, outs, huber, weighted, gs, ld_q, ld_next, with_errors, seed):
    from coach_amd import _rlx
    B, A = c.B, c.A
    r = c.ref(huber, weighted, gs)
    rng = np.random.RandomState(seed)
    x, w = _lower_output(rng, B, K, lower), rng.randn(K, A).astype(F32)
    i = Inputs(dev, q=_pitch(c.q, ld_q), q_next=_pitch(c.q_next, ld_next),
               q_sel=None if c.q_sel is None else _pitch(c.q_sel, ld_next), actions=c.actions, rewards=c.rewards,
               dones=c.dones, weights=c.weights if weighted else None, x=x, w=w)
    dQ, dw, db, dx = _out((B, A), F32, dev), _out((K, A), F32, dev), _out(A, F32, dev), _out((B, K), F32, dev)
    err, loss = _out(B, F64, dev), _out(1, F32, dev)
    st = Guarded(4, dev, _tdtype(np.int32), init=np.zeros(1, dtype=np.int32))
    p = _rlx.SmallDenseProblem()
    p.x, p.w, p.dy = i["x"].data_ptr(), i["w"].data_ptr(), dQ.t.data_ptr()
    if "dw" in outs:
        p.dw, p.db = dw.t.data_ptr(), db.t.data_ptr()
    if "dx" in outs:
        p.dx = dx.t.data_ptr()
    p.towers, p.M, p.K, p.N, p.activation, p.lower_activation = 1, B, K, A, 0, lower
    rlx.dqn_head_loss_backward(ctypes.byref(p), i["q"], ld_q, i["q_next"], i["q_sel"], ld_next, i["actions"], i["rewards"],
                               i["dones"], i["weights"], DISCOUNT, B, A, huber, gs, err.t if with_errors else None, loss.t,
                               st.t, 0)
    what = (B, A, K, lower, outs, huber, weighted, gs, ld_q, ld_next)
    # dQ: the stand-alone kernel's values, and 0.0 in the rows of a refused action (dW is computed from them)
    got_dq = dQ.numpy().reshape(B, A)
    cmp_got, cmp_want = got_dq.copy(), r["dq"].copy()
    left_out = _taken(c, np.nonzero(r["nan_huber"])[0])
    cmp_got[left_out] = 0
    cmp_want[left_out] = 0
    assert same_bits(cmp_got, cmp_want), ("dQ",) + what
    exp_err = _sentinel(B, F64)
    if with_errors:
        exp_err[r["valid"]] = r["td_errors"][r["valid"]]
    assert same_bits(err.numpy(), exp_err), ("td_errors",) + what
    assert same_bits(loss.numpy(), np.array([r["loss_f32"]], dtype=F32)), ("loss",) + what
    assert int(st.numpy()[0]) == r["status"], what
    # dW, db, dx: float64 products of the dQ that was just pinned, inside the bounds that hold for any order
    hb = R.head_backward(x, w, got_dq, lower)
    worst = {}
    for key, g, shape in (("dw", dw, (K, A)), ("db", db, (A,)), ("dx", dx, (B, K))):
        got = g.numpy().reshape(shape)
        if key in outs or (key == "db" and "dw" in outs):
            ok, worst[key] = R.within(got, hb[key], hb[key + "_bound"])
            assert ok, (key, worst[key]) + what
        else:                                   # an output that was not asked for: not a byte of its buffer is written
            assert same_bits(got, _sentinel(shape, F32)), (key,) + what
    i.unchanged()
    for g in (dQ, dw, db, dx, err, loss, st):
        g.check_guards()
    return worst


KS = [1, 15, 16, 17, 33]
OUTS = [("dw",), ("dx",), ("dw", "dx")]


@pytest.mark.parametrize("A", [1, 2, 4, 5, 8, 9, 16])
@pytest.mark.parametrize("B", [1, 20, 64, 65, 256])
def test_dqn_head_loss_backward(rlx, dev, B, A):
    """every template width and the first size above it, one workgroup / several / a ragged last one (K), the three lower
    activations, dw-only / dx-only / both; Huber, weights, grad_scale, the selector, the pitches and td_errors = NULL change
    from launch to launch"""
    worst = dict(dw=0.0, db=0.0, dx=0.0)
    batches = {(nf, dd): Rows(B, A, 5, nonfinite=nf, ddqn=dd) for nf in (False, True) for dd in (False, True)}
    for n, (K, lower, outs) in enumerate(itertools.product(KS, (0, 1, 2), OUTS)):
        huber, weighted, gs = VARIANTS[n % 8]
        c = batches[(n % 5 == 4, n % 3 == 1)]
        ld_q, ld_next = [(A, A), (A + 5, A + 5), (A + 2, A + 5)][(n // 2) % 3]
        got = _run_head_bwd(rlx, dev, c, K, lower, outs, huber, weighted, gs, ld_q, ld_next, n % 4 != 3, seed=n)
        for k, v in got.items():
            worst[k] = max(worst[k], v)
    for k in sorted(worst):
        _measured("dqn_head_bwd_%s_err_over_bound[B=%d,A=%d]" % (k, B, A), worst[k])


def test_dqn_head_loss_backward_refused_action_rows(rlx, dev):
    """the stand-alone kernel leaves the row of an action outside [0, A) unwritten; the one-launch form writes zeros into
    its dQ row, because dW and dx are computed from it: both pinned on the same batch"""
    c = Rows(20, 3, 6)
    bad = [c.planted["a=-1"], c.planted["a=A"]]
    r = c.ref(1, True, 1.0)
    assert r["status"] == 1 and not r["valid"][bad].any() and not r["dq"][bad].any()
    _run_head_loss(rlx, dev, c, 1, True, 1.0, _layouts(3)["pitched"], None)         # sentinel in those rows
    _run_head_bwd(rlx, dev, c, 17, 2, ("dw", "dx"), 1, True, 1.0, 8, 8, True, seed=0)     # 0.0f in those rows
    terms = r["terms64"]
    assert terms[bad[0]] == 0 and terms[bad[1]] == 0                                 # they add nothing to the loss


@pytest.mark.parametrize("which", ["B=257", "A=17"])
def test_dqn_head_loss_backward_refusals(rlx, dev, which):
    from coach_amd import _rlx
    B, A, K = (257, 3, 8) if which == "B=257" else (8, 17, 8)
    c, i, o = _buffers_for_refusal(dev, B, A)
    x = Inputs(dev, x=np.ones((B, K), dtype=F32), w=np.ones((K, A), dtype=F32))
    o.update(dw=_out((K, A), F32, dev), db=_out(A, F32, dev), dx=_out((B, K), F32, dev))
    p = _rlx.SmallDenseProblem()
    p.x, p.w, p.dy = x["x"].data_ptr(), x["w"].data_ptr(), o["dq"].t.data_ptr()
    p.dw, p.db, p.dx = o["dw"].t.data_ptr(), o["db"].t.data_ptr(), o["dx"].t.data_ptr()
    p.towers, p.M, p.K, p.N, p.activation, p.lower_activation = 1, B, K, A, 0, 1
    with pytest.raises(_rlx.RlxError, match="rlx_dqn_head_loss_backward"):
        rlx.dqn_head_loss_backward(ctypes.byref(p), i["q"], A, i["q_next"], None, A, i["actions"], i["rewards"], i["dones"],
                                   i["weights"], DISCOUNT, B, A, 1, 1.0, o["err"].t, o["loss"].t, o["st"].t, 0)
    _untouched(i, o)
    x.unchanged()


# ------------------------------------------------------------------------------------------------ rlx_ac_td_targets

CLIP = (-3.0, 2.5)


@pytest.mark.parametrize("B", [1, 256, 257])
def test_ac_td_targets(rlx, dev, B):
    """q_stride 1 and 3 (NaN in the skipped columns), both terminal-state rules, the clip off and on; targets exactly on
    each bound, +-inf (clipped to the bound) and NaN (kept).  With use_non_zero_discount_for_terminal_states the product
    discount * q is the reference's fp32 product (targets_ref.ac_td_targets) and the result does not depend on the done
    bytes (0, 1 and 255 are all present); that the bytes are not even loaded cannot be seen from outside, because the
    entry point wants a non-NULL game_overs."""
    rng = np.random.RandomState(B)
    for n, (stride, nonzero, clip) in enumerate(itertools.product((1, 3), (0, 1), (None, CLIP))):
        rewards = (2 * rng.randn(B)).astype(F32)
        dones = rng.choice(np.array([0, 1, 255], dtype=np.uint8), size=B)
        q = np.full((B, stride), NAN, dtype=F32)
        q[:, 0] = 2 * rng.randn(B)
        # reward, q: with q = 0 the target is the reward
        planted = [(CLIP[0], 0), (CLIP[1], 0), (np.nextafter(F32(CLIP[1]), F32(9)), 0), (np.nextafter(F32(CLIP[0]), F32(-9)), 0),
                   (INF, 0), (-INF, 0), (NAN, 0), (0, NAN), (0, INF), (0, -INF), (INF, -INF), (-0.0, 0), (1e8, 1e-3)]
        for k, (rw, qv) in enumerate(planted[n if B == 1 else 0:]):          # B = 1: another planted value each time
            if k < B:
                rewards[k], q[k, 0] = rw, qv
        want = R.ac_td_targets(rewards, dones, q, stride, DISCOUNT, nonzero, clip)
        if B > 8 and clip:
            assert want[4] == F32(CLIP[1]) and want[5] == F32(CLIP[0]) and np.isnan(want[6]) and np.isnan(want[7])
        i = Inputs(dev, rewards=rewards, dones=dones, q=q)
        out = _out(B, F32, dev)
        rlx.ac_td_targets(i["rewards"], i["dones"], i["q"], stride, DISCOUNT, nonzero, 1 if clip else 0,
                          clip[0] if clip else 0.0, clip[1] if clip else 0.0, B, out.t, 0)
        assert same_bits(out.numpy(), want), (B, stride, nonzero, clip)
        i.unchanged()
        out.check_guards()


# ------------------------------------------------------------------------------------------------ smoothing and merging

NOISE_CLIP = 0.5


def _actor_batch(B, A, D, seed):
    rng = np.random.RandomState(seed + 100 * B + 10 * A + D)
    low = -(0.5 + rng.rand(A)).astype(F32)                    # per dimension, not symmetric
    high = (0.25 + rng.rand(A)).astype(F32)
    c = dict(actions=rng.randn(B, A).astype(F32), obs=rng.randn(B, D).astype(F32), next_obs=rng.randn(B, D).astype(F32),
             next_actions=(0.8 * rng.randn(B, A)).astype(F32), noise=0.4 * rng.randn(B, A), low=low, high=high)
    # noise beyond +-c, exactly on it, NaN, +-inf; an action that is already NaN; a sum exactly on a bound
    flat_n, flat_a = c["noise"].reshape(-1), c["next_actions"].reshape(-1)
    planted = [(2.0, None), (-2.0, None), (NOISE_CLIP, None), (-NOISE_CLIP, None), (NAN, None), (0.1, NAN), (INF, None),
               (-INF, 0.0), (0.0, "high"), (0.0, INF), (-0.0, -0.0)]
    if flat_n.size < len(planted):                    # a small batch holds the planted values `size` at a time, by seed
        planted = [planted[(seed * flat_n.size + j) % len(planted)] for j in range(flat_n.size)]
    for k, (nz, a) in enumerate(planted):
        flat_n[k] = nz
        if a is not None:
            flat_a[k] = high[k % A] if a == "high" else a
    return c


SHAPES = [(1, 1, 1), (3, 2, 5), (100, 6, 17), (257, 3, 4)]


@pytest.mark.parametrize("B,A,D", SHAPES)
def test_td3_smooth_actions(rlx, dev, B, A, D):
    for seed in range(-(-11 // (B * A)) if B * A < 11 else 1):       # (1, 1, 1): 11 batches, one planted value each
        c = _actor_batch(B, A, D, seed)
        want = R.td3_smooth_actions(c["next_actions"], c["noise"], NOISE_CLIP, c["low"], c["high"])
        i = Inputs(dev, next_actions=c["next_actions"], noise=c["noise"], low=c["low"], high=c["high"])
        out = _out((B, A), F32, dev)
        rlx.td3_smooth_actions(i["next_actions"], i["noise"], NOISE_CLIP, i["low"], i["high"], B, A, out.t, 0)
        assert same_bits(out.numpy().reshape(B, A), want), (B, A, seed)
        if B * A >= 11:
            assert np.isnan(want.reshape(-1)[[4, 5]]).all() and want.reshape(-1)[8] == c["high"][8 % A]
        i.unchanged()
        out.check_guards()


@pytest.mark.parametrize("B,A,D", SHAPES)
def test_ac_merge_inputs(rlx, dev, B, A, D):
    """merged2 against targets_ref.ac_merge_inputs (not against rlx_td3_smooth_actions: the two kernels share their clip);
    noise = NULL (DDPG): no draw and neither bound is read -- the bounds passed are NaN; merged_obs_only NULL and given,
    its action columns keep the sentinel"""
    W = A + D
    for smooth, with_only in itertools.product((False, True), (False, True)):
        c = _actor_batch(B, A, D, 2 * smooth + with_only)
        poisoned = np.full(A, NAN, dtype=F32)
        low, high = (c["low"], c["high"]) if smooth else (poisoned, poisoned)
        want2, want_obs = R.ac_merge_inputs(c["actions"], c["obs"], c["next_actions"], c["noise"] if smooth else None,
                                            NOISE_CLIP, low, high, c["next_obs"])
        i = Inputs(dev, actions=c["actions"], obs=c["obs"], next_actions=c["next_actions"],
                   noise=c["noise"] if smooth else None, low=low, high=high, next_obs=c["next_obs"])
        m2, only = _out((2, B, W), F32, dev), _out((B, W), F32, dev)
        rlx.ac_merge_inputs(i["actions"], i["obs"], i["next_actions"], i["noise"], NOISE_CLIP, i["low"], i["high"],
                            i["next_obs"], B, A, D, m2.t, only.t if with_only else None, 0)
        what = (B, A, D, smooth, with_only)
        assert same_bits(m2.numpy().reshape(2, B, W), want2), what
        exp_only = _sentinel((B, W), F32)
        if with_only:
            exp_only[:, A:] = want_obs
        assert same_bits(only.numpy().reshape(B, W), exp_only), what
        i.unchanged()
        m2.check_guards()
        only.check_guards()


# ------------------------------------------------------------------------------------------------ rlx_sac_value_targets

@pytest.mark.parametrize("B", [1, 256, 257])
def test_sac_value_targets(rlx, dev, B):
    rng = np.random.RandomState(B)
    for rep in range(3):
        q, lp = rng.randn(B).astype(F32), rng.randn(B).astype(F32)
        planted = [(INF, INF), (-INF, -INF), (INF, -INF), (NAN, 0), (0, NAN), (-0.0, 0.0), (0.0, 0.0), (1e8, 1e-3)]
        for k, (a, b) in enumerate(planted[rep * 3 if B == 1 else 0:]):
            if k < B:
                q[k], lp[k] = a, b
        want = R.sac_value_targets(q, lp)
        i = Inputs(dev, q=q, lp=lp)
        out = _out(B, F32, dev)
        rlx.sac_value_targets(i["q"], i["lp"], B, out.t, 0)
        assert same_bits(out.numpy(), want), (B, rep)
        i.unchanged()
        out.check_guards()
