"""csrc/optim.hip and csrc/adam_block_body.hpp, every entry point called by name and compared with an independent
reference (tests/optim_ref.py): oracle.optim.AdamTF1 / mix_weights for the update, the restated summation order and the
float64 sum for the gradient norm, numpy's minimum / maximum for the value clip.

optim.hip is built without contraction and without fast-math, so the update is the oracle's sequence of correctly rounded
fp32 operations: w, m, v, target and the beta powers are compared BIT FOR BIT after each of three consecutive steps (a NaN
where the oracle has a NaN, of any payload).  The norm is held to two things: bit-identity with optim_ref.norm_f32, which
adds in the kernels' order, and the error bound of that order against the float64 sum (optim_ref.norm_bound: it follows
from the number of additions on the longest path of the case's geometry, nothing is measured).

Every buffer a kernel writes is an interior slice of a larger allocation filled with 0xA5 (tests.test_frontend_kernels.
Guarded): the bytes around it, every input buffer, and the workspace behind the launch's `blocks` partial sums must come
back unchanged, and the ticket words must be zero again after every step."""
import ctypes

import numpy as np
import pytest

import optim_ref as R
from oracle.optim import AdamTF1
from test_frontend_kernels import FILL, Guarded, same_bits
from tests.util import dev_tensor

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
LR, B1, B2, EPS, RATE = 2.5e-4, 0.9, 0.99, 1e-4, 0.005
STEPS = 3

# (n, workspace_floats): the float4 body, the <= 3-element tail, one and two blocks; one register-held block running all
# four iterations (and 4100: one float4 too many for it -> the two-launch form); a strided 2nd..4th iteration over three
# blocks; 33 and 40 blocks: uneven groups of the two-level ticket
SMALL = [(n, 1024) for n in (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1027)]
CLAMPED = [(4093, 1), (4096, 1), (4099, 1), (4100, 1), (3 * 4096 - 5, 3), (40003, 33), (40003, 4096)]
GEOMETRIES = SMALL + CLAMPED
MIXED_SPLIT = [(3 * 4096 - 5, 3), (40003, 33), (40003, 4096)]        # some blocks early, some late

#           entry, norm_in_kernel, norm, target
VARIANTS = [("tf1", 2, False, False), ("tf1_norm", 2, True, False)] + \
           [("step", mode, norm, target) for mode in (0, 1, 2) for norm in (False, True) for target in (False, True)] + \
           [("split", 2, True, False)]


def _measured(name, value):
    print("MEASURED %s %.6g" % (name, value))


def _gid(p):
    return "n%d_ws%d" % p


def _vid(v):
    return "%s_mode%d_norm%d_target%d" % (v[0], v[1], int(v[2]), int(v[3]))


def _step_blocks(rlx, n, ws_floats):
    b = ctypes.c_int(-1)
    rlx.adam_step_blocks(n, ws_floats, ctypes.byref(b))
    return b.value


class Buffers(object):
    """everything an Adam launch touches, guarded; `n_alloc` floats per array (the call may name fewer)"""

    def __init__(self, dev, n_alloc, ws_floats, n_acc, w0, t0, acc0):
        import torch
        f = torch.float32
        zeros = np.zeros(n_alloc, dtype=F32)
        self.w = Guarded(4 * n_alloc, dev, f, init=w0)
        self.m = Guarded(4 * n_alloc, dev, f, init=zeros)
        self.v = Guarded(4 * n_alloc, dev, f, init=zeros)
        self.t = Guarded(4 * n_alloc, dev, f, init=t0)
        self.state = Guarded(8, dev, f, init=np.array([B1, B2], dtype=F32))
        self.norm = Guarded(4, dev, f)
        self.ws_alloc = max(1, min(ws_floats, R.MAX_BLOCKS)) + 8
        self.ws = Guarded(4 * self.ws_alloc, dev, f)
        self.acc = Guarded(4 * max(n_acc, 1), dev, f, init=acc0 if n_acc else None)
        from coach_amd import _rlx
        self.ticket = Guarded(4 * _rlx.ADAM_TICKET_WORDS, dev, torch.int32,
                              init=np.zeros(_rlx.ADAM_TICKET_WORDS, dtype=np.int32))
        self.all = dict(w=self.w, m=self.m, v=self.v, t=self.t, state=self.state, norm=self.norm, ws=self.ws, acc=self.acc,
                        ticket=self.ticket)

    def snapshot(self):
        return {k: b.whole.cpu().numpy().copy() for k, b in self.all.items()}

    def check_guards(self):
        for b in self.all.values():
            b.check_guards()


def _call(rlx, dev, variant, buf, g, n, ws_floats, grad_scale, acc_src, n_acc, lists=None):
    """one optimiser step through the entry point `variant` names"""
    entry, _, norm, target = variant
    a = buf
    if entry == "tf1":
        rlx.adam_tf1(a.w.t, g, a.m.t, a.v.t, n, LR, B1, B2, EPS, a.state.t, grad_scale, 0)
    elif entry == "tf1_norm":
        rlx.adam_tf1_norm(a.w.t, g, a.m.t, a.v.t, n, LR, B1, B2, EPS, a.state.t, grad_scale, a.norm.t, a.ws.t, ws_floats,
                          acc_src, a.acc.t if n_acc else None, n_acc, 0)
    elif entry == "step":
        rlx.adam_tf1_step(a.w.t, g, a.m.t, a.v.t, n, LR, B1, B2, EPS, a.state.t, grad_scale, a.norm.t if norm else None,
                          a.ws.t if norm else None, ws_floats, acc_src, a.acc.t if n_acc else None, n_acc,
                          a.t.t if target else None, RATE, a.ticket.t, 0)
    else:
        from coach_amd import _rlx
        dev_lists, ne, nl, nb = lists
        d = _rlx.AdamSplitDesc()
        d.weights, d.grads, d.m, d.v, d.n = a.w.t.data_ptr(), g.data_ptr(), a.m.t.data_ptr(), a.v.t.data_ptr(), n
        d.learning_rate, d.beta1, d.beta2, d.epsilon, d.grad_scale = LR, B1, B2, EPS, grad_scale
        d.state, d.partials, d.blocks = a.state.t.data_ptr(), a.ws.t.data_ptr(), nb
        d.early, d.late, d.n_early, d.n_late = dev_lists.data_ptr(), dev_lists.data_ptr() + 4 * ne, ne, nl
        rlx.adam_tf1_step_early(ctypes.byref(d), 2, 0)                  # 2: a workgroup loops over its early blocks
        rlx.adam_tf1_step_late(ctypes.byref(d), a.norm.t, acc_src, a.acc.t if n_acc else None, n_acc, a.ticket.t, 0)


def _split_lists(rlx, dev, n, nb):
    """the blocks whose every run lies in [1024, n) go early: never block 0, never a block without elements"""
    import torch
    flat = (ctypes.c_longlong * 2)(1024, n)
    early, late = (ctypes.c_int * nb)(), (ctypes.c_int * nb)()
    ne, nl = ctypes.c_int(), ctypes.c_int()
    rlx.adam_split_blocks(n, nb, flat, 1, early, ctypes.byref(ne), late, ctypes.byref(nl))
    assert sorted(list(early[:ne.value]) + list(late[:nl.value])) == list(range(nb))
    lists = torch.tensor(list(early[:ne.value]) + list(late[:nl.value]), dtype=torch.int32, device=dev)
    return lists, ne.value, nl.value, nb


def _run_steps(rlx, dev, variant, n, ws_floats, grads, grad_scale=0.5, n_acc=0, w0=None, seed=0):
    """STEPS steps from m = v = 0 through `variant`, each compared with the oracle.  -> the device's w, m, v, target, norms"""
    entry, mode, norm, target = variant
    rng = np.random.RandomState(seed + n)
    w0 = rng.randn(n).astype(F32) if w0 is None else w0
    t0 = rng.randn(n).astype(F32)
    acc0 = rng.randn(max(n_acc, 1)).astype(F32)
    buf = Buffers(dev, n, ws_floats, n_acc, w0, t0, acc0)
    opt = AdamTF1(n, LR, B1, B2, EPS)
    w_ref, t_ref, acc_ref = w0.copy(), t0.copy(), acc0.copy()
    blocks = R.adam_blocks(n, ws_floats)
    lists = None
    rlx.adam_norm_in_kernel(mode)
    try:
        nb = _step_blocks(rlx, n, ws_floats)
        assert nb == (blocks if mode == 2 and R.register_held(n, blocks) else 0)
        if (n, ws_floats) == (4100, 1):
            assert nb == 0, "4100 parameters are one float4 more than one register-held block takes"
        if entry == "split":
            lists = _split_lists(rlx, dev, n, nb)
            if (n, ws_floats) in MIXED_SPLIT:
                assert lists[1] >= 1 and lists[2] >= 1, lists[1:]
        norms, worst = [], 0.0
        for s in range(STEPS):
            g = grads[s]
            g_dev = Guarded(4 * n, dev, buf.w.t.dtype, init=g)
            src = rng.randn(max(n_acc, 1)).astype(F32)
            src_dev = Guarded(4 * max(n_acc, 1), dev, buf.w.t.dtype, init=src)
            _call(rlx, dev, variant, buf, g_dev.t, n, ws_floats, grad_scale, src_dev.t if n_acc else None, n_acc, lists)
            R.step_reference(opt, w_ref, g, grad_scale, t_ref if target else None, RATE)
            what = (_vid(variant), n, ws_floats, "step %d" % s)
            assert same_bits(buf.w.numpy(), w_ref), ("w",) + what
            assert same_bits(buf.m.numpy(), opt.m), ("m",) + what
            assert same_bits(buf.v.numpy(), opt.v), ("v",) + what
            assert same_bits(buf.t.numpy(), t_ref), ("target",) + what
            assert same_bits(buf.state.numpy(), np.array([opt.b1p, opt.b2p], dtype=F32)), ("beta powers",) + what
            assert same_bits(g_dev.numpy(), g), ("g was written",) + what
            g_dev.check_guards()
            ws = buf.ws.numpy()
            if norm:
                want, part = R.norm_f32(g, blocks)
                got = buf.norm.numpy()[0]
                norms.append(got)
                assert same_bits(ws[:blocks], part), ("partial sums",) + what
                assert same_bits(np.array([got]), np.array([want])), ("norm", got, want) + what
                exact = R.norm_f64(g)
                if np.isfinite(exact) and exact > 0 and np.isfinite(got):
                    rel = abs(F64(got) - exact) / exact
                    worst = max(worst, rel / R.norm_bound(n, blocks))
                    assert rel <= R.norm_bound(n, blocks), (rel, R.norm_bound(n, blocks), R.norm_depth(n, blocks)) + what
                if n_acc:
                    acc_ref = acc_ref + src
                    assert same_bits(buf.acc.numpy(), acc_ref), ("acc_dst",) + what
                    assert same_bits(src_dev.numpy(), src), ("acc_src was written",) + what
            used = blocks if norm else 0
            assert (ws[used:].view(np.uint8) == FILL).all(), ("workspace behind the partial sums was written",) + what
            assert not buf.ticket.numpy().any(), ("ticket words not re-armed",) + what
            buf.check_guards()
        if norm:
            _measured("adam_norm_rel_err_over_bound[%s,%d,%d]" % (_vid(variant), n, ws_floats), worst)
    finally:
        rlx.adam_norm_in_kernel(2)
    return dict(w=buf.w.numpy(), m=buf.m.numpy(), v=buf.v.numpy(), t=buf.t.numpy(), norms=norms)


def _grads(n, seed=0):
    rng = np.random.RandomState(7000 + seed + n)
    return [rng.randn(n).astype(F32) for _ in range(STEPS)]


def _cases():
    out = []
    for geo in GEOMETRIES:
        for v in VARIANTS:
            if v[0] == "split" and not R.register_held(geo[0], R.adam_blocks(*geo)):
                continue                    # (4100, 1): refused, see test_refusals_leave_every_buffer_untouched
            out.append(pytest.param(geo, v, id=_gid(geo) + "-" + _vid(v)))
    return out


@pytest.mark.parametrize("geo,variant", _cases())
def test_adam_equals_the_oracle_bit_for_bit(rlx, dev, geo, variant):
    n, ws_floats = geo
    _run_steps(rlx, dev, variant, n, ws_floats, _grads(n), grad_scale=0.5, n_acc=3 if variant[2] else 0)


@pytest.mark.parametrize("n_acc", [0, 3, 64])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("variant", [VARIANTS[1], ("step", 0, True, True), ("step", 1, True, True), ("step", 2, True, True),
                                     VARIANTS[-1]], ids=_vid)
@pytest.mark.parametrize("geo", [(1027, 1024), (4099, 1), (40003, 33)], ids=_gid)
def test_adam_grad_scale_and_signal_sums(rlx, dev, geo, variant, grad_scale, n_acc):
    """acc_dst[i] += acc_src[i] for i < n_acc rides with the norm's finish: one fp32 add each, bit for bit"""
    n, ws_floats = geo
    _run_steps(rlx, dev, variant, n, ws_floats, _grads(n, 1), grad_scale=grad_scale, n_acc=n_acc, seed=1)


#  index -> planted gradient (n = 1027: 1024, 1025, 1026 are the tail behind the last float4; 600 sits in block 0's
#  thread 150, 1020 in its last thread)
PLANTED = {
    "nonfinite": {0: np.nan, 5: np.inf, 300: -np.inf, 7: 0.0, 1024: 0.0, 1025: 1e-20, 600: 1e20, 1026: np.nan, 1020: -1e-20},
    "overflow": {7: 0.0, 1024: 0.0, 1025: 1e-20, 600: 1e20, 1020: -1e20},
}


@pytest.mark.parametrize("variant", [VARIANTS[0], VARIANTS[1], ("step", 0, True, True), ("step", 1, True, True),
                                     ("step", 2, True, True), ("step", 2, False, True), VARIANTS[-1]], ids=_vid)
@pytest.mark.parametrize("which", sorted(PLANTED))
def test_adam_planted_values_stay_where_they_are(rlx, dev, which, variant):
    """NaN, +-inf: m, v, w and target of that element follow numpy's NaN / inf arithmetic.  0 with m = v = 0: w keeps its
    bits (index 7: 1.5, index 1024: -0.0).  1e-20: g^2 is a denormal.  1e20: g^2 overflows to inf.  The same gradients with
    ordinary values in the planted places give the same bits everywhere else; the norm is numpy's NaN or inf."""
    n, ws_floats = 1027, 1024
    clean = _grads(n, 2)
    planted = [g.copy() for g in clean]
    idx = np.array(sorted(PLANTED[which]))
    for g in planted:
        g[idx] = np.array([PLANTED[which][i] for i in idx], dtype=F32)
    assert np.float32(1e-20) * np.float32(1e-20) > 0 and np.float32(1e-20) * np.float32(1e-20) < np.finfo(F32).tiny
    w0 = np.random.RandomState(5).randn(n).astype(F32)
    w0[7], w0[1024] = 1.5, -0.0
    a = _run_steps(rlx, dev, variant, n, ws_floats, planted, n_acc=3 if variant[2] else 0, w0=w0, seed=2)
    b = _run_steps(rlx, dev, variant, n, ws_floats, clean, n_acc=3 if variant[2] else 0, w0=w0, seed=2)
    others = np.ones(n, dtype=bool)
    others[idx] = False
    for k in ("w", "m", "v", "t"):
        assert same_bits(a[k][others], b[k][others]), k
    assert a["w"][[7, 1024]].view(np.uint32).tolist() == np.array([1.5, -0.0], dtype=F32).view(np.uint32).tolist()
    if variant[2]:
        assert all(np.isnan(x) for x in a["norms"]) if which == "nonfinite" else all(np.isposinf(x) for x in a["norms"])
        assert all(np.isfinite(x) for x in b["norms"])


# ------------------------------------------------------------------------------------------------ rlx_mix_weights

@pytest.mark.parametrize("rate", [0.0, 0.005, 0.25, 1.0])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025])
def test_mix_weights_equals_numpy(rlx, dev, n, rate):
    """two fp32 products and one add, both coefficients rounded to fp32 first (architecture.py:604-605); a NaN in target
    times a zero coefficient (rate = 1) stays a NaN, as in numpy"""
    import torch
    rng = np.random.RandomState(n)
    online, target = rng.randn(n).astype(F32), rng.randn(n).astype(F32)
    target[n // 2] = np.nan
    online[0] = np.inf if n > 1 else online[0]
    with np.errstate(invalid="ignore"):
        want = np.float32(rate) * online + np.float32(1.0 - rate) * target
    assert np.isnan(want[n // 2])
    t = Guarded(4 * n, dev, torch.float32, init=target)
    o = Guarded(4 * n, dev, torch.float32, init=online)
    rlx.mix_weights(t.t, o.t, n, rate, 0)
    assert same_bits(t.numpy(), want)
    assert same_bits(o.numpy(), online)
    t.check_guards()
    o.check_guards()


# ------------------------------------------------------------------------------------------------ rlx_clip_by_value

@pytest.mark.parametrize("clip", [1.0, 0.37])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 262145])
def test_clip_by_value_equals_numpy(rlx, dev, n, clip):
    """tf.clip_by_value = minimum(maximum(x, -c), c), NaN kept.  262145 = 1024 blocks x 256 + 1: the grid is capped at 1024
    blocks, so the stride loop makes a second pass for the last element."""
    import torch
    c = F32(clip)
    rng = np.random.RandomState(n)
    x = (rng.randn(n) * 2).astype(F32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, c, -c, np.nextafter(c, F32(np.inf)), np.nextafter(c, F32(0)),
                        np.nextafter(-c, F32(-np.inf)), np.nextafter(-c, F32(0))], dtype=F32)
    if n >= special.size:
        x[:special.size] = special
        x[-1] = F32(3.0)                                   # the second pass's element is clipped as well
    else:
        x[0] = special[n % 3]
    with np.errstate(invalid="ignore"):
        want = np.minimum(np.maximum(x, -c), c)
    buf = Guarded(4 * n, dev, torch.float32, init=x)
    rlx.clip_by_value(buf.t, n, float(c), 0)
    assert same_bits(buf.numpy(), want)
    buf.check_guards()


# ------------------------------------------------------------------------------------------------ refusals

def _refusal_calls(rlx, dev):
    """name -> (call(buffers, g, src), message): every call must raise RlxError before anything is launched"""
    import torch
    n = 1027

    def step(n_=n, norm=True, ws_floats=1024, n_acc=0, offset=False):
        def call(a, g, src):
            w = a.w.whole[a.w.lo + 4:a.w.lo + 4 + 4 * 16].view(torch.float32) if offset else a.w.t
            rlx.adam_tf1_step(w, g, a.m.t, a.v.t, n_, LR, B1, B2, EPS, a.state.t, 0.5, a.norm.t if norm else None,
                              a.ws.t if norm else None, ws_floats, src, a.acc.t, n_acc, a.t.t, RATE, a.ticket.t, 0)
        return call

    def tf1(n_=n, offset=False):
        def call(a, g, src):
            m = a.m.whole[a.m.lo + 4:a.m.lo + 4 + 4 * 16].view(torch.float32) if offset else a.m.t
            rlx.adam_tf1(a.w.t, g, m, a.v.t, n_, LR, B1, B2, EPS, a.state.t, 0.5, 0)
        return call

    def tf1_norm(n_=n, ws_floats=1024, n_acc=0, offset=False):
        def call(a, g, src):
            gg = g[1:17] if offset else g
            rlx.adam_tf1_norm(a.w.t, gg, a.m.t, a.v.t, n_, LR, B1, B2, EPS, a.state.t, 0.5, a.norm.t, a.ws.t, ws_floats, src,
                              a.acc.t, n_acc, 0)
        return call

    def mix(n_=n, offset=False):
        def call(a, g, src):
            rlx.mix_weights(a.t.t, g[1:17] if offset else g, n_, RATE, 0)
        return call

    def clip(n_=n, c=1.0):
        def call(a, g, src):
            rlx.clip_by_value(a.w.t, n_, c, 0)
        return call

    def split_too_large(a, g, src):
        early, late = (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
        ne, nl = ctypes.c_int(), ctypes.c_int()
        rlx.adam_split_blocks(4100, 1, None, 0, early, ctypes.byref(ne), late, ctypes.byref(nl))

    return {
        "step_n0": (step(n_=0), "empty"), "step_offset": (step(offset=True), "16-byte aligned"),
        "step_norm_without_workspace_floats": (step(ws_floats=0), "workspace too small"),
        "step_n_acc_65": (step(n_acc=65), "signal accumulation"),
        "step_n_acc_without_norm": (step(norm=False, n_acc=3), "give norm_out"),
        "tf1_n0": (tf1(n_=0), "empty"), "tf1_offset": (tf1(offset=True), "16-byte aligned"),
        "tf1_norm_n0": (tf1_norm(n_=0), "empty"), "tf1_norm_offset": (tf1_norm(offset=True), "16-byte aligned"),
        "tf1_norm_without_workspace_floats": (tf1_norm(ws_floats=0), "workspace too small"),
        "tf1_norm_n_acc_65": (tf1_norm(n_acc=65), "signal accumulation"),
        "mix_n0": (mix(n_=0), "bad arguments"), "mix_offset": (mix(offset=True), "16-byte aligned"),
        "clip_n0": (clip(n_=0), "bad arguments"), "clip_negative": (clip(c=-1.0), "must be positive"),
        "split_does_not_fit": (split_too_large, "do not fit"),
    }


REFUSALS = ["step_n0", "step_offset", "step_norm_without_workspace_floats", "step_n_acc_65", "step_n_acc_without_norm",
            "tf1_n0", "tf1_offset", "tf1_norm_n0", "tf1_norm_offset", "tf1_norm_without_workspace_floats", "tf1_norm_n_acc_65",
            "mix_n0", "mix_offset", "clip_n0", "clip_negative", "split_does_not_fit"]


# rlx_adam_norm_in_kernel only selects among the forms of rlx_adam_tf1_step: its refusals are tried in all three modes
@pytest.mark.parametrize("name,mode", [(name, mode) for name in REFUSALS for mode in ((0, 1, 2) if name.startswith("step") else (2,))])
def test_refusals_leave_every_buffer_untouched(rlx, dev, name, mode):
    """an RlxError comes back BEFORE any launch: weights, moments, target, beta powers, norm, workspace, signal sums, ticket
    and the gradient hold the bits they held.  (n_acc > 0 without norm_out used to be refused behind the Adam launch.)"""
    import torch
    from coach_amd._rlx import RlxError
    n = 1027
    rng = np.random.RandomState(11)
    buf = Buffers(dev, n, 1024, 64, rng.randn(n).astype(F32), rng.randn(n).astype(F32), rng.randn(64).astype(F32))
    buf.m.t.copy_(dev_tensor(rng.rand(n).astype(F32), dev))
    buf.v.t.copy_(dev_tensor(rng.rand(n).astype(F32), dev))
    g = Guarded(4 * n, dev, torch.float32, init=rng.randn(n).astype(F32))
    src = Guarded(4 * 65, dev, torch.float32, init=rng.randn(65).astype(F32))
    before = buf.snapshot()
    g0, src0 = g.whole.cpu().numpy().copy(), src.whole.cpu().numpy().copy()
    call, message = _refusal_calls(rlx, dev)[name]
    assert sorted(_refusal_calls(rlx, dev)) == sorted(REFUSALS)
    rlx.adam_norm_in_kernel(mode)
    try:
        with pytest.raises(RlxError, match=message):
            call(buf, g.t, src.t)
    finally:
        rlx.adam_norm_in_kernel(2)
    torch.cuda.synchronize()
    after = buf.snapshot()
    for k in before:
        assert np.array_equal(before[k], after[k]), "%s changed although the call was refused" % k
    assert np.array_equal(g.whole.cpu().numpy(), g0) and np.array_equal(src.whole.cpu().numpy(), src0)
