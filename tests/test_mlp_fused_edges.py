"""rlx_mlp_dqn_update and rlx_mlp_q_act (csrc/mlp_fused.hip) at the edges of their shapes and of their inputs, against
the layer-by-layer device path and against tests/mlp_ref.py (float64).

The fused update never writes a gradient to memory, and Adam's first step from zero slots moves a weight by about
lr * sign(g): weights after a few steps cannot see a gradient of the right sign and the wrong size.  The Adam slots can:
after ONE update from zero state m = (1 - beta1) g and v = (1 - beta2) g^2, so every case compares adam.m and adam.v per
named tensor with the layer-by-layer path's and with mlp_ref's float64 gradient -- the gradient check of this kernel.

The seeded cases come from mlp_ref (CASES / make_case); tests/test_mlp_ref.py asserts on the CPU that none of their
discontinuities (a relu's sign, a selecting arg-max, the Huber branch) is within fp32 reach, so every element of every
tensor is compared, none masked.  Each case first asserts that the fused path is the one taken.  Tolerances are those of
tests/test_mlp_fused.py (loss, |TD|, norm, weights) and of tests/test_conv_dw_f32.py (gradients: rtol 2e-5 and 2e-6 of
the tensor's largest gradient); each test prints its worst figures (`pytest -s`) before it asserts.  Nothing here tries to
reach the barrier's spin limit (status bit 8) or any fault."""
import numpy as np
import pytest

import mlp_ref as R

pytestmark = pytest.mark.gpu

G_TOL = dict(rtol=2e-5, atol_of_max=2e-6)
_ids = lambda k: "%s-A%d-B%d-%s-%s-%s" % ("x".join(map(str, R.SHAPES[k[0]][0])), R.SHAPES[k[0]][1], R.SHAPES[k[0]][2],
                                        "huber" if k[1] else "mse", "ddqn" if k[2] else "dqn", k[3])
_REF = {}


def _ref(c, discount=R.DISCOUNT):
    """mlp_ref's run of a case, computed once and shared"""
    hit = _REF.get(c["key"])
    if hit is None:
        with np.errstate(invalid="ignore"):
            hit = _REF[c["key"]] = R.run_case(c, discount)
    return hit


def _dv(dev, x, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dt)


def _net(dev, c, fused):
    """tests/test_mlp_fused.py::_net with the case's weights: online and target copies are written from mlp_ref's draws
    (biases that are not zero, a target network that is not the online one)"""
    from coach_amd.nn.networks import DQNNet
    d0, h1, h2 = c["dims"]
    net = DQNNet(dev, (d0,), c["A"], embedder=[h1], middleware=[h2], learning_rate=R.LR, adam_beta1=R.BETA1,
                 adam_beta2=R.BETA2, optimizer_epsilon=R.EPS, replace_mse_with_huber_loss=c["huber"], seed=4)
    if not fused:
        net._fused = None
    else:
        assert net._fused is not None, "the fused update does not take this shape"
    for k in R.NAMES:
        net.params.w(R.PARAM_NAMES[k]).copy_(_dv(dev, c["W"][k], net.params.weights.dtype))
        net.params.w(R.PARAM_NAMES[k], buf=net.target).copy_(_dv(dev, c["Wt"][k], net.params.weights.dtype))
    return net


def _slot(net, buf, k):
    return net.params.view(buf, R.PARAM_NAMES[k]).cpu().numpy().astype(np.float64)


def _args(dev, c, discount=R.DISCOUNT):
    import torch
    return (_dv(dev, c["s"], torch.float32), _dv(dev, c["s2"], torch.float32), c["B"], _dv(dev, c["a"], torch.int32),
            _dv(dev, c["r"], torch.float32), _dv(dev, c["done"], torch.uint8), discount)


def _iw(dev, c):
    import torch
    if c["iw"] is None:
        return None
    return _dv(dev, c["iw"], torch.float32 if c["iw_kind"] == "f32" else torch.float64)


def _learn(dev, net, c, discount=R.DISCOUNT, td_fill=0.0, check=True):
    """one update -> (loss, norm, |TD| [B], status word)"""
    import torch
    td = torch.full((c["B"],), td_fill, dtype=torch.float64, device=dev)
    loss = net.learn_from_batch(*_args(dev, c, discount), importance_weights=_iw(dev, c), td_errors=td,
                                double_dqn=c["ddqn"])
    status = int(net.status.item())
    if check:
        net.check_status()
    else:
        net.status.zero_()
    return float(loss.item()), float(net.norm.item()), td.cpu().numpy(), status


def _close(got, ref, rtol, atol, what):
    """assert |got - ref| <= atol + rtol |ref| elementwise, NaN where and only where ref is; -> worst error / bound"""
    got, ref = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN masks differ (%d vs %d NaN)" % (
        what, np.isnan(got).sum(), np.isnan(ref).sum())
    fin = ~np.isnan(ref)
    if not fin.any():
        return 0.0
    bound = np.broadcast_to(np.asarray(atol, dtype=np.float64), ref.shape)[fin] + rtol * np.abs(ref[fin])
    err = np.abs(got[fin] - ref[fin])
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound), "%s: worst error %.3g of its bound (abs %.3g)" % (what, worst, err.max())
    return worst


def _check_slots(f, p, g64, tag):
    """adam.m / adam.v of the fused net after ONE update from zero state against the layer-by-layer net's and against
    (1 - beta1) g64 / (1 - beta2) g64^2, per named tensor.  m: the gradient's tolerance.  v: what that tolerance allows a
    square to move, (2 |g| t + t^2) with t = rtol |g| + atol."""
    worst = {}
    for k in R.NAMES:
        g = g64[k]
        fin = np.abs(g[~np.isnan(g)])
        gmax = float(fin.max()) if fin.size else 0.0
        with np.errstate(invalid="ignore"):
            t = G_TOL["rtol"] * np.abs(g) + G_TOL["atol_of_max"] * gmax
            tv = (1 - R.BETA2) * (2 * np.abs(g) * t + t * t)
        mf, mp, vf, vp = _slot(f, f.adam.m, k), _slot(p, p.adam.m, k), _slot(f, f.adam.v, k), _slot(p, p.adam.v, k)
        om1 = 1 - R.BETA1
        w = [_close(mf, om1 * g, 0.0, om1 * t, "%s m[%s] fused vs fp64" % (tag, k)),
             _close(mp, om1 * g, 0.0, om1 * t, "%s m[%s] layerwise vs fp64" % (tag, k)),
             _close(mf, mp, 0.0, om1 * t, "%s m[%s] fused vs layerwise" % (tag, k)),
             _close(vf, (1 - R.BETA2) * g * g, 1e-6, tv, "%s v[%s] fused vs fp64" % (tag, k)),
             _close(vf, vp, 1e-6, tv, "%s v[%s] fused vs layerwise" % (tag, k))]
        worst[k] = max(w)
        if gmax > 0:
            assert np.nanmax(np.abs(mf)) > 0, "%s: m[%s] is all zero" % (tag, k)
    print("MEASURED %s gradient error / tolerance per tensor: %s" % (tag, {k: "%.3g" % v for k, v in worst.items()}))


def _check_first_update(dev, c, discount=R.DISCOUNT, td_fill=0.0, expect_status=0):
    """fused and layer-by-layer nets from the case's weights, one update from zero Adam state, everything compared
    path to path and with mlp_ref -> (fused net, layer-by-layer net, reference)"""
    import torch
    ref = _ref(c, discount)
    f, p = _net(dev, c, True), _net(dev, c, False)
    bits = lambda t: t.view(torch.int32)                                  # (a case may carry a NaN)
    assert torch.equal(bits(f.params.weights), bits(p.params.weights)) and torch.equal(bits(f.target), bits(p.target))
    assert float(f.adam.m.abs().max()) == 0 and float(f.adam.v.abs().max()) == 0
    tag = str(c["key"])
    lf, nf, tdf, sf = _learn(dev, f, c, discount, td_fill, check=not expect_status)
    lp, np_, tdp, sp = _learn(dev, p, c, discount, td_fill, check=not expect_status)
    assert sf == sp == expect_status == ref["status"], (sf, sp, ref["status"])
    print("MEASURED %s loss fused %.9g layerwise %.9g fp64 %.9g; norm %.9g %.9g %.9g" % (tag, lf, lp, ref["loss"], nf, np_, ref["norm"]))
    _close(lf, lp, 2e-5, 1e-7, tag + " loss fused vs layerwise")
    _close(lf, ref["loss"], 2e-4, 1e-7, tag + " loss fused vs fp64")
    _close(nf, np_, 2e-4, 0.0, tag + " norm fused vs layerwise")
    _close(nf, ref["norm"], 2e-4, 0.0, tag + " norm fused vs fp64")
    ok = ref["valid"]
    assert np.array_equal(tdf[~ok], tdp[~ok]) and np.all(tdf[~ok] == td_fill)      # a refused row's slot: left as it was
    print("MEASURED %s |TD| worst of bound: vs layerwise %.3g, vs fp64 %.3g" % (
        tag, _close(tdf[ok], tdp[ok], 1e-4, 2e-6, tag + " |TD| fused vs layerwise"),
        _close(tdf[ok], ref["td"][ok], 2e-3, 5e-6, tag + " |TD| fused vs fp64")))
    _check_slots(f, p, ref["grads"], tag)
    with np.errstate(invalid="ignore"):
        w64, _, _ = R.adam_first_step(c["W"], ref["grads"])
    for k in R.NAMES:
        wf, wp = _slot(f, f.params.weights, k), _slot(p, p.params.weights, k)
        a = _close(wf, wp, 0.0, 2e-5, "%s weights[%s] fused vs layerwise" % (tag, k))
        b = _close(wf, w64[k], 0.0, 5e-5, "%s weights[%s] fused vs fp64" % (tag, k))
        print("MEASURED %s weights[%s] abs err: vs layerwise %.3g, vs fp64 %.3g" % (tag, k, a * 2e-5, b * 5e-5))
        assert np.array_equal(_slot(f, f.target, k), c["Wt"][k].astype(np.float64), equal_nan=True)   # the target copy is read only
    assert torch.allclose(f.adam.state, p.adam.state)
    assert int(f._fused["sync"].abs().sum().item()) == 0
    return f, p, ref


@pytest.mark.parametrize("key", R.case_list(), ids=_ids)
def test_update_at_shape_edges(dev, key):
    """The shapes of mlp_ref.SHAPES (each edge is named there), MSE and Huber, DQN and Double DQN, importance weights
    absent / fp32 / fp64 with one weight exactly 0.  One update from zero Adam state: m, v, loss, |TD|, norm, weights.
    Then three more updates with a target sync after the second: the weights again, the barrier words re-armed."""
    import torch
    c = R.make_case(key)
    f, p, _ = _check_first_update(dev, c)
    rng = np.random.RandomState(1000 + R.SEEDS[key])
    d0 = c["dims"][0]
    for it in range(3):
        b = dict(c, s=rng.randn(c["B"], d0).astype(np.float32), s2=rng.randn(c["B"], d0).astype(np.float32),
                 a=rng.randint(0, c["A"], c["B"]).astype(np.int32), r=rng.randn(c["B"]).astype(np.float32),
                 done=(rng.rand(c["B"]) < 0.2).astype(np.uint8))
        res = [_learn(dev, net, b) for net in (f, p)]
        _close(res[0][0], res[1][0], 2e-5, 1e-7, "loss, update %d" % (it + 2))
        _close(res[0][2], res[1][2], 1e-4, 2e-6, "|TD|, update %d" % (it + 2))
        if it == 1:
            f.update_target(1.0); p.update_target(1.0)
    for k in R.NAMES:
        a = _close(_slot(f, f.params.weights, k), _slot(p, p.params.weights, k), 0.0, 2e-5, "weights[%s] after four updates" % k)
        print("MEASURED %s weights[%s] after four updates, abs err vs layerwise %.3g" % (key, k, a * 2e-5))
    assert torch.allclose(f.adam.state, p.adam.state)
    assert int(f._fused["sync"].abs().sum().item()) == 0


def test_supported_predicate_edges(dev):
    """rlx_mlp_dqn_supported at its limits.  H1 = 288: lds_floats gives 163,392 B with D0 = 8 and 163,920 B with D0 = 9
    (one more padded pair of input rows) against 163,840 B."""
    import torch
    from coach_amd import _rlx
    from coach_amd.nn.networks import DQNNet
    sup = _rlx.lib().rlx_mlp_dqn_supported
    for B in (1, 32):
        for A in (1, 16):
            assert sup(B, 8, 288, 32, A) == 1 and sup(B, 9, 288, 32, A) == 0
    assert sup(1, 4, 32, 2048, 2) == 0                      # H1 % G != 0 (G = 64)
    assert sup(1, 4, 64, 2048, 2) == 1
    assert sup(1, 4, 64, 2080, 2) == 0                      # G = 65
    assert sup(32, 4, 64, 64, 2) == 1 and sup(33, 4, 64, 64, 2) == 0
    assert sup(32, 4, 64, 64, 16) == 1 and sup(32, 4, 64, 64, 17) == 0
    assert sup(32, 16, 64, 64, 2) == 1 and sup(32, 17, 64, 64, 2) == 0
    assert sup(32, 4, 320, 32, 2) == 0                      # the next H1 beyond 288 does not fit whatever D0 is
    for shape in R.SHAPES:
        assert sup(shape[2], *shape[0], shape[1]) == 1, shape
    # G = 5 does not divide H1 = 96: the network trains layer by layer, and still acts in one launch
    net = DQNNet(dev, (8,), 5, embedder=[96], middleware=[160], learning_rate=1e-3, seed=4)
    assert sup(20, 8, 96, 160, 5) == 0 and net._fused is None and net.can_act_fused(3)
    rng = np.random.RandomState(0)
    before = net.params.weights.clone()
    loss = net.learn_from_batch(_dv(dev, rng.randn(20, 8).astype(np.float32), torch.float32),
                                _dv(dev, rng.randn(20, 8).astype(np.float32), torch.float32), 20,
                                _dv(dev, rng.randint(0, 5, 20), torch.int32), _dv(dev, rng.randn(20).astype(np.float32), torch.float32),
                                _dv(dev, np.zeros(20), torch.uint8), 0.97)
    net.check_status()
    assert np.isfinite(float(loss.item())) and not torch.equal(before, net.params.weights)


@pytest.mark.parametrize("variant", ["all_done", "done_255", "discount_0"])
def test_terminal_and_discount_edges(dev, variant):
    """every game_over = 1, one game_over byte of 255, discount = 0: in each the targets (of the rows concerned) are the
    rewards, whatever the target network says -- asserted on the reference, whose |TD| the device must then match"""
    c, discount = R.make_edge_case(variant)
    ref = _ref(c, discount)
    rows = np.arange(c["B"]) if variant != "done_255" else np.array([7])
    assert np.array_equal(ref["targets"][rows], c["r"][rows].astype(np.float64))
    if variant == "done_255":
        assert c["done"][7] == 255 and not np.array_equal(ref["targets"], c["r"].astype(np.float64))
    _check_first_update(dev, c, discount)


@pytest.mark.parametrize("sign", [1, -1])
def test_huber_at_an_error_of_exactly_one(dev, sign):
    """|e| = 1 without rounding (mlp_ref.make_huber_one_case): the loss is 0.5 per row from either branch, the gradient
    sign * iw / B reaches b3 alone.  m[b3] = (1 - beta1) * sum over the rows that took the action, exact up to the
    rounding of (1 - beta1); every other slot stays exactly zero."""
    c = R.make_huber_one_case(sign)
    f, p, ref = _check_first_update(dev, c)
    assert np.array_equal(ref["e"], np.full(c["B"], float(sign)))
    want = np.array([sign * c["iw"][c["a"] == a].astype(np.float64).sum() / c["B"] for a in range(c["A"])])
    np.testing.assert_allclose(ref["grads"]["b3"], want, rtol=1e-14)
    assert abs(ref["loss"] - 0.5 * c["iw"].astype(np.float64).mean()) < 1e-12
    for net in (f, p):
        np.testing.assert_allclose(float(net.loss.item()), 0.5 * c["iw"].astype(np.float64).mean(), rtol=1e-6)
        np.testing.assert_allclose(_slot(net, net.adam.m, "b3"), (1 - R.BETA1) * want, rtol=1e-6, atol=0)
        for k in R.NAMES[:-1]:
            assert not _slot(net, net.adam.m, k).any() and not _slot(net, net.adam.v, k).any(), k


def test_refused_actions(dev):
    """An action of -1 and an action of A: both paths raise status bit 1, leave the row's slot of a pre-filled |TD| tensor
    as it was, give the row no loss term and no gradient (the mean still divides by B), and agree on everything else."""
    c, discount = R.make_edge_case("bad_actions")
    f, p, ref = _check_first_update(dev, c, discount, td_fill=7.0, expect_status=1)
    assert (~ref["valid"]).sum() == 2 and list(np.flatnonzero(~ref["valid"])) == list(R.BAD_ROWS)


@pytest.mark.parametrize("ddqn", [False, True])
def test_nan_gradient_reaches_inactive_units(dev, ddqn):
    """A NaN in the target network's last bias (mlp_ref.make_nan_case; MSE, so that the NaN error's gradient is NaN on the
    device as in numpy).  The rows that select the NaN column have a NaN dQ; the relu backward MULTIPLIES, so dz2 of those
    rows is NaN at every unit, active or not (NaN * 0), and a hidden unit that is inactive over the whole batch gets a NaN
    column of W2 and entry of b2 all the same -- and so one layer down.  `h > 0 ? dy : 0` wrote 0 there and kept those
    weights finite: with that form in mlp_fused.hip the masks of w2 / b2 / w1 / b1 below differ from the layer-by-layer
    path's and the reference's at exactly the units tests/test_mlp_ref.py finds inactive (run against the kernel with the
    select form: "m[w1] fused vs fp64: NaN masks differ", 648 of 768 NaN under DQN, 600 under Double DQN, where the
    layer-by-layer path and the reference have 768).  Finite elements agree at the
    usual tolerances (in _check_first_update, which compares NaN masks first)."""
    c = R.make_nan_case(ddqn)
    f, p, ref = _check_first_update(dev, c)
    dead1, dead2 = R.inactive_units(ref)
    assert len(dead1) and len(dead2)
    for net in (f, p):
        for buf in (net.params.weights, net.adam.m, net.adam.v):
            assert np.isnan(_slot(net, buf, "w2")[:, dead2]).all() and np.isnan(_slot(net, buf, "b2")[dead2]).all()
            assert np.isnan(_slot(net, buf, "w1")[:, dead1]).all() and np.isnan(_slot(net, buf, "b1")[dead1]).all()
    for k in R.NAMES:
        masks = [np.isnan(_slot(net, net.params.weights, k)) for net in (f, p)] + [np.isnan(ref["grads"][k])]
        assert np.array_equal(masks[0], masks[1]) and np.array_equal(masks[0], masks[2]), k


def test_finite_updates_keep_the_bits_of_the_select_form(dev, golden):
    """Multiplying by relu' instead of selecting changes no finite result: s * 1 = s, and s * 0 = +-0 is absorbed by the
    sums it enters (they start from +0).  tests/golden/mlp_fused_bits.npz holds the weights, Adam slots and |TD errors|
    after two updates (Huber, importance weights; DQN and Double DQN) as the kernel with the select form produced them."""
    want = golden("mlp_fused_bits")
    for tag, got in fused_bits(dev).items():
        assert got.dtype == want[tag].dtype and np.array_equal(got.view(np.uint8), want[tag].view(np.uint8)), tag


def fused_bits(dev):
    """what tests/golden/mlp_fused_bits.npz records: mlp_ref.make_edge_case("done_255"), two fused updates on the same
    batch -> the weights and |TD errors| (DQN and Double DQN) and the Adam slots (Double DQN: all three towers run)"""
    out = {}
    for ddqn in (False, True):
        c, discount = R.make_edge_case("done_255", ddqn)
        f = _net(dev, c, True)
        for _ in range(2):
            _, _, td, _ = _learn(dev, f, c, discount)
        tag = "ddqn" if ddqn else "dqn"
        out[tag + "_w"], out[tag + "_td"] = f.params.weights.cpu().numpy(), td
        if ddqn:
            out[tag + "_m"], out[tag + "_v"] = f.adam.m.cpu().numpy(), f.adam.v.cpu().numpy()
    return out


def test_update_in_a_captured_graph(dev):
    """the fused update captured in one graph (a single kernel node) and replayed three times against three eager
    updates of a twin: weights, Adam slots, Adam state and |TD| bit for bit, the barrier words zero after every replay"""
    import torch
    from coach_amd.agents.vector_agent import capture
    from coach_amd import _rlx
    c, discount = R.make_edge_case("done_255")
    _learn(dev, _net(dev, c, True), c, discount)       # the kernel is loaded and its LDS attribute set before the capture
    res = {}
    for captured in (True, False):
        net = _net(dev, c, True)
        args, iw = _args(dev, c, discount), _iw(dev, c)
        td = torch.zeros(c["B"], dtype=torch.float64, device=dev)
        step = lambda: net.learn_from_batch(*args, importance_weights=iw, td_errors=td, double_dqn=False)
        if captured:
            torch.cuda.synchronize()
            calls = _rlx.CALL_COUNT
            g = capture(step)                          # (capturing runs nothing: the state is still the initial one)
            assert _rlx.CALL_COUNT - calls == 1        # one library call, which is one launch: a single kernel node
            for _ in range(3):
                g.replay()
                torch.cuda.synchronize()
                assert int(net._fused["sync"].abs().sum().item()) == 0
        else:
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        net.check_status()
        res[captured] = [x.clone() for x in (net.params.weights, net.adam.m, net.adam.v, net.adam.state, td, net.loss, net.norm)]
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
    assert float(res[True][1].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- acting
def _act_net(dev, dims, A, seed=3):
    from coach_amd.nn.networks import DQNNet
    d0, h1, h2 = dims
    rng = np.random.RandomState(seed)
    W = R.make_weights(dims, A, rng)
    net = DQNNet(dev, (d0,), A, embedder=[h1], middleware=[h2], learning_rate=1e-3, seed=seed)
    for k in R.NAMES:
        net.params.w(R.PARAM_NAMES[k]).copy_(_dv(dev, W[k], net.params.weights.dtype))
    return net, W


def _check_act(dev, net, W, dims, A, n_env, seed=0, states=None):
    """Q against the float64 forward (within its a-priori fp32 bound plus 2e-5 relative) and against net.q_values (the
    existing test's rtol 2e-5, atol 2e-6); the choice against rlx_egreedy fed the fused Q, at epsilon 0, 0.3 and 1"""
    import torch
    from coach_amd import _rlx
    lib = _rlx.lib()
    assert net.can_act_fused(n_env)
    rng = np.random.RandomState(seed)
    s = rng.randn(n_env, dims[0]).astype(np.float32) if states is None else states
    sd = _dv(dev, s, torch.float32)
    with np.errstate(invalid="ignore"):
        fw = R.forward(W, s)
    q_ref = net.q_values(sd, n_env, tag="ref").data.view(n_env, A).clone()
    for eps in (0.0, 0.3, 1.0):
        u, ra, tie = _dv(dev, rng.rand(n_env), torch.float64), _dv(dev, rng.randint(0, A, n_env), torch.int32), \
            _dv(dev, rng.rand(n_env, A), torch.float64)
        q_f = torch.zeros(n_env, A, dtype=torch.float32, device=dev)
        a_f = torch.full((n_env,), -1, dtype=torch.int32, device=dev)
        a_ref = torch.full((n_env,), -2, dtype=torch.int32, device=dev)
        net.q_act(sd, n_env, u, ra, tie, eps, q_f, a_f)
        lib.egreedy(q_f, A, u, ra, tie, eps, n_env, A, a_ref, _rlx.current_stream())
        assert torch.equal(a_f, a_ref), (eps, a_f, a_ref)
        got = q_f.cpu().numpy()
        w = _close(got, fw["q"], 2e-5, fw["eq"], "Q fused vs fp64 (%s, n_env %d)" % (dims, n_env))
        _close(got, q_ref.cpu().numpy(), 2e-5, 2e-6, "Q fused vs layer launches (%s, n_env %d)" % (dims, n_env))
    print("MEASURED q_act %s A=%d n_env=%d: worst Q error %.3g of its fp64 bound" % (dims, A, n_env, w))
    return q_f, a_f


@pytest.mark.parametrize("n_env", range(1, 9))
def test_q_act_every_env_count(dev, n_env):
    """one template instantiation each"""
    net, W = _act_net(dev, (4, 64, 64), 3)
    _check_act(dev, net, W, (4, 64, 64), 3, n_env)


@pytest.mark.parametrize("dims,A,n_env", [
    ((16, 4, 4), 16, 8),          # widest input and head on the narrowest layers; xs fills its 128 floats
    ((16, 4, 4), 16, 1),
    ((1, 1024, 4), 2, 1),         # one group of four units, 1024 slices of four rows
    ((1, 4, 1024), 2, 1),         # four slices of which one has rows
    ((8, 100, 160), 5, 3),        # H1 no multiple of 4 * S: 17 slices of 8 rows, the 13th ragged (4 rows), four empty
])
def test_q_act_shape_edges(dev, dims, A, n_env):
    net, W = _act_net(dev, dims, A)
    _check_act(dev, net, W, dims, A, n_env)


@pytest.mark.parametrize("n_env,largest", [(1, 768), (8, 672)])
def test_q_act_largest_square_network(dev, n_env, largest):
    """the largest h1 = h2 rlx_mlp_q_act_supported accepts (64 KB of LDS: 8 (32 + 2 h) + n_env S h floats; 768 with five
    slices fills it to the byte), found by calling it; the next multiple of 4 is refused"""
    from coach_amd import _rlx
    sup = _rlx.lib().rlx_mlp_q_act_supported
    ok = [h for h in range(4, 1028, 4) if sup(n_env, 4, h, h, 3)]
    assert max(ok) == largest and not sup(n_env, 4, largest + 4, largest + 4, 3)
    net, W = _act_net(dev, (4, largest, largest), 3)
    _check_act(dev, net, W, (4, largest, largest), 3, n_env)


def test_q_act_tie_and_nan(dev):
    """Two equal maxima, made by duplicating a head column (and raising both above the rest), and a NaN in one Q value:
    the choice must be rlx_egreedy's on the same values (the tie draw decides; a NaN is the maximum)."""
    import torch
    dims, A, n_env = (4, 64, 64), 3, 5
    net, W = _act_net(dev, dims, A)
    W["w3"][:, 2] = W["w3"][:, 0]
    W["b3"][0] = W["b3"][2] = 10.0
    for k in ("w3", "b3"):
        net.params.w(R.PARAM_NAMES[k]).copy_(_dv(dev, W[k], torch.float32))
    q, _ = _check_act(dev, net, W, dims, A, n_env)
    q = q.cpu().numpy()
    assert np.array_equal(q[:, 0], q[:, 2]) and np.all(q[:, 0] > q[:, 1])
    W["b3"][1] = np.nan
    net.params.w(R.PARAM_NAMES["b3"]).copy_(_dv(dev, W["b3"], torch.float32))
    q, a = _check_act(dev, net, W, dims, A, n_env)
    assert np.isnan(q.cpu().numpy()[:, 1]).all() and np.isfinite(q.cpu().numpy()[:, [0, 2]]).all()
