"""Direct Future Prediction on the device: rlx_dfp_head_loss, rlx_dfp_egreedy / rlx_dfp_argmax and
rlx_dfp_future_measurements (csrc/dfp.hip) against the numpy restatement (tests/dfp_ref.py, itself pinned to the
reference agent by tests/test_dfp_ref.py) on the recorded shapes of tests/golden/dfp.npz, and the leaky_relu activation
of the generic dense path (rlx_dense_small_*, rlx_leaky_relu behind rlx_gemm, rlx_act_backward) against numpy.

Everything the DFP launches write is compared bit for bit: the file is compiled without FMA contraction and the
restatement states every rounding.  The leaky dense layer is held to the tolerances tests/test_architecture.py uses for
dense outputs (rtol 1e-3, atol 1e-4)."""
import numpy as np
import pytest

import dfp_ref as R
from dfp_ref import ACT_CASES, ACT_STEPS, LEARN_CASES, LENGTHS, MEAS, SCALES, STEPS

pytestmark = pytest.mark.gpu

DENSE = dict(rtol=1e-3, atol=1e-4)          # tests/test_architecture.py: dense outputs against the oracle


def _t(x, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(name, got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, ref.dtype, got.shape, ref.shape)
    assert np.array_equal(_bits(got), _bits(ref)), "%s differs in %d of %d elements" % (
        name, int((_bits(got) != _bits(ref)).sum()), got.size)


def _loss(rlx, dev, E, X, actions, future, grad_scale=1.0, pad=0):
    """-> dict of everything the launch writes; pad: extra columns in every leading dimension."""
    import torch
    B, A, K = X.shape

    def padded(a, cols):
        buf = np.full((B, cols + pad), np.float32(np.nan))
        buf = buf.astype(np.float32)
        buf[:, :cols] = a.reshape(B, cols)
        return _t(buf, dev)
    dE = torch.full((B, K + pad), float("nan"), dtype=torch.float32, device=dev)
    dX = torch.full((B, A * K + pad), float("nan"), dtype=torch.float32, device=dev)
    y = torch.full((B, A * K), float("nan"), dtype=torch.float32, device=dev)
    tg = torch.full((B, A * K), float("nan"), dtype=torch.float32, device=dev)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(256, dtype=torch.float32, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    out = []
    for _ in range(2):                                    # twice: the ticket is left at zero, the result is the same bits
        rlx.dfp_head_loss(padded(E, K), K + pad, padded(X, A * K), A * K + pad, _t(actions.astype(np.int32), dev),
                          _t(np.asarray(future).astype(np.float32).reshape(B, K), dev), A, K, B, grad_scale, dE, K + pad,
                          dX, A * K + pad, ws, ticket, loss, status, y, tg, 0)
        torch.cuda.synchronize()
        out.append(dict(y=y.cpu().numpy().reshape(B, A, K), targets=tg.cpu().numpy().reshape(B, A, K),
                        loss=loss.cpu().numpy()[0], dE=dE.cpu().numpy()[:, :K],
                        dX=dX.cpu().numpy()[:, :A * K].reshape(B, A, K), status=int(status.item()),
                        ticket=int(ticket.item())))
    for key in ("y", "targets", "dE", "dX"):
        _same(key + " (second launch)", out[1][key], out[0][key])
    assert out[0]["loss"].tobytes() == out[1]["loss"].tobytes() and out[1]["ticket"] == 0
    if pad:
        assert np.isnan(dE.cpu().numpy()[:, K:]).all() and np.isnan(dX.cpu().numpy()[:, A * K:]).all()
    return out[0]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("case", range(len(LEARN_CASES)))
def test_head_loss_equals_the_restatement_bit_for_bit(rlx, dev, golden, case, pad):
    g = golden("dfp")
    p = "learn%d_" % case
    B, A, S, M = LEARN_CASES[case]
    E, X, actions, future = g[p + "E"], g[p + "X"], g[p + "actions"], g[p + "future"]
    assert X.shape == (B, A, S * M)
    for scale in (1.0, 0.5):
        k = _loss(rlx, dev, E, X, actions, future, scale, pad)
        r = R.head_loss(E, X, actions, future, scale)
        print("\n  case %s scale %g: loss %.9g (restatement %.9g)" % ((B, A, S, M), scale, k["loss"], r["loss"]))
        assert k["status"] == 0 and k["ticket"] == 0
        for key in ("y", "targets", "dE", "dX"):
            _same(key, k[key], r[key])
        assert k["loss"].tobytes() == r["loss"].tobytes()
    # the reference keeps the NaNs in the targets it hands to the head, whose tf.where puts the prediction there
    rec = g[p + "targets"]
    assert np.array_equal(np.isnan(rec)[np.arange(B), actions], np.isnan(future.reshape(B, -1)))
    _same("recorded targets", k["targets"], np.where(np.isnan(rec), k["y"], rec))
    nan_rows = np.isnan(future.reshape(B, -1)).all(axis=1)
    if B > 1:
        assert nan_rows.any()
    assert np.all(k["dE"][nan_rows] == 0.0) and np.all(k["dX"][nan_rows] == 0.0)
    assert not np.isnan(k["dE"]).any() and not np.isnan(k["dX"]).any() and np.any(k["dE"] != 0.0)


def test_head_loss_flags_an_invalid_action_and_refuses_large_shapes(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    rng = np.random.RandomState(7)
    B, A, K = 4, 3, 5
    E, X = rng.randn(B, K).astype(np.float32), rng.randn(B, A, K).astype(np.float32)
    future = rng.randn(B, K).astype(np.float32)
    for bad in (3, -1):
        actions = np.array([0, bad, 1, 2])
        k, r = _loss(rlx, dev, E, X, actions, future), R.head_loss(E, X, actions, future)
        assert k["status"] == 1 == r["status"]
        assert np.all(k["dE"][1] == 0.0) and np.all(k["dX"][1] == 0.0) and np.any(k["dE"][0] != 0.0)
        for key in ("y", "targets", "dE", "dX"):
            _same(key, k[key], r[key])
        assert k["loss"].tobytes() == r["loss"].tobytes()
    buf = torch.zeros(257, 19 * 65, dtype=torch.float32, device=dev)
    ints = torch.zeros(257, dtype=torch.int32, device=dev)
    ld = 19 * 65
    for A_, K_, B_ in ((2, 4, 257), (19, 4, 2), (2, 65, 2), (0, 4, 2), (2, 0, 2)):
        with pytest.raises(RlxError):
            rlx.dfp_head_loss(buf, ld, buf, ld, ints, buf, A_, K_, B_, 1.0, buf, ld, buf, ld, buf, ints, buf, ints, None,
                              None, 0)
    with pytest.raises(RlxError):                         # a leading dimension below A * K
        rlx.dfp_head_loss(buf, ld, buf, 7, ints, buf, 2, 4, 2, 1.0, buf, ld, buf, ld, buf, ints, buf, ints, None, None, 0)
    assert int(ints.sum().item()) == 0


@pytest.mark.parametrize("A", [1, 2, 6, 18])
def test_merge_with_one_column_equals_dueling_combine(rlx, dev, A):
    import torch
    rng = np.random.RandomState(A)
    B = 37
    E = rng.randn(B, 1).astype(np.float32)
    X = (rng.randn(B, A, 1) * 3).astype(np.float32)
    X[0] = -0.0                                           # a zero sum: the one place where the sum's start matters
    X[1] = 0.0
    k = _loss(rlx, dev, E, X, np.zeros(B, np.int64), np.zeros((B, 1), np.float32))
    q = torch.full((B, A), float("nan"), dtype=torch.float32, device=dev)
    rlx.dueling_combine(_t(E.reshape(B), dev), _t(X.reshape(B, A), dev), B, A, q, 0)
    _same("y", k["y"].reshape(B, A), q.cpu().numpy())
    _same("restatement", R.merge(E, X).reshape(B, A), q.cpu().numpy())


def _future(rlx, dev, meas_col, out_col, scale, s0, T, env, n_env, ring, S, M, last_step):
    import torch
    rlx.dfp_future_measurements(meas_col, out_col, _t(np.asarray(scale, np.float64), dev), s0, T, env, n_env, ring, S, M,
                                int(last_step), 0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("M", MEAS)
@pytest.mark.parametrize("T", LENGTHS)
def test_future_measurements_equal_the_recording(rlx, dev, golden, T, M):
    """every recorded case of this (T, M), in three layouts: the episode alone in a ring of its own length; in env 1 of
    two with sentinel rows around it; wrapped around the end of the ring."""
    import torch
    g = golden("dfp")
    meas = g["fm_T%d_M%d_meas" % (T, M)]
    layouts = ((1, 0, T, 0), (2, 1, T + 7, 3), (2, 1, T + 2, 5), (3, 2, T, T // 2 + 1))   # (n_env, env, ring, s0)
    for S in STEPS:
        for mode in ("NAN", "LastStep"):
            for sname, scale in SCALES.items():
                want = g["fm_T%d_M%d_S%d_%s_%s" % (T, M, S, mode, sname)].astype(np.float32)
                for n_env, env, ring, s0 in layouts:
                    rows = ring * n_env
                    col = np.full((rows, M), 1e300)
                    own = [((s0 + k) % ring) * n_env + env for k in range(T)]
                    col[own] = meas
                    sentinel = np.float32(-77.25)
                    out = torch.full((rows, S * M), float(sentinel), dtype=torch.float32, device=dev)
                    _future(rlx, dev, _t(col, dev), out, scale[:M], s0, T, env, n_env, ring, S, M, mode == "LastStep")
                    got = out.cpu().numpy()
                    _same("T%d M%d S%d %s %s layout %s" % (T, M, S, mode, sname, (n_env, env, ring, s0)),
                          got[own].reshape(T, S, M), want)
                    others = np.setdiff1d(np.arange(rows), own)
                    assert np.all(got[others] == sentinel)
                _same("restatement", R.future_measurements(meas, S, scale[:M], mode == "LastStep"), want)


def test_future_measurements_refuses_bad_shapes(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    col = torch.zeros(16, 8, dtype=torch.float64, device=dev)
    out = torch.zeros(16, 64, dtype=torch.float32, device=dev)
    for S, M, T, env, n_env, ring, mode in ((9, 1, 4, 0, 1, 4, 0), (1, 9, 4, 0, 1, 4, 0), (2, 2, 5, 0, 1, 4, 0),
                                            (2, 2, 4, 1, 1, 4, 0), (2, 2, 0, 0, 1, 4, 0), (2, 2, 4, 0, 1, 4, 2)):
        with pytest.raises(RlxError):
            rlx.dfp_future_measurements(col, out, col, 0, T, env, n_env, ring, S, M, mode, 0)


def _act(rlx, dev, E, X, goal, weights, S, M, explore_u, random_actions, tie, epsilon):
    import torch
    n, A, K = X.shape
    q = torch.full((n, A), float("nan"), dtype=torch.float64, device=dev)
    acts = torch.full((n,), -1, dtype=torch.int32, device=dev)
    gd, wd = _t(np.asarray(goal, np.float64), dev), _t(np.asarray(weights, np.float64), dev)
    Ed, Xd = _t(E, dev), _t(X.reshape(n, A * K), dev)
    rlx.dfp_egreedy(Ed, K, Xd, A * K, gd, wd, S, M, len(weights), _t(explore_u, dev), _t(random_actions.astype(np.int32), dev),
                    _t(tie, dev), epsilon, n, A, q, acts, 0)
    q2 = torch.full((n, A), float("nan"), dtype=torch.float64, device=dev)
    greedy = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rlx.dfp_argmax(Ed, K, Xd, A * K, gd, wd, S, M, len(weights), n, A, q2, greedy, 0)
    none = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rlx.dfp_argmax(Ed, K, Xd, A * K, gd, wd, S, M, len(weights), n, A, None, none, 0)
    torch.cuda.synchronize()
    assert np.array_equal(greedy.cpu().numpy(), none.cpu().numpy())
    _same("argmax scores", q2.cpu().numpy(), q.cpu().numpy())
    return q.cpu().numpy(), acts.cpu().numpy(), greedy.cpu().numpy()


@pytest.mark.parametrize("case", range(len(ACT_CASES)))
def test_action_scores_are_the_recorded_ones_and_the_choice_is_the_shared_one(rlx, dev, golden, case):
    g = golden("dfp")
    A, M, W = ACT_CASES[case]
    p = "act%d_" % case
    E, X, want, goal, weights = g[p + "E"], g[p + "X"], g[p + "scores"], g[p + "goal"], g[p + "weights"]
    n = len(E)
    assert len(goal) == M and len(weights) == W and want.shape == (n, A)
    rng = np.random.RandomState(case)
    explore_u, random_actions, tie = rng.rand(n), rng.randint(0, A, size=n), rng.rand(n, A)
    explore_u[1] = 0.0                                    # a row that explores whatever epsilon is
    q, acts, greedy = _act(rlx, dev, E, X, goal, weights, ACT_STEPS, M, explore_u, random_actions, tie, 0.3)
    _same("scores", q, want)
    _same("restatement", R.scores(E, X, goal, weights, ACT_STEPS, M), want)
    assert np.array_equal(acts, R.egreedy(want, explore_u, random_actions, tie, 0.3))
    assert np.array_equal(greedy, np.argmax(want, axis=1))
    assert acts[1] == random_actions[1]


def test_a_tie_is_broken_by_the_draws_and_argmax_takes_the_first(rlx, dev, golden):
    g = golden("dfp")
    case = len(ACT_CASES) - 1
    A, M, W = ACT_CASES[case]
    p = "act%d_" % case
    E, X, want = g[p + "E"][:1], g[p + "X"][:1], g[p + "scores"][:1]
    assert want[0, 0] == want[0, A - 1] == want[0].max() and np.sum(want[0] == want[0].max()) == 2
    seen = set()
    for seed in range(6):
        tie = np.random.RandomState(seed).rand(1, A)
        q, acts, greedy = _act(rlx, dev, E, X, g[p + "goal"], g[p + "weights"], ACT_STEPS, M, np.ones(1),
                               np.zeros(1, np.int64), tie, 0.0)
        _same("scores", q, want)
        assert acts[0] == (0 if tie[0, 0] > tie[0, A - 1] else A - 1) == R.egreedy(want, np.ones(1), np.zeros(1), tie, 0.0)[0]
        assert greedy[0] == 0
        seen.add(int(acts[0]))
    assert seen == {0, A - 1}


def test_acting_refuses_bad_shapes(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    f32 = torch.zeros(4, 19 * 65, dtype=torch.float32, device=dev)
    f64 = torch.zeros(64, dtype=torch.float64, device=dev)
    ints = torch.zeros(64, dtype=torch.int32, device=dev)
    ld = 19 * 65
    for S, M, W, A in ((6, 1, 7, 2), (6, 1, 0, 2), (9, 8, 1, 2), (6, 1, 3, 19), (6, 1, 3, 0)):
        with pytest.raises(RlxError):
            rlx.dfp_egreedy(f32, ld, f32, ld, f64, f64, S, M, W, f64, ints, f64, 0.1, 2, A, None, ints, 0)
        with pytest.raises(RlxError):
            rlx.dfp_argmax(f32, ld, f32, ld, f64, f64, S, M, W, 2, A, None, ints, 0)
    with pytest.raises(RlxError):
        rlx.dfp_argmax(f32, 5, f32, ld, f64, f64, 6, 1, 3, 2, 2, None, ints, 0)


def test_accumulated_reward_measurement_lags_by_one_step(rlx, dev):
    """three envs whose episodes end on different steps, two measurements per state (the accumulated reward is column
    1; column 0 is left alone): every state's measurement equals the restatement of the reference's injection order."""
    import torch
    rng = np.random.RandomState(5)
    n, M, steps = 3, 2, 12
    rewards = (rng.rand(steps, n) * 3 + 0.1).astype(np.float32)
    over = np.zeros((steps, n), bool)
    over[[3, 8], 0] = True
    over[[0, 1, 11], 1] = True
    acc = torch.zeros(n, dtype=torch.float64, device=dev)
    cur = torch.zeros(n, M, dtype=torch.float64, device=dev)
    cur[:, 0] = 7.5
    cur32 = torch.zeros(n, M, dtype=torch.float32, device=dev)
    state = torch.full((n, M), float("nan"), dtype=torch.float64, device=dev)
    got_state, got_next = [], []
    for t in range(steps):
        rlx.dfp_accumulated_reward_step(_t(rewards[t], dev), _t(over[t].astype(np.uint8), dev), acc, cur, cur32,
                                        state if t % 2 == 0 else None, n, M, 1, 0)
        if t % 2 == 0:
            got_state.append((t, state.cpu().numpy().copy()))
        got_next.append(cur.cpu().numpy().copy())
        assert np.array_equal(cur32.cpu().numpy()[:, 1], got_next[-1][:, 1].astype(np.float32))
    got_next = np.stack(got_next)
    assert np.all(got_next[:, :, 0] == 7.5)
    for e in range(n):
        want, start = [], 0                         # the measurement of the state AFTER every step
        for end in list(np.nonzero(over[:, e])[0]) + [steps - 1]:
            m = R.accumulated_reward_measurements(rewards[start:end + 1, e])
            want.extend(m[1:] if not over[end, e] else list(m[1:-1]) + [0.0])     # a game over: the new episode's s_0
            start = end + 1
            if start >= steps:
                break
        _same("env %d" % e, got_next[:, e, 1], np.array(want[:steps]))
        for t, s in got_state:                      # the state the step was taken in: the previous step's next state
            assert s[e, 1] == (got_next[t - 1, e, 1] if t else 0.0) and s[e, 0] == 7.5
    from coach_amd._rlx import RlxError
    for M_, col in ((9, 0), (2, 2), (2, -1), (0, 0)):
        with pytest.raises(RlxError):
            rlx.dfp_accumulated_reward_step(_t(rewards[0], dev), _t(over[0].astype(np.uint8), dev), acc, cur, None, None, n,
                                            M_, col, 0)


# ------------------------------------------------------------------------------------------- the leaky activation
def _leaky(v):
    return np.where(v > 0, v, 0.2 * v)


def _leaky_deriv(y):
    return np.where(y > 0, 1.0, 0.2)


# (towers, do they share one input, the lower layer's activation, are the two gradient products one launch); the
# shared-input path never pairs its products, so it is listed with pair = True only
_LEAKY_PATHS = [(T, shared, lower, pair) for T, shared in ((1, False), (2, False), (2, True))
                for lower in ("leaky_relu", None) for pair in (True, False) if pair or not shared]


@pytest.mark.parametrize("T,shared,lower,pair", _LEAKY_PATHS)
@pytest.mark.parametrize("M,K,N", [(5, 3, 7), (64, 768, 256)])
def test_leaky_dense_layer_forward_and_backward(dev, monkeypatch, M, K, N, T, shared, lower, pair):
    """A G.Dense layer with leaky_relu on the launches it can pick: the narrow-dense forward and backward launches
    (N = 7; the backward one folds the LOWER layer's leaky derivative into dx), the tiled / folded GEMM followed by
    rlx_leaky_relu, rlx_act_backward, the weight- and input-gradient products alone or paired and accumulated over towers
    that share their input — whose epilogues decline the leaky derivative, so that x.grad stays the plain input gradient."""
    import torch
    from coach_amd.nn import graph as G
    monkeypatch.setattr(G, "PAIR_GRADIENT_GEMMS", pair)
    rng = np.random.RandomState(M + N + T)
    params = G.FlatParams()
    layer = G.Dense(params, "l", K, N, "leaky_relu", T)
    params.finalize(dev)
    layer.initialize(rng)
    w = np.stack([params.w(layer.kname, t).cpu().numpy().reshape(K, N) for t in range(T)]).astype(np.float64)
    b = (0.1 * rng.randn(T, N)).astype(np.float32)
    for t in range(T):
        params.w(layer.bname, t).copy_(torch.from_numpy(b[t]).to(dev).view_as(params.w(layer.bname, t)))
    xt = 1 if shared else T
    x_np = _leaky(rng.randn(xt, M, K)).astype(np.float32)            # a leaky layer's output: both signs
    ctx = G.Context(dev)
    xd = torch.from_numpy(x_np).to(dev)
    x = G.Tensor(xd, M, K, 0 if shared else T, act=lower)
    y = layer.forward(ctx, x)
    xin = np.broadcast_to(x_np.astype(np.float64), (T, M, K)) if shared else x_np.astype(np.float64)
    z = np.einsum("tmk,tkn->tmn", xin, w) + b[:, None, :].astype(np.float64)
    y_ref = _leaky(z)
    got_y = y.data.cpu().numpy().reshape(T, M, N)
    np.testing.assert_allclose(got_y, y_ref, **DENSE)
    assert (got_y < 0).any() and (got_y > 0).any()
    dy = rng.randn(T, M, N).astype(np.float32)
    y.ensure_grad().copy_(torch.from_numpy(dy).to(dev).view_as(y.ensure_grad()))
    layer.backward(ctx, x, y)
    ctx.flush_deferred()
    torch.cuda.synchronize()
    dz = dy.astype(np.float64) * _leaky_deriv(got_y.astype(np.float64))
    dw = np.einsum("tmk,tmn->tkn", xin, dz)
    dx = np.einsum("tmn,tkn->tmk", dz, w)
    if shared:
        dx = dx.sum(axis=0, keepdims=True)
    folded = lower is not None and N <= G.SMALL_N and M * N <= 1024 and not shared      # the narrow-dense backward launch
    if folded:
        dx = dx * _leaky_deriv(x_np.astype(np.float64))
    assert x.grad_is_dz == folded
    for t in range(T):
        np.testing.assert_allclose(params.g(layer.kname, t).cpu().numpy().reshape(K, N), dw[t], **DENSE)
        np.testing.assert_allclose(params.g(layer.bname, t).cpu().numpy().reshape(N), dz[t].sum(axis=0), **DENSE)
    np.testing.assert_allclose(x.grad.cpu().numpy().reshape(xt, M, K), dx, **DENSE)


def test_leaky_activation_codes_and_act_backward(rlx, dev):
    import torch
    from coach_amd import _rlx
    assert _rlx.ACT["leaky_relu"] == 3 and _rlx.ABI_VERSION == 11
    y = np.array([-2.0, -0.0, 0.0, 1e-30, 3.0, -1e-30, 5.0], np.float32)
    dy = torch.full((7,), 2.0, dtype=torch.float32, device=dev)
    rlx.act_backward(dy, _t(y, dev), 7, _rlx.ACT["leaky_relu"], 0)
    assert np.array_equal(dy.cpu().numpy(), np.float32(2.0) * np.where(y > 0, np.float32(1.0), np.float32(0.2)))
    with pytest.raises(_rlx.RlxError):
        rlx.act_backward(dy, _t(y, dev), 7, 4, 0)
    v = np.array([-2.5, -0.0, 0.0, 1e-30, 3.0, -1e-30, 5.0] * 100, np.float32)
    out = _t(v, dev)
    rlx.leaky_relu(out, out.numel(), 0)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.where(v > 0, v, np.float32(0.2) * v).view(np.uint32))


def test_a_leaky_layer_offered_to_a_fused_launch_raises(rlx, dev):
    """the launches that do not implement it keep refusing an activation above 2, and the graph layer's adapters never
    send them one: NoisyDense raises when built, its backward pass declines a leaky lower layer."""
    import torch
    from coach_amd import _rlx
    from coach_amd.nn import graph as G
    leaky = _rlx.ACT["leaky_relu"]
    f = torch.zeros(64, 64, dtype=torch.float32, device=dev)
    with pytest.raises(_rlx.RlxError, match="unknown activation"):
        rlx.noisy_dense_forward(f, 8, f, f, f, f, f, f, 8, 4, 8, 8, leaky, f, f.numel(), 0)
    with pytest.raises(_rlx.RlxError, match="unknown activation"):
        rlx.noisy_dense_backward(f, 8, f, f, f, 8, f, f, f, f, f, f, 8, 4, 8, 8, leaky, f, f.numel(), 0)
    with pytest.raises(_rlx.RlxError, match="unknown activation"):
        rlx.bn_forward(f, f, f, f, f, 4, 8, 1e-3, 1, leaky, f, f, f, 0)
    with pytest.raises(_rlx.RlxError, match="unknown activation"):          # the GEMM epilogues were left as they are
        _rlx.gemm(8, 8, 8, f, f, f, activation="leaky_relu")
    with pytest.raises(_rlx.RlxError, match="unknown activation"):
        _rlx.gemm(8, 8, 8, f, f, f, deriv_aux=f, deriv_kind="leaky_relu")
    with pytest.raises(NotImplementedError):
        G.NoisyDense(G.FlatParams(), "n", 8, 8, "leaky_relu")
    wide = G.Dense(G.FlatParams(), "w", 8, 64, "leaky_relu")
    with pytest.raises(NotImplementedError):                                 # no deferred form of a wide leaky layer
        wide.forward(G.Context(dev), G.Tensor(f[:8, :8].contiguous().view(1, 8, 8), 8, 8, 1), launch=False)
    # a NoisyDense layer above a leaky Dense layer: the noisy backward launch is not handed the leaky derivative
    params = G.FlatParams()
    low = G.Dense(params, "low", 6, 8, "leaky_relu")
    top = G.NoisyDense(params, "top", 8, 4, None)
    params.finalize(dev)
    rng = np.random.RandomState(0)
    low.initialize(rng)
    top.initialize(rng)
    top.index = 0
    ctx = G.Context(dev)
    top.noise(ctx, "").zero_()
    params.w(top.wsname).zero_()
    x = G.Tensor(torch.from_numpy(rng.randn(1, 5, 6).astype(np.float32)).to(dev), 5, 6, 1)
    h = low.forward(ctx, x)
    y = top.forward(ctx, h)
    dy = rng.randn(5, 4).astype(np.float32)
    y.ensure_grad().copy_(torch.from_numpy(dy).to(dev).view(1, 5, 4))
    top.backward(ctx, h, y)
    assert h.grad_is_dz is False
    low.backward(ctx, x, h, need_dx=False)
    torch.cuda.synchronize()
    hv = h.data.cpu().numpy().reshape(5, 8).astype(np.float64)
    wt = params.w(top.wmname).cpu().numpy().reshape(8, 4).astype(np.float64)
    dz = (dy.astype(np.float64) @ wt.T) * _leaky_deriv(hv)
    np.testing.assert_allclose(params.g(low.kname).cpu().numpy().reshape(6, 8),
                               x.data.cpu().numpy().reshape(5, 6).astype(np.float64).T @ dz, **DENSE)
