"""The factorised NoisyNet dense layer on the MI355X (nn.graph.NoisyDense, csrc/noisy_dense.hip, rlx_noisy_sample)
against the numpy twin tests/noisy_ref.py: the noise bit for bit, forward and all five gradients at the shapes that occur,
zero stddev against the plain dense layer, fresh noise per pass, also per replay of a captured graph."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noisy_ref as R  # noqa: E402
from tolerances import LOSS, OUT  # noqa: E402

pytestmark = pytest.mark.gpu
SEED, RANK = 11, 2


def _sample(dev, specs, noise_pass, counters):
    """specs: [(layer index, K, N)] -> per spec (fp32 vector, fp64 vector) as numpy, one launch"""
    import torch
    from coach_amd import _rlx
    arr = (_rlx.NoisyLayer * len(specs))()
    bufs = []
    for q, (layer, K, N) in zip(arr, specs):
        f = torch.zeros(K + 2 * N, dtype=torch.float32, device=dev)
        f64 = torch.zeros(K + 2 * N, dtype=torch.float64, device=dev)
        q.f, q.f64, q.K, q.N, q.layer = f.data_ptr(), f64.data_ptr(), K, N, layer
        bufs.append((f, f64))
    _rlx.lib().noisy_sample(ctypes.byref(arr), len(arr), counters, noise_pass, SEED, RANK, _rlx.current_stream())
    torch.cuda.synchronize()
    return [(f.cpu().numpy(), f64.cpu().numpy()) for f, f64 in bufs]


def test_noise_equals_the_twin_bit_for_bit(dev):
    import torch
    from coach_amd import _rlx
    specs = [(0, 4, 256), (1, 256, 512), (2, 3136, 7), (5, 33, 306)]
    counters = torch.zeros(8 * _rlx.NOISY_PASSES, dtype=torch.int64, device=dev)
    start = {0: 0, 1: 3, 2: (1 << 32) + 5, 5: 77}
    for noise_pass in (0, 1, 3):
        for layer, c in start.items():
            counters[layer * _rlx.NOISY_PASSES + noise_pass] = c
        for rep in range(2):                                  # the launch advances its counters itself
            got = _sample(dev, specs, noise_pass, counters)
            for (layer, K, N), (f32, f64) in zip(specs, got):
                ref = np.concatenate(R.noise(SEED, RANK, layer, noise_pass, start[layer] + rep, K, N))
                assert np.array_equal(f64.view(np.uint64), ref.view(np.uint64)), (layer, noise_pass, rep)
                assert np.array_equal(f32.view(np.uint32), ref.astype(np.float32).view(np.uint32)), (layer, noise_pass)
        for layer, c in start.items():
            assert int(counters[layer * _rlx.NOISY_PASSES + noise_pass].item()) == c + 2


def _layer(dev, K, N, act, seed=0):
    from coach_amd.nn import graph as G
    params = G.FlatParams()
    layer = G.NoisyDense(params, "l", K, N, act)
    params.finalize(dev)
    layer.initialize(np.random.RandomState(seed))
    layer.index = 0
    return G, params, layer, G.Context(dev)


def _close(name, got, ref, tol, relative_to_max=False):
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    bound = tol["atol"] + tol["rtol"] * (np.abs(ref).max() if relative_to_max else np.abs(ref))
    print("%-10s worst |error| %.3e  worst error / bound %.3f  (largest |reference| %.3e)"
          % (name, err.max(), (err / bound).max(), np.abs(ref).max()))
    assert (err <= bound).all(), name


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("M,K,N", [(32, 3136, 512), (32, 512, 306), (32, 512, 2), (1, 4, 256), (64, 512, 512)])
def test_forward_and_gradients_against_the_twin(dev, M, K, N, act):
    """outputs within OUT; the five gradients within LOSS relative to the gradient's largest magnitude"""
    import torch
    G, params, layer, ctx = _layer(dev, K, N, act)
    rng = np.random.RandomState(M + K + N)
    params.w(layer.bmname).copy_(torch.from_numpy((0.1 * rng.randn(N)).astype(np.float32)))
    x_np = (np.abs(rng.randn(M, K)) * (rng.rand(M, K) > 0.4)).astype(np.float32)       # a relu layer's output
    counters = torch.zeros(G._rlx.NOISY_PASSES, dtype=torch.int64, device=dev)
    counters[1] = 9
    import ctypes as C
    arr = (G._rlx.NoisyLayer * 1)()
    arr[0].f, arr[0].f64, arr[0].K, arr[0].N, arr[0].layer = layer.noise(ctx, "train").data_ptr(), None, K, N, 0
    ctx.lib.noisy_sample(C.byref(arr), 1, counters, 1, SEED, RANK, ctx.stream)
    f_in, f_out, f_b = R.noise_f32(SEED, RANK, 0, 1, 9, K, N)
    assert np.array_equal(layer.noise(ctx, "train").cpu().numpy(), np.concatenate([f_in, f_out, f_b]))
    x = G.Tensor(torch.from_numpy(x_np).to(dev).view(1, M, K), M, K, 1, act="relu")
    y = layer.forward(ctx, x, tag="train")
    w = {n: params.w(getattr(layer, n)).cpu().numpy() for n in ("wmname", "wsname", "bmname", "bsname")}
    y_ref = R.forward(x_np, w["wmname"], w["wsname"], w["bmname"], w["bsname"], f_in, f_out, f_b, act)
    _close("y", y.data.cpu().numpy().reshape(M, N), y_ref, OUT)
    dy = rng.randn(M, N).astype(np.float32)
    y.ensure_grad().copy_(torch.from_numpy(dy).to(dev).view(1, M, N))
    layer.backward(ctx, x, y)
    torch.cuda.synchronize()
    dz = dy.astype(np.float64) * R.act_deriv(y.data.cpu().numpy().reshape(M, N).astype(np.float64), act)
    ref = R.backward(x_np, w["wmname"], w["wsname"], dz, f_in, f_out, f_b, "relu")
    assert x.grad_is_dz
    for key, got in (("dwm", params.g(layer.wmname)), ("dws", params.g(layer.wsname)), ("dbm", params.g(layer.bmname)),
                     ("dbs", params.g(layer.bsname)), ("dx", x.grad.view(M, K))):
        _close(key, got.cpu().numpy(), ref[key], LOSS, relative_to_max=True)


@pytest.mark.parametrize("M,K,N", [(32, 3136, 512), (32, 512, 2), (1, 4, 256)])
def test_zero_stddev_equals_the_plain_dense_layer(dev, M, K, N):
    import torch
    G, params, layer, ctx = _layer(dev, K, N, "relu")
    params.w(layer.wsname).zero_()
    params.w(layer.bsname).zero_()
    plain_params = G.FlatParams()
    plain = G.Dense(plain_params, "p", K, N, "relu")
    plain_params.finalize(dev)
    plain_params.w(plain.kname).copy_(params.w(layer.wmname))
    rng = np.random.RandomState(4)
    bias = torch.from_numpy((0.1 * rng.randn(N)).astype(np.float32)).to(dev)
    params.w(layer.bmname).copy_(bias)
    plain_params.w(plain.bname).copy_(bias)
    layer.noise(ctx, "t").copy_(torch.from_numpy(rng.randn(K + 2 * N).astype(np.float32)))
    x = torch.from_numpy(rng.randn(M, K).astype(np.float32)).to(dev).view(1, M, K)
    y = layer.forward(ctx, G.Tensor(x, M, K, 1), tag="t").data.cpu().numpy()
    y_plain = plain.forward(ctx, G.Tensor(x, M, K, 1), tag="t").data.cpu().numpy()
    _close("y", y, y_plain, OUT)


def test_relu_keeps_a_nan_bias_mean(dev):
    """One NaN bias-mean entry: that column is NaN in every row, as np.maximum(z, 0) leaves it (v > 0 ? v : 0 made it 0);
    the other columns keep the bits of the run without the NaN."""
    import torch
    M, K, N, col = 1, 4, 256, 77
    G, params, layer, ctx = _layer(dev, K, N, "relu")
    rng = np.random.RandomState(5)
    layer.noise(ctx, "t").copy_(torch.from_numpy(rng.randn(K + 2 * N).astype(np.float32)))
    x = torch.from_numpy(rng.randn(M, K).astype(np.float32)).to(dev).view(1, M, K)
    clean = layer.forward(ctx, G.Tensor(x, M, K, 1), tag="t").data.cpu().numpy().reshape(M, N)
    params.w(layer.bmname)[col] = float("nan")
    got = layer.forward(ctx, G.Tensor(x, M, K, 1), tag="t").data.cpu().numpy().reshape(M, N)
    nan = np.zeros((M, N), bool)
    nan[:, col] = True
    assert not np.isnan(clean).any() and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), clean[~nan].view(np.uint32))


def test_every_pass_and_every_graph_replay_draws_its_own_noise(dev):
    import torch
    from coach_amd.nn.networks import DQNNet
    net = DQNNet(dev, (4,), 2, noisy=True, seed=1)
    net.noise_seed, net.noise_rank = SEED, RANK
    assert net._fused is None and net._act is None and len(net.noisy_layers) == 3
    obs = torch.from_numpy(np.random.RandomState(0).randn(3, 4).astype(np.float32)).to(dev)
    names = net.params.named_arrays()

    def twin(counter):
        h = obs.cpu().numpy()
        for l in net.noisy_layers:
            f = R.noise_f32(SEED, RANK, l.index, R.PASS["act"], counter, l.K, l.N)
            h = R.forward(h, names[l.wmname][0], names[l.wsname][0], names[l.bmname][0], names[l.bsname][0], *f, l.act)
        return h

    outs = [net.q_values(obs, 3, tag="act").data.cpu().numpy().reshape(3, 2).copy() for _ in range(2)]
    assert not np.array_equal(outs[0], outs[1])
    for c, o in enumerate(outs):
        _close("eager %d" % c, o, twin(c), OUT)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.q_values(obs, 3, tag="act")                      # counter 2: warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            q = net.q_values(obs, 3, tag="act").data
    torch.cuda.current_stream().wait_stream(side)
    replays = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        replays.append(q.cpu().numpy().reshape(3, 2).copy())
    assert not np.array_equal(replays[0], replays[1])
    for c, o in zip((3, 4), replays):
        _close("replay %d" % c, o, twin(c), OUT)
    assert int(net.noise_counters[0].item()) == 5
