"""G.LSTM (csrc/lstm.hip) against a plain fp64 restatement of tf BasicLSTMCell in CPU torch; its gradients from autograd."""
import numpy as np
import pytest

from tolerances import OUT

pytestmark = pytest.mark.gpu

CELLS, INPUTS = (16, 48, 128, 256), (4, 17)


def reference(kernel, bias, x, S, T, state, dy=None):
    """gate blocks i, j, f, o on [x_t | h_{t-1}] kernel + bias; rows s * T + t -> (all h_t, final c, final h, {gradients})"""
    import torch
    f64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    k, b, xt = f64(kernel).requires_grad_(), f64(bias).requires_grad_(), f64(x).requires_grad_()
    H = k.shape[1] // 4
    c, h = (f64(state[0]), f64(state[1])) if state is not None else (torch.zeros(S, H, dtype=torch.float64),) * 2
    xs, hs = xt.view(S, T, -1), []
    for t in range(T):
        i, j, f, o = (torch.cat([xs[:, t], h], 1) @ k + b).split(H, 1)
        c = c * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
        h = torch.tanh(c) * torch.sigmoid(o)
        hs.append(h)
    y = torch.stack(hs, 1).reshape(S * T, H)
    if dy is not None:
        y.backward(f64(dy))
    grads = {"dkernel": k.grad, "dbias": b.grad, "dx": xt.grad} if dy is not None else {}
    return y.detach().numpy(), c.detach().numpy(), h.detach().numpy(), {n: g.numpy() for n, g in grads.items()}


def run(dev, H, I, S, T, with_state, dy_kind=None):
    import torch
    from coach_amd.nn import graph as G
    rng = np.random.RandomState(1000 * H + 100 * I + 10 * S + T)
    params = G.FlatParams()
    layer = G.LSTM(params, "main/middleware/lstm", I, H)
    params.finalize(dev)
    layer.initialize(rng)
    params.w(layer.bname).copy_(torch.from_numpy((0.1 * rng.randn(4 * H)).astype(np.float32)))
    x_np = rng.randn(S * T, I).astype(np.float32)
    state_np = tuple(rng.uniform(-1, 1, size=(S, H)).astype(np.float32) for _ in range(2)) if with_state else None
    inp = dict(kernel=params.w(layer.kname).cpu().numpy(), bias=params.w(layer.bname).cpu().numpy(), x=x_np, state=state_np)
    ctx = G.Context(dev)
    x = G.Tensor(torch.from_numpy(x_np).to(dev).view(1, S * T, I), S * T, I, 1, act=None)
    state = tuple(torch.from_numpy(a).to(dev) for a in state_np) if with_state else None
    previous = tuple(torch.full((S, H), 7.0, device=dev) for _ in range(2))
    y = layer.forward(ctx, x, tag="t", seq=(S, T), state=state, previous=previous, save=dy_kind is not None)
    out = dict(y=y.data.view(S * T, H), c=y.lstm["final"][0], h=y.lstm["final"][1], pc=previous[0], ph=previous[1])
    if dy_kind is not None:
        inp["dy"] = dy = rng.randn(S * T, H).astype(np.float32)
        dy[-1] *= dy_kind != "bootstrap"                                       # the bootstrap row has no head gradient
        y.ensure_grad().copy_(torch.from_numpy(dy).to(dev).view(1, S * T, H))
        layer.backward(ctx, x, y)
        out.update(dkernel=params.g(layer.kname), dbias=params.g(layer.bname), dx=x.grad.view(S * T, I))
    torch.cuda.synchronize()
    return inp, {k: v.cpu().numpy().copy() for k, v in out.items()}


@pytest.mark.parametrize("with_state", [False, True])
@pytest.mark.parametrize("S,T", [(1, 1), (1, 2), (1, 21), (15, 1), (16, 1), (17, 1), (3, 5)])
@pytest.mark.parametrize("I", INPUTS)
@pytest.mark.parametrize("H", CELLS)
def test_forward(dev, H, I, S, T, with_state):
    inp, out = run(dev, H, I, S, T, with_state)
    y, c, h, _ = reference(inp["kernel"], inp["bias"], inp["x"], S, T, inp["state"])
    for got, ref in ((out["y"], y), (out["c"], c), (out["h"], h)):
        np.testing.assert_allclose(got, ref, **OUT)
    for got, before in zip((out["pc"], out["ph"]), inp["state"] if with_state else (np.zeros((S, H), np.float32),) * 2):
        assert np.array_equal(got.view(np.uint32), before.view(np.uint32))


@pytest.mark.parametrize("S,T,dy_kind", [(1, 1, "random"), (1, 2, "random"), (1, 21, "random"), (1, 21, "bootstrap"),
                                         (3, 5, "random")])
@pytest.mark.parametrize("I", INPUTS)
@pytest.mark.parametrize("H", CELLS)
def test_backward(dev, H, I, S, T, dy_kind):
    inp, out = run(dev, H, I, S, T, True, dy_kind=dy_kind)
    _, _, _, grads = reference(inp["kernel"], inp["bias"], inp["x"], S, T, inp["state"], dy=inp["dy"])
    for name, ref in grads.items():
        np.testing.assert_allclose(out[name], ref, err_msg=name, **OUT)


def test_two_runs_give_the_same_bits(dev):
    _, a = run(dev, 128, 17, 1, 21, True, dy_kind="bootstrap")
    _, b = run(dev, 128, 17, 1, 21, True, dy_kind="bootstrap")
    for name in a:
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name


@pytest.mark.parametrize("H,T,named", [(24, 3, "cells = 24"), (272, 3, "cells = 272"), (128, 0, "T = 0")])
def test_refusals_name_the_argument(dev, rlx, H, T, named):
    import torch
    from coach_amd import _rlx
    buf = torch.zeros(4 * 4 * 272, device=dev)
    with pytest.raises(_rlx.RlxError, match=named):
        rlx.lstm_forward(None, 0, buf, 4 * H, buf, 4 * H, None, None, buf, H, None, None, None, 0, 0, buf, buf, None, None,
                         1, T, H, 0)
    with pytest.raises(_rlx.RlxError, match=named):
        rlx.lstm_backward(buf, H, buf, buf, None, buf, 4 * H, buf, 1, T, H, 0)
