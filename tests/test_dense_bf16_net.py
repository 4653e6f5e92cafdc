"""G.Dense(precision="bf16") in a Sequential and in DQNNet; the public `precision` parameter and its refusals.
The Sequential's reference is torch fp64 autograd whose products round both operands to bf16 where the kernels do; every
bound is the per-product bound of tests/test_gemm_bf16.py carried through the layers: an operand known only to within
e > 0 can round to a neighbouring bf16 value (rounding is monotonic: the ends of [v - e, v + e] give the worst case),
relu' can flip where |z| <= e, and tanh is allowed 2^-22 |y|."""
import types

import numpy as np
import pytest

from tests.test_gemm_bf16 import U, bf16, bound
from tests.util import dev_tensor

DIMS, ACTS = (4, 24, 17, 3), ("relu", "tanh", None)


def rounded(v, e):
    """(bf16(v), how far the device's rounded operand can be from it); exact inputs and weights (e = 0) do not move"""
    r, e = bf16(v), np.where(e > 0, e * (1 + 2.0 ** -20) + np.spacing(np.abs(v).astype(np.float32)), 0.0)
    return r, np.maximum(np.abs(bf16(v + e) - r), np.abs(bf16(v - e) - r))


def product(a, ea, b, eb, L, bias=0.0):
    """bound of bf16(a) @ bf16(b) (+ bias) computed on device from operands known to within ea, eb"""
    (ra, da), (rb, db) = rounded(a, ea), rounded(b, eb)
    moved = da @ np.abs(rb) + np.abs(ra) @ db + da @ db
    return moved + bound(np.abs(ra @ rb + bias) + moved, (np.abs(ra) + da) @ (np.abs(rb) + db) + np.abs(bias), L)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 33])
def test_sequential_forward_and_gradients(dev, B):
    import torch
    from coach_amd.nn import graph as G
    r = lambda t: torch.from_numpy(bf16(t.detach().numpy()))
    f = {"relu": torch.relu, "tanh": torch.tanh, None: lambda t: t}

    class Product(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w):
            ctx.save_for_backward(x, w)
            return r(x) @ r(w)

        @staticmethod
        def backward(ctx, g):
            x, w = ctx.saved_tensors
            return r(g) @ r(w).T, r(x).T @ r(g)
    params = G.FlatParams()
    seq = G.Sequential([G.Dense(params, "l%d" % i, DIMS[i], DIMS[i + 1], ACTS[i], precision="bf16") for i in range(3)])
    params.finalize(dev)
    rng = np.random.RandomState(B)
    seq.initialize(rng)
    for l in seq.layers:
        params.w(l.bname).copy_(dev_tensor(rng.randn(l.N).astype(np.float32), dev))
    x, dq = rng.randn(B, 4).astype(np.float32), rng.randn(B, 3).astype(np.float32)
    ctx = G.Context(dev)
    acts = seq.forward(ctx, G.input_tensor(dev_tensor(x, dev), B, 4))
    acts[-1].ensure_grad().copy_(dev_tensor(dq, dev).view(1, B, 3))
    seq.backward(ctx, acts)
    W = [params.w(l.kname).cpu().double().requires_grad_() for l in seq.layers]
    b = [params.w(l.bname).cpu().double().requires_grad_() for l in seq.layers]
    h, zs = torch.from_numpy(x).double(), []
    for i, a in enumerate(ACTS):
        zs.append(Product.apply(h, W[i]) + b[i])
        zs[-1].retain_grad()
        h = f[a](zs[-1])
    (h * torch.from_numpy(dq).double()).sum().backward()
    n = lambda t: t.detach().numpy()
    close = lambda got, ref, tol, what: (np.abs(got.cpu().numpy().reshape(ref.shape) - ref) <= tol).all() or pytest.fail(what)
    ys, ey, ez = [x.astype(np.float64)], [np.zeros(x.shape)], []         # forward: every layer's output and its bound
    for i, a in enumerate(ACTS):
        ez.append(product(ys[-1], ey[-1], n(W[i]), 0.0, DIMS[i] + 1, n(b[i])))
        ys.append(n(f[a](zs[i])))
        ey.append(ez[-1] + (2.0 ** -22 * np.abs(ys[-1]) if a == "tanh" else 0.0))
        close(acts[i + 1].data, ys[-1], ey[-1], "forward, layer %d" % i)
    dy, edy = dq.astype(np.float64), np.zeros(dq.shape)                  # backward: dz = dy * act'(y), then the products
    for i in (2, 1, 0):
        dz, y, e = n(zs[i].grad), ys[i + 1], ey[i + 1]
        if ACTS[i] == "relu":
            edz = edy + np.where(np.abs(n(zs[i])) <= ez[i], np.abs(dy) + edy, 0.0)
        elif ACTS[i] == "tanh":       # 1 - y * y and the product: three fp32 roundings
            moved = 2 * np.abs(y) * e + e ** 2
            edz = edy * (np.abs(1 - y * y) + moved) + np.abs(dy) * moved + 4 * U * (np.abs(dy) + edy)
        else:
            edz = edy
        close(acts[i + 1].grad, dz, edz, "dz, layer %d" % i)
        close(params.g(seq.layers[i].kname), n(W[i].grad), product(ys[i].T, ey[i].T, dz, edz, B), "dW, layer %d" % i)
        close(params.g(seq.layers[i].bname), n(b[i].grad),
              edz.sum(0) + bound(np.abs(dz).sum(0) + edz.sum(0), (np.abs(dz) + edz).sum(0), B), "db, layer %d" % i)
        dy, edy = bf16(dz) @ bf16(n(W[i])).T, product(dz, edz, n(W[i]).T, 0.0, DIMS[i + 1])


@pytest.mark.gpu
def test_dqn_net_graph_replays_agree_and_fp32_is_untouched(dev):
    import torch
    from coach_amd.agents.vector_agent import capture
    from coach_amd.nn.networks import DQNNet
    rng = np.random.RandomState(7)
    batch = [dev_tensor(v, dev) for v in (rng.randn(33, 4).astype(np.float32), rng.randn(33, 4).astype(np.float32),
                                          rng.randint(0, 2, 33).astype(np.int32), rng.randn(33).astype(np.float32),
                                          np.zeros(33, np.float32))]

    def update(net):
        net.learn_from_batch(batch[0], batch[1], 33, batch[2], batch[3], batch[4], 0.99)
        torch.cuda.synchronize()
        return net.params.weights.clone()
    before = update(DQNNet(dev, (4,), 2, seed=3))                        # fp32, before any bf16 network exists
    net = DQNNet(dev, (4,), 2, seed=3, precision="bf16")
    assert net._fused is None and net._act is None and all(l.precision == "bf16" for l in net.torso.layers + [net.q_head])
    live = (net.params.both, net.adam.m, net.adam.v, net.adam.state)
    state = [t.clone() for t in live]
    restore = lambda: [t.copy_(s) for t, s in zip(live, state)]
    eager = update(net)
    assert not torch.equal(eager, before), "the bf16 network computed the fp32 network's bits"
    restore()
    graph = capture(lambda: net.learn_from_batch(batch[0], batch[1], 33, batch[2], batch[3], batch[4], 0.99))
    for _ in range(2):
        restore()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(net.params.weights, eager)
    assert torch.equal(update(DQNNet(dev, (4,), 2, seed=3)), before)     # fp32 alongside: the same bits


def test_default_is_fp32_and_the_entries_are_bound():
    from coach_amd import _rlx
    from coach_amd.agents.dqn_agent import DQNAgentParameters
    from coach_amd.base_parameters import NetworkParameters
    from coach_amd.presets import CartPole_DQN_bf16
    assert NetworkParameters.precision == "fp32" and DQNAgentParameters().network_wrappers["main"].precision == "fp32"
    assert CartPole_DQN_bf16.graph_manager.agent_params.network_wrappers["main"].precision == "bf16"
    for name in ("forward", "input_grad", "weight_grad"):
        assert callable(getattr(_rlx.lib(), "rlx_dense_bf16_" + name))


@pytest.mark.parametrize("case,message", [("image", "not for image observations"), ("noise", "not for the ParameterNoise"),
                                          ("dist", "not for data-parallel training"), ("agent", "not for PALAgent"),
                                          ("dueling", "not for the dueling head"),
                                          ("network", "DQNNetworkParameters"), ("fp16", "precision must be one of")])
def test_refusals(case, message):
    from coach_amd.agents import dqn_agent, pal_agent
    from coach_amd.architectures.head_parameters import DuelingQHeadParameters
    from coach_amd.exploration_policies.parameter_noise import ParameterNoiseParameters
    from coach_amd.nn.networks import common_net_kwargs
    ap = dqn_agent.DQNAgentParameters()
    net = ap.network_wrappers["main"]
    net.precision = "fp16" if case == "fp16" else "bf16"
    if case == "noise":
        ap.exploration = ParameterNoiseParameters(ap)
    if case == "dueling":
        net.heads_parameters = [DuelingQHeadParameters()]
    env = types.SimpleNamespace(p=types.SimpleNamespace(kind="image" if case == "image" else "vector"))
    with pytest.raises(ValueError, match=message):
        if case == "network":                 # a network class without bf16 layers: what every *_net_kwargs starts from
            common_net_kwargs(net, 0)
        else:
            agent = pal_agent.PALAgent if case == "agent" else dqn_agent.DQNAgent
            agent(ap, env, dist=types.SimpleNamespace(enabled=case == "dist"))
