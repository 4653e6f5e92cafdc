"""numpy twin of the factorised NoisyNet dense layer (coach_amd/nn/graph.py NoisyDense, csrc/noisy_dense.hip,
rlx_noisy_sample in csrc/noise.hip): the noise vectors from tests/noise_ref.py's generator, f, the layer's forward and
backward formulas in fp64, the initialiser.  Restates rl_coach/architectures/tensorflow_components/layers.py:220-257."""
import numpy as np

import noise_ref

SIGMA0 = 0.5
NOISY_PASSES = 4
PASS = {"act": 0, "online": 1, "target": 2, "online_next": 3}
FIRST_STREAM = 5                 # streams 0..4 belong to rlx_normal_fill's users


def f(v):
    """sign(v) sqrt(|v|), fp64 (sqrt is correctly rounded: bit-identical to the device)."""
    v = np.asarray(v, dtype=np.float64)
    return np.sign(v) * np.sqrt(np.abs(v))


def noise(seed, rank, layer, noise_pass, counter, K, N):
    """-> (f_in [K], f_out [N], f_b [N]) in fp64, before the cast to fp32: the draw of (seed, rank, layer, pass, counter)."""
    stream0 = FIRST_STREAM + 3 * (NOISY_PASSES * layer + noise_pass)
    z = noise_ref.normal_fill([counter], stream0, 3, max(K, N), seed, rank)[0]
    return f(z[0, :K]), f(z[1, :N]), f(z[2, :N])


def noise_f32(seed, rank, layer, noise_pass, counter, K, N):
    """what the layer computes with: each vector rounded once to fp32."""
    return tuple(v.astype(np.float32) for v in noise(seed, rank, layer, noise_pass, counter, K, N))


def act(z, kind):
    if kind == "relu":
        return np.maximum(z, 0.0)
    if kind == "tanh":
        return np.tanh(z)
    return z


def act_deriv(y, kind):
    """the activation's derivative through its OUTPUT y"""
    if kind == "relu":
        return (y > 0).astype(np.float64)
    if kind == "tanh":
        return 1.0 - y * y
    return np.ones_like(y)


def forward(x, wm, ws, bm, bs, f_in, f_out, f_b, activation=None):
    """y = act(x W + b), W = wm + ws * (f_in outer f_out), b = bm + bs * f_b, all in fp64."""
    x, wm, ws, bm, bs, f_in, f_out, f_b = (np.asarray(a, dtype=np.float64) for a in (x, wm, ws, bm, bs, f_in, f_out, f_b))
    W = wm + ws * np.outer(f_in, f_out)
    b = bm + bs * f_b
    return act(x @ W + b, activation)


def backward(x, wm, ws, dz, f_in, f_out, f_b, lower_activation=None):
    """dz = dL/d(pre-activation) -> dict(dwm, dws, dbm, dbs, dx): the factorised formulas of the device layer.  dx carries
    the lower layer's activation derivative act'(x) (x is that layer's output)."""
    x, wm, ws, dz, f_in, f_out, f_b = (np.asarray(a, dtype=np.float64) for a in (x, wm, ws, dz, f_in, f_out, f_b))
    dwm = x.T @ dz
    dws = dwm * f_in[:, None] * f_out[None, :]
    dbm = dz.sum(axis=0)
    dbs = dbm * f_b
    dx = dz @ wm.T + ((dz * f_out[None, :]) @ ws.T) * f_in[None, :]
    dx = dx * act_deriv(x, lower_activation)
    return dict(dwm=dwm, dws=dws, dbm=dbm, dbs=dbs, dx=dx)


def initialize(rng, K, N, sigma0=SIGMA0):
    """layers.py:233-242 (default branch): -> (weight_mean, bias_mean, weight_stddev, bias_stddev) fp32, drawn from rng
    in the order weight_mean, weight_stddev, bias_stddev."""
    lim = 1.0 / np.sqrt(K)
    wm = rng.uniform(-lim, lim, size=(K, N)).astype(np.float32)
    ws = rng.uniform(-sigma0 * lim, sigma0 * lim, size=(K, N)).astype(np.float32)
    bs = rng.uniform(-sigma0 * lim, sigma0 * lim, size=(N,)).astype(np.float32)
    return wm, np.zeros(N, dtype=np.float32), ws, bs
