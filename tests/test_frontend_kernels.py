"""The kernels between an emulator frame and a stored observation / reward, each called directly and compared with a
plain numpy / oracle.filters reference: rlx_max_over_frames_u8, rlx_resize_bilinear_u8, rlx_rgb_to_y_u8,
rlx_running_stats_merge / _push / _normalize, rlx_reward_filter and the same filter inside rlx_rollout_observe_step.

Every result is bytes, or fp64 values computed in the reference's operation order (rounded once to fp32 where the entry
point returns fp32): every comparison is bit-exact, sign of zero included, NaN where the reference is NaN.  Outputs
live in a buffer with 64 guard bytes on both sides of the region the kernel may write; the guards must be intact.

The NaN rule (include/rlx.h): Python's min / max, np.clip and np.maximum keep a NaN where HIP's fmin / fmax would
return the other operand, so a NaN reward is stored as NaN and not as a clipping bound."""
import numpy as np
import pytest

from oracle import filters as F
from tests.util import dev_tensor

GUARD, FILL = 64, 0xA5
EPS = 1e-2


class Guarded(object):
    """`nbytes` device bytes to write into (viewed as `dtype`), 64 guard bytes before and after, 16-byte aligned plus
    `offset`."""

    def __init__(self, nbytes, dev, dtype=None, offset=0, init=None):
        import torch
        self.whole = torch.full((GUARD + offset + nbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.lo, self.hi = GUARD + offset, GUARD + offset + nbytes
        raw = self.whole[self.lo:self.hi]
        assert (raw.data_ptr() - offset) % 16 == 0
        self.t = raw if dtype is None else raw.view(dtype)
        if init is not None:
            self.t.copy_(dev_tensor(init, dev).view(self.t.dtype).reshape(self.t.shape))

    def numpy(self):
        return self.t.cpu().numpy()

    def check_guards(self):
        w = self.whole.cpu().numpy()
        assert (w[:self.lo] == FILL).all(), "bytes before the output were written"
        assert (w[self.hi:] == FILL).all(), "bytes after the output were written"


def same_bits(got, want):
    """bit-identical (so -0.0 is not 0.0); where the reference is NaN the result must be a NaN, of any payload"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return np.array_equal(got.view(u)[~nan], want.view(u)[~nan])


# ---------------------------------------------------------------------------------------------- max over frames

@pytest.mark.gpu
@pytest.mark.parametrize("n_env,K,frame_bytes", [(1, 1, 16), (1, 2, 16), (3, 2, 48), (5, 3, 192), (2, 4, 16 * 257),
                                                 (1, 2, 16 * (64 * 256 + 3))])
def test_max_over_frames_equals_numpy_max(rlx, dev, n_env, K, frame_bytes):
    """16 * 257: a second, partly filled 256-thread block.  16 * (64 * 256 + 3): the launch caps the grid at 64 blocks,
    so the stride loop makes a second pass."""
    rng = np.random.RandomState(n_env * 100 + K)
    frames = rng.randint(0, 256, size=(n_env, K, frame_bytes)).astype(np.uint8)
    # the maximum in each of the K positions: byte k of every env has it in frame k
    frames[:, :, :K] = rng.randint(0, 100, size=(n_env, K, K))
    for k in range(K):
        frames[:, k, k] = 200 + k
    # 0x00 / 0xFF / 0x7F / 0x80 in neighbouring byte lanes of one word, against their opposites in the last frame: a
    # signed compare takes 0x7F for more than 0x80, a carry between the lanes of the packed maximum spoils a neighbour
    frames[0, :, 8:16] = 1
    frames[0, 0, 8:16] = [0x00, 0xFF, 0x7F, 0x80, 0x80, 0x7F, 0xFF, 0x00]
    if K > 1:
        frames[0, K - 1, 8:16] = [0xFF, 0x00, 0x80, 0x7F, 0x7F, 0x80, 0x00, 0xFF]
    want = np.max(frames, axis=1)
    if K > 1:
        assert want[0, 8:16].tolist() == [0xFF, 0xFF, 0x80, 0x80, 0x80, 0x80, 0xFF, 0xFF]
    out = Guarded(n_env * frame_bytes, dev)
    rlx.max_over_frames_u8(dev_tensor(frames, dev), out.t, n_env, K, frame_bytes, 0)
    assert np.array_equal(out.numpy().reshape(n_env, frame_bytes), want)
    out.check_guards()


@pytest.mark.gpu
def test_max_over_frames_refusals(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    src = torch.zeros(256, dtype=torch.uint8, device=dev)
    out = Guarded(64, dev)
    with pytest.raises(RlxError, match="multiples of 16 bytes"):
        rlx.max_over_frames_u8(src, out.t, 1, 2, 24, 0)
    with pytest.raises(RlxError, match="16-byte aligned"):
        rlx.max_over_frames_u8(src[4:], out.t, 1, 2, 16, 0)
    with pytest.raises(RlxError, match="16-byte aligned"):
        rlx.max_over_frames_u8(src, Guarded(64, dev, offset=4).t, 1, 2, 16, 0)
    with pytest.raises(RlxError):
        rlx.max_over_frames_u8(src, out.t, 1, 0, 16, 0)
    out.check_guards()


# ---------------------------------------------------------------------------------------------- rescale

RESIZE_SHAPES = [(1, 1, 1, 1, 1, 1), (2, 1, 1, 1, 3, 2), (1, 2, 2, 3, 7, 5), (3, 5, 7, 4, 5, 7), (1, 2, 3, 1, 84, 84),
                 (2, 1, 16, 3, 4, 4), (2, 33, 47, 2, 61, 29), (1, 9, 1, 1, 4, 3), (26, 20, 30, 3, 84, 84)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,H,W,C,OH,OW", RESIZE_SHAPES)
def test_resize_equals_the_oracle(rlx, dev, n, H, W, C, OH, OW):
    """(2, 2) -> (7, 5): the mirror at both edges.  (5, 7) -> (5, 7): the identity.  26 x 84 x 84 x 3 = 550 368 outputs,
    more than 2048 blocks x 256: the stride loop's second pass."""
    rng = np.random.RandomState(H * 7 + W + n)
    img = rng.randint(0, 256, size=(n, H, W, C)).astype(np.uint8)
    want = np.stack([F.resize_bilinear_u8(img[i], (OH, OW)) for i in range(n)])
    assert want.shape == (n, OH, OW, C)
    if (H, W) == (OH, OW):
        assert np.array_equal(want, img)
    out = Guarded(want.size, dev)
    rlx.resize_bilinear_u8(dev_tensor(img, dev), out.t, n, H, W, C, OH, OW, 0)
    assert np.array_equal(out.numpy().reshape(want.shape), want)
    out.check_guards()


# ---------------------------------------------------------------------------------------------- luminance -> uint8

def _exhaustive_rgb():
    r, g, b = np.meshgrid(np.arange(256), np.arange(256), np.arange(0, 256, 17), indexing="ij")
    grid = np.stack([r.ravel(), g.ravel(), b.ravel()], axis=1)
    grey = np.repeat(np.arange(256)[:, None], 3, axis=1)
    return np.concatenate([grid, grey]).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("n_pixels", [1, 2, 3, 4, 5, 7, 8, 1023, 4 * 2048 * 256 + 5, "grid"])
def test_rgb_to_y_equals_the_oracle(rlx, dev, n_pixels):
    """4 * 2048 * 256 + 5 pixels: the first size at which the grouped loop strides (6 MB in).  "grid": all 256 x 256
    (r, g) x b in range(0, 256, 17), and all 256 greys.  With the bounds (-100, 400) every value lies in [51, 181.04]:
    no out-of-range cast.  The grouped path stores whole words: the bytes right after out[n_pixels] must be untouched."""
    if n_pixels == "grid":
        rgb = _exhaustive_rgb()
    else:
        rgb = np.random.RandomState(n_pixels % 1000).randint(0, 256, size=(n_pixels, 3)).astype(np.uint8)
    src = dev_tensor(rgb, dev)
    for lo, hi in ((0.0, 255.0), (-100.0, 400.0)):
        want = F.to_uint8(F.rgb_to_y(rgb), lo, hi)
        out = Guarded(len(rgb), dev)
        rlx.rgb_to_y_u8(src, out.t, len(rgb), lo, hi, 0)
        assert np.array_equal(out.numpy(), want), (lo, hi)
        out.check_guards()


@pytest.mark.gpu
def test_rgb_to_y_refusals(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    src = torch.zeros(64, dtype=torch.uint8, device=dev)
    out = Guarded(16, dev)
    with pytest.raises(RlxError, match="4-byte aligned"):
        rlx.rgb_to_y_u8(src[1:], out.t, 8, 0.0, 255.0, 0)
    with pytest.raises(RlxError, match="4-byte aligned"):
        rlx.rgb_to_y_u8(src, Guarded(16, dev, offset=2).t, 8, 0.0, 255.0, 0)
    for lo, hi in ((255.0, 255.0), (255.0, 0.0)):
        with pytest.raises(RlxError, match="high values can be less or equal to the input observation space low"):
            rlx.rgb_to_y_u8(src, out.t, 8, lo, hi, 0)
    out.check_guards()


# ---------------------------------------------------------------------------------------------- running statistics

class DeviceStats(object):
    """the five arrays of the running statistics in the reference's initial state (shared_running_stats.py:118-128)"""
    NAMES = ("sum", "sumsq", "count", "mean", "std")

    def __init__(self, dim, dev):
        import torch
        f64 = torch.float64
        self.dim = dim
        self.sum = Guarded(8 * dim, dev, f64, init=np.zeros(dim))
        self.sumsq = Guarded(8 * dim, dev, f64, init=EPS * np.ones(dim))
        self.count = Guarded(8, dev, f64, init=np.array([EPS]))
        self.mean = Guarded(8 * dim, dev, f64, init=np.zeros(dim))
        self.std = Guarded(8 * dim, dev, f64, init=np.sqrt(EPS) * np.ones(dim))

    def args(self):
        return self.sum.t, self.sumsq.t, self.count.t, self.mean.t, self.std.t

    def state(self):
        return [getattr(self, k).numpy() for k in self.NAMES]

    def check_against(self, o, what):
        want = [o._sum, o._sum_squares, np.array([o._count]), o._mean, o._std]
        for k, g, w in zip(self.NAMES, self.state(), want):
            assert same_bits(g, np.asarray(w, np.float64)), (what, k, g, w)
            getattr(self, k).check_guards()


def _delta(batch):
    batch = np.asarray(batch, np.float64)
    return np.concatenate([batch.sum(0), np.square(batch).sum(0), [float(len(batch))]])


def _batches(dim):
    rng = np.random.RandomState(dim)
    sizes = (1, 37, 0, 12)          # one sample first: count - 1 < 1.  A delta of count 0: totals unchanged
    batches = [rng.randn(n, dim) * 3 + 1 for n in sizes]
    if dim > 1:
        for b in batches:
            b[:, 0] = 2.5           # a constant column: the variance floor, std == sqrt(epsilon)
    return batches


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 17, 256, 257, 1000])
def test_running_stats_merge_equals_the_oracle(rlx, dev, dim):
    """257 and 1000 make the single workgroup's 256 threads loop."""
    o = F.RunningStatsOracle((dim,), epsilon=EPS)
    st = DeviceStats(dim, dev)
    st.check_against(o, "initial")
    for k, b in enumerate(_batches(dim)):
        before = [o._sum.copy(), o._sum_squares.copy(), o._count]
        o.push(b)
        if len(b) == 0:
            assert np.array_equal(before[0], o._sum) and np.array_equal(before[1], o._sum_squares) and before[2] == o._count
        rlx.running_stats_merge(dev_tensor(_delta(b), dev), dim, *st.args(), EPS, 0)
        st.check_against(o, "delta %d" % k)
    assert dim == 1 or o._std[0] == np.sqrt(EPS)
    if dim in (17, 257):            # the same batches through the push kernel: the same state
        pushed = DeviceStats(dim, dev)
        for b in _batches(dim):
            if len(b):
                rlx.running_stats_push(dev_tensor(b, dev), 1, len(b), dim, *pushed.args(), EPS, 0)
        pushed.check_against(o, "pushed")


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("n,dim", [(1, 1), (1000, 1), (1, 17), (59, 17)])
def test_running_stats_normalize_equals_the_oracle(rlx, dev, n, dim, f64):
    """fp64 and fp32 input; out32 only, out64 only, both; values that clip on both sides; a column with std = 0 (the
    division is by 1e-15: 0 where x equals the mean, a clip bound elsewhere); +-inf."""
    import torch
    rng = np.random.RandomState(n + dim)
    o = F.RunningStatsOracle((dim,), epsilon=EPS)
    o.push(rng.randn(50, dim) * 2 + 1)
    o._std[dim - 1] = 0.0
    o._mean[dim - 1] = np.float32(o._mean[dim - 1])                 # so that an fp32 input can equal it
    x = (rng.randn(n, dim) * 8 + 1).astype(np.float64 if f64 else np.float32)
    x[0, dim - 1] = o._mean[dim - 1]
    if n > 4:
        x[1, 0], x[2, 0], x[3, dim - 1], x[4, dim - 1] = np.inf, -np.inf, np.inf, -np.inf
        x[5, 0], x[6, 0] = -0.0, 1e300 if f64 else 3e38
    with np.errstate(over="ignore"):
        want = o.normalize(x)
    assert want.dtype == np.float64
    if n > 4:
        assert (want == 5.0).any() and (want == -5.0).any() and (np.abs(want) < 5.0).any()
    mean, std, src = dev_tensor(o._mean, dev), dev_tensor(o._std, dev), dev_tensor(x, dev)
    for use32, use64 in ((True, False), (False, True), (True, True)):
        o32, o64 = Guarded(4 * n * dim, dev, torch.float32), Guarded(8 * n * dim, dev, torch.float64)
        rlx.running_stats_normalize(src, int(f64), n, dim, mean, std, -5.0, 5.0, o32.t if use32 else None,
                                    o64.t if use64 else None, 0)
        if use32:
            assert same_bits(o32.numpy().reshape(n, dim), want.astype(np.float32))
        else:
            assert (o32.whole.cpu().numpy() == FILL).all()
        if use64:
            assert same_bits(o64.numpy().reshape(n, dim), want)
        else:
            assert (o64.whole.cpu().numpy() == FILL).all()
        o32.check_guards(); o64.check_guards()


# ---------------------------------------------------------------------------------------------- NaN and special values

SPECIAL_REWARDS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, 3.4e38, -3.4e38, 0.3], np.float32)
CLIPS = [None, (-1.0, 1.0), (0.0, 1.0), (-1.0, 0.0)]


def _filtered(rewards, factor, clip):
    with np.errstate(over="ignore"):
        return np.array([np.float32(F.reward_rescale(r, factor) if clip is None else
                                    F.reward_clip(F.reward_rescale(r, factor), clip[0], clip[1])) for r in rewards],
                        np.float32)


def test_the_oracle_keeps_a_nan_reward():
    for clip in CLIPS[1:]:
        assert np.isnan(F.reward_clip(float("nan"), *clip))
    assert np.isnan(_filtered(SPECIAL_REWARDS, 1.0, (-1.0, 1.0))[0])


@pytest.mark.gpu
@pytest.mark.parametrize("factor", [1.0, -2.0, 10.0])
@pytest.mark.parametrize("clip", CLIPS, ids=["noclip", "clip-1+1", "clip0+1", "clip-1+0"])
def test_reward_filter_nan_and_special_values(rlx, dev, clip, factor):
    import torch
    want = _filtered(SPECIAL_REWARDS, factor, clip)
    assert np.isnan(want[0])
    out = Guarded(4 * len(want), dev, torch.float32)
    lo, hi = clip or (0.0, 0.0)
    rlx.reward_filter(dev_tensor(SPECIAL_REWARDS, dev), out.t, len(want), factor, int(clip is not None), lo, hi, 0)
    assert same_bits(out.numpy(), want), (out.numpy(), want)
    out.check_guards()


@pytest.mark.gpu
@pytest.mark.parametrize("clip", CLIPS[1:], ids=["clip-1+1", "clip0+1", "clip-1+0"])
def test_rollout_observe_step_stores_a_nan_reward_as_nan(rlx, dev, clip):
    import torch
    n_env, rows, row0 = 3, 8, 3
    reward = np.array([np.nan, 0.5, -3.0], np.float32)
    want = _filtered(reward, 1.0, clip)
    assert np.isnan(want[0])
    filtered = Guarded(4 * n_env, dev, torch.float32)
    mem_reward = Guarded(4 * rows, dev, torch.float32, init=np.full(rows, 7.0, np.float32))
    ep_return = torch.zeros(n_env, dtype=torch.float64, device=dev)
    ep_len = torch.zeros(n_env, dtype=torch.int32, device=dev)
    acc = torch.zeros(8, dtype=torch.float64, device=dev)
    rlx.episode_stats_init(ep_return, ep_len, n_env, acc, 0)
    game_over = torch.zeros(n_env, dtype=torch.uint8, device=dev)
    actions = dev_tensor(np.array([2, 0, 1], np.int32), dev)
    mem_action = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    mem_done = torch.full((rows,), 9, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rlx.rollout_observe_step(dev_tensor(reward, dev), filtered.t, 1.0, 1, clip[0], clip[1], game_over, ep_return, ep_len,
                             acc, None, None, actions, 4, mem_action, mem_reward.t, mem_done, row0, rows, n_env, status, 0)
    assert status.item() == 0
    assert same_bits(filtered.numpy(), want), (filtered.numpy(), want)
    stored = np.full(rows, 7.0, np.float32)
    stored[row0:row0 + n_env] = want
    assert same_bits(mem_reward.numpy(), stored), (mem_reward.numpy(), stored)
    assert mem_action.cpu().numpy().tolist() == [-1, -1, -1, 2, 0, 1, -1, -1]
    assert mem_done.cpu().numpy().tolist() == [9, 9, 9, 0, 0, 0, 9, 9]
    filtered.check_guards(); mem_reward.check_guards()


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [True, False])
def test_running_stats_normalize_keeps_a_nan(rlx, dev, f64):
    import torch
    n, dim = 4, 3
    o = F.RunningStatsOracle((dim,), epsilon=EPS)
    o.push(np.random.RandomState(0).randn(20, dim))
    x = np.arange(n * dim, dtype=np.float64 if f64 else np.float32).reshape(n, dim) - 5
    x[1, 2] = x[3, 0] = np.nan
    want = o.normalize(x)
    assert np.isnan(want).sum() == 2
    o32, o64 = Guarded(4 * n * dim, dev, torch.float32), Guarded(8 * n * dim, dev, torch.float64)
    rlx.running_stats_normalize(dev_tensor(x, dev), int(f64), n, dim, dev_tensor(o._mean, dev), dev_tensor(o._std, dev),
                                -5.0, 5.0, o32.t, o64.t, 0)
    assert same_bits(o64.numpy().reshape(n, dim), want), (o64.numpy(), want)
    assert same_bits(o32.numpy().reshape(n, dim), want.astype(np.float32))
    o32.check_guards(); o64.check_guards()


@pytest.mark.gpu
@pytest.mark.parametrize("through", ["push", "merge"])
def test_running_stats_nan_sample_makes_its_column_nan_only(rlx, dev, through):
    dim = 4
    rng = np.random.RandomState(3)
    first, batch = rng.randn(6, dim), rng.randn(5, dim)
    batch[2, 1] = np.nan
    o = F.RunningStatsOracle((dim,), epsilon=EPS)
    st = DeviceStats(dim, dev)
    for b in (first, batch):
        with np.errstate(invalid="ignore"):
            o.push(b)
        if through == "push":
            rlx.running_stats_push(dev_tensor(b, dev), 1, len(b), dim, *st.args(), EPS, 0)
        else:
            rlx.running_stats_merge(dev_tensor(_delta(b), dev), dim, *st.args(), EPS, 0)
    assert np.isnan(o._mean).tolist() == np.isnan(o._std).tolist() == [False, True, False, False]
    st.check_against(o, through)
