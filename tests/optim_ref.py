"""What the optimiser tests hold csrc/optim.hip and csrc/adam_block_body.hpp to.

The UPDATE needs no restatement of its own: oracle.optim.AdamTF1 and oracle.optim.mix_weights state the kernels' expression
operation by operation in numpy fp32, and optim.hip is built without contraction and without fast-math, so both sides do
the same correctly rounded adds, multiplies, divides and square roots (step_reference below only strings them together).

The gradient NORM is a sum, and a sum has an order.  norm_f32 restates the order the Adam launches use, from the comments
in adam_block_body.hpp (block_step) and optim.hip (adam_step_kernel, adam_norm_finish, adam_finish_norm_kernel):

  1. thread `tid` of block `b` of `blocks` adds g^2 (an fp32 product, rounded, then an fp32 add) onto 0.0f, in this order:
     the four elements of float4 number  b * 256 + tid + it * blocks * 256  for it = 0, 1, ... while that float4 exists,
     then -- threads 0 .. (n & 3) - 1 of block 0 only -- the one element  4 * (n >> 2) + tid  behind the last float4;
  2. the 256 sums of a block meet in a halving tree: red[t] += red[t + d] for d = 128, 64, ... 1;
  3. thread `tid` of the finishing workgroup adds the block sums tid, tid + 256, ... in index order onto 0.0f;
  4. the same tree again, then one fp32 square root.

  adam_blocks(n, workspace_floats)   -> the number of blocks a norm launch uses (grid_for(n / 4 + 1, 256, 1024), clamped)
  register_held(n, blocks)           -> whether rlx_adam_tf1_step keeps the step in registers (rlx_adam_step_blocks != 0)
  norm_f32(g, blocks)                -> (norm as np.float32, the per-block partial sums as fp32)
  norm_depth(n, blocks)              -> D: the largest number of additions a term of the sum passes through
  norm_bound(n, blocks)              -> the relative error norm_f32 (or any evaluation in that order) may have
  step_reference(opt, w, g, ...)     -> one oracle step in place, and the target mixed towards the stepped weights"""
import numpy as np

from oracle.optim import mix_weights

F32 = np.float32
F64 = np.float64
U24 = 2.0 ** -24
BLOCK, NORM_IT, MAX_BLOCKS = 256, 4, 1024


def adam_blocks(n, workspace_floats=None):
    blocks = min(max((n // 4 + 1 + BLOCK - 1) // BLOCK, 1), MAX_BLOCKS)
    return blocks if workspace_floats is None else min(blocks, workspace_floats)


def register_held(n, blocks):
    return blocks >= 1 and (n >> 2) <= blocks * BLOCK * NORM_IT


def _tree(red):
    """red: (rows, 256) fp32 -> (rows,) by the halving tree"""
    red = red.copy()
    d = BLOCK // 2
    while d > 0:
        red[:, :d] = red[:, :d] + red[:, d:2 * d]
        d //= 2
    return red[:, 0]


def norm_f32(g, blocks):
    g = np.ascontiguousarray(g, dtype=F32)
    n = g.size
    n4, stride = n >> 2, blocks * BLOCK
    its = max(1, -(-n4 // stride))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        sq = np.zeros(its * stride * 4, dtype=F32)       # (adding a square of +0.0 where no float4 exists changes no bit:
        sq[:4 * n4] = g[:4 * n4] * g[:4 * n4]            #  a sum of squares is never -0.0)
        sq = sq.reshape(its, blocks, BLOCK, 4)
        ss = np.zeros((blocks, BLOCK), dtype=F32)
        for it in range(its):
            for k in range(4):
                ss = ss + sq[it, :, :, k]
        tail = g[4 * n4:]
        ss[0, :tail.size] = ss[0, :tail.size] + tail * tail
        part = _tree(ss)
        rows = -(-blocks // BLOCK)
        padded = np.zeros(rows * BLOCK, dtype=F32)
        padded[:blocks] = part
        s = np.zeros(BLOCK, dtype=F32)
        for r in range(rows):
            s = s + padded.reshape(rows, BLOCK)[r]
        total = _tree(s[None, :])[0]
        return np.sqrt(total), part


def norm_depth(n, blocks):
    """additions on the longest path: a thread's own run (four per float4 it holds, one more for a tail element: thread 0 of
    block 0 has the most float4s and the first tail element), 8 tree levels, the finishing thread's run, 8 tree levels."""
    n4, stride = n >> 2, blocks * BLOCK
    own = 4 * -(-n4 // stride) + (1 if n & 3 else 0)
    return own + 8 + -(-blocks // BLOCK) + 8


def norm_bound(n, blocks):
    """every term is a rounded product that then passes through at most D rounded additions of non-negative numbers: the
    sum is within gamma_{D+1} = (D+1) u / (1 - (D+1) u) of exact, relatively (u = 2^-24).  The square root halves a
    relative error (sqrt(1 + e) <= 1 + e / 2) and rounds once more."""
    k = norm_depth(n, blocks) + 1
    gamma = k * U24 / (1.0 - k * U24)
    return (1.0 + gamma / 2.0) * (1.0 + U24) - 1.0


def norm_f64(g):
    g = np.asarray(g, dtype=F32).astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt(np.sum(g * g))


def step_reference(opt, w, g, grad_scale, target=None, rate=None):
    """opt: oracle.optim.AdamTF1.  Steps w (and opt's m, v, beta powers) in place; mixes `target` towards the NEW w."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        opt.step(w, g, grad_scale)
        if target is not None:
            target[...] = mix_weights(target, w, rate)
    return w

