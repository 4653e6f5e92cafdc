// Conditional Imitation Learning (rl_coach/agents/cil_agent.py, heads/cil_head.py): K command-selected copies of a
// three-layer regression head over the middleware's output, with dropout behind the hidden activations while training.
//   y_k = act(act(x W1_k + b1_k) W2_k + b2_k) W3_k + b3_k
//
// Work split (all three kernels): one workgroup of 4 waves per (branch, tile of 16 rows = the M of
// v_mfma_f32_16x16x4_f32).  The tile goes through every layer inside its workgroup; x [16][F + 4] and the hidden
// activations [16][H + 4] live in LDS and are the A operands of the next product.  No synchronisation between workgroups,
// no atomics on sums: two launches give the same bits.
//
// cil_branches_kernel (forward and train).  A wave owns 64 output columns of a hidden layer.  Lane (k = lane / 16,
// n = lane % 16) loads, for each of the four reduction rows 16 s + 4 k + j, the 16 bytes W[row][c0 + 4 n .. c0 + 4 n + 3];
// component q of that load is the B operand of accumulator q, so the lane ends up with the four ADJACENT columns
// c0 + 4 n + q of rows 4 k + r: the bias add, the activation, ONE Philox call for the dropout mask of those four
// columns and a 16-byte store to LDS (and to the saved activations) need no exchange between lanes.  Training keeps two
// accumulator sets from layer 2 on, the clean one (the reference's `predict`, which makes the targets) and the dropped
// one, both fed by the same weight registers: every weight tile is read once.  Layer 1's product is shared, the passes
// part at its dropout.  With both rates 0 the kernel is instantiated without the second set.  The output layer (A <= 16
// columns, rows of A floats: scalar loads, masked at A) is one 16 x 16 tile of wave 0, which also forms the targets, the
// loss terms and dy in its accumulator layout and leaves the tile's loss sum in the workspace.
//
// cil_loss_finish_kernel (one wave) adds the tiles' sums in tile, then branch order, and advances the draw index -- it
// runs behind the main launch, which is what makes it safe for every workgroup of that launch to read the index.
//
// cil_backward_kernel.  dy [16][16] -> dh2 = dy W3^T -> dz2 -> dh1 = dz2 W2^T -> dz1.  The transposed operands are read as
// ROWS of W (the reduction index is the contiguous one: lane (k, n) takes 16 bytes of row 16 t + n per four MFMAs), a
// wave owning the 16-column tiles t = wave, wave + 4, ..  Each product lands in LDS; an element-wise pass (a thread per
// four adjacent columns, again one Philox call) applies mask, scale and activation derivative in place and stores dz.
//
// cil_split_observation_kernel feeds the agent's two consumers from one stored observation: the embedder's columns and
// the row's command (the width-1 slice state_key_with_the_class_index names), element-wise.
#include "philox.hpp"
#include "rlx_device.hpp"

namespace {

using rlx::f32x4;

constexpr int kTile = 16, kWaves = 4, kThreads = 64 * kWaves;
constexpr uint32_t kNoiseTag = 0x4E4F4953u;      // noise.hip's counter word 3 tag: one generator, disjoint stream ids

struct Dropout {
    uint32_t thr1, thr2;           // keep iff word >= floor(rate * 2^32); 0 keeps everything
    float scale1, scale2;          // fp32 1 / (1 - rate)
    float keep1, keep2;            // fp32 1 - rate (the backward pass: a = h * keep)
    uint32_t seed, rank;
};

struct CilRun {
    const int *commands;
    float *y;                      // [K][B][A] clean prediction
    float *values;                 // forward: [B][ld_values]
    long long ld_values;
    const float *actions;          // train: [B][ld_actions]
    long long ld_actions;
    Dropout drop;
    const long long *draw;
    int huber;
    float loss_scale, dy_scale;    // loss_weight / B, grad_scale * loss_weight / B
    float *y_train, *dy, *h1, *h2;
    double *partials;              // [K][tiles]
    int *status;
};

// the four mask words of (branch, layer, row, columns 4 c4 .. 4 c4 + 3) at a draw index
__device__ __forceinline__ rlx::U4 mask_words(const Dropout &d, long long draw, int branch, int layer, int row, int c4) {
    return rlx::philox4x32_10((uint32_t)row * 64u + (uint32_t)c4, (uint32_t)(RLX_CIL_STREAM0 + 2 * branch + layer),
                              (uint32_t)draw, (uint32_t)((unsigned long long)draw >> 32) ^ kNoiseTag, d.seed, d.rank);
}

__device__ __forceinline__ f32x4 dropped(f32x4 v, const rlx::U4 &w, uint32_t thr, float scale) {
    return f32x4{w.x >= thr ? v[0] * scale : 0.f, w.y >= thr ? v[1] * scale : 0.f, w.z >= thr ? v[2] * scale : 0.f,
                 w.w >= thr ? v[3] * scale : 0.f};
}

// acc[s][q][r] += sum_k a[s][row 4 kk + r][k] * w[k][col + q]: one wave's 16 x 64 block for kSets A operands that share
// the weight loads (a[1] is unused where kSets = 1).  a[s]: LDS [16][lda]; w: [Kdim][N] row-major, col = the lane's first column (col_ok: inside N).
template <int kSets>
__device__ __forceinline__ void product64(const float *const (&a)[2], int lda, const float *w, int N, int Kdim,
                                          int col, bool col_ok, int kk, int nn, f32x4 (&acc)[kSets][4]) {
    for (int k0 = 0; k0 < Kdim; k0 += 16) {
        f32x4 av[kSets], b[4];
#pragma unroll
        for (int s = 0; s < kSets; ++s) av[s] = *reinterpret_cast<const f32x4 *>(a[s] + nn * lda + k0 + 4 * kk);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            b[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (col_ok) b[j] = *reinterpret_cast<const f32x4 *>(w + (long long)(k0 + 4 * kk + j) * N + col);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int s = 0; s < kSets; ++s)
                    acc[s][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s][j], b[j][q], acc[s][q], 0, 0, 0);
    }
}

// One hidden layer of the tile: in[s] -> out[s] (LDS), s = 0 clean, s = 1 the training pass (kSetsOut = 2: it exists
// behind this layer; kSetsIn = 1 with kSetsOut = 2: the passes part at this layer's dropout).  saved: the training pass's
// output rows in global memory ([B][N] of this branch) or null.
template <int kSetsIn, int kSetsOut>
__device__ __forceinline__ void hidden_layer(const float *const (&in)[2], int lda, const float *w, const float *bias,
                                             int Kdim, int N, int act, float *const (&out)[2], float *saved,
                                             const Dropout &dr, uint32_t thr, float scale, long long draw, int branch,
                                             int layer, int row0, int B) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kk = lane >> 4, nn = lane & 15, ldo = N + 4;
    for (int c0 = 64 * wave; c0 < N; c0 += 64 * kWaves) {
        const int col = c0 + 4 * nn;
        const bool col_ok = col < N;
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (col_ok) bv = *reinterpret_cast<const f32x4 *>(bias + col);
        f32x4 acc[kSetsIn][4];
#pragma unroll
        for (int s = 0; s < kSetsIn; ++s)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[s][q] = f32x4{bv[q], bv[q], bv[q], bv[q]};
        product64<kSetsIn>(in, lda, w, N, Kdim, col, col_ok, kk, nn, acc);
        if (!col_ok) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 4 * kk + r, row = row0 + m;
            f32x4 v[kSetsIn];
#pragma unroll
            for (int s = 0; s < kSetsIn; ++s)
#pragma unroll
                for (int q = 0; q < 4; ++q) v[s][q] = rlx::act_apply(acc[s][q][r], act);
            *reinterpret_cast<f32x4 *>(out[0] + m * ldo + col) = v[0];
            f32x4 t = v[kSetsIn - 1];
            if (kSetsOut == 2) {
                if (thr && row < B) t = dropped(t, mask_words(dr, draw, branch, layer, row, col >> 2), thr, scale);
                *reinterpret_cast<f32x4 *>(out[kSetsOut - 1] + m * ldo + col) = t;
            }
            if (saved && row < B) *reinterpret_cast<f32x4 *>(saved + (long long)row * N + col) = t;
        }
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {      // rlx::wave_sum's butterfly on doubles
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <bool kTrain, bool kDrop>
__global__ void __launch_bounds__(kThreads) cil_branches_kernel(const rlx_cil_desc d, const CilRun p) {
    extern __shared__ float lds[];
    constexpr int kSets = kDrop ? 2 : 1;
    const int k = blockIdx.y, row0 = blockIdx.x * kTile, tid = threadIdx.x;
    const int B = d.B, F = d.F, H1 = d.H1, H2 = d.H2, A = d.A;
    const int ldx = F + 4, ld1 = H1 + 4, ld2 = H2 + 4;
    float *xs = lds, *h1c = xs + kTile * ldx, *h2c = h1c + kTile * ld1;
    float *h1d = h2c + kTile * ld2, *h2d = h1d + kTile * ld1;              // kDrop only (the launch sizes the LDS)
    const long long draw = kDrop ? *p.draw : 0;

    for (int i = tid; i < kTile * (F / 4); i += kThreads) {
        const int m = i / (F / 4), c = 4 * (i % (F / 4));
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row0 + m < B) v = *reinterpret_cast<const f32x4 *>(d.x + (long long)(row0 + m) * d.ld_x + c);
        *reinterpret_cast<f32x4 *>(xs + m * ldx + c) = v;
    }
    __syncthreads();
    {
        const float *const in[2] = {xs, xs};
        float *const out[2] = {h1c, h1d};
        float *saved = kTrain ? p.h1 + (long long)k * B * H1 : nullptr;
        hidden_layer<1, kSets>(in, ldx, d.w1 + k * d.stride1, d.b1 + k * d.stride1, F, H1, d.activation, out, saved,
                               p.drop, p.drop.thr1, p.drop.scale1, draw, k, 0, row0, B);
    }
    __syncthreads();
    {
        const float *const in[2] = {h1c, h1d};
        float *const out[2] = {h2c, h2d};
        float *saved = kTrain ? p.h2 + (long long)k * B * H2 : nullptr;
        hidden_layer<kSets, kSets>(in, ld1, d.w2 + k * d.stride2, d.b2 + k * d.stride2, H1, H2, d.activation, out, saved,
                                   p.drop, p.drop.thr2, p.drop.scale2, draw, k, 1, row0, B);
    }
    __syncthreads();
    if (tid >= 64) return;
    // the output layer: one 16 x 16 tile, lane (kk, nn) = rows 4 kk + r of column nn
    const int kk = tid >> 4, nn = tid & 15;
    const bool col_ok = nn < A;
    const float *w3 = d.w3 + k * d.stride3;
    const float b3 = col_ok ? d.b3[k * d.stride3 + nn] : 0.f;
    f32x4 acc[kSets];
#pragma unroll
    for (int s = 0; s < kSets; ++s) acc[s] = f32x4{b3, b3, b3, b3};
    for (int k0 = 0; k0 < H2; k0 += 16) {
        f32x4 av[kSets];
        av[0] = *reinterpret_cast<const f32x4 *>(h2c + nn * ld2 + k0 + 4 * kk);
        if (kDrop) av[kSets - 1] = *reinterpret_cast<const f32x4 *>(h2d + nn * ld2 + k0 + 4 * kk);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float b = col_ok ? w3[(long long)(k0 + 4 * kk + j) * A + nn] : 0.f;
#pragma unroll
            for (int s = 0; s < kSets; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s][j], b, acc[s], 0, 0, 0);
        }
    }
    double lsum = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * kk + r;
        if (row >= B) continue;
        const float yc = acc[0][r];
        const int cmd = p.commands ? p.commands[row] : -1;
        const bool bad = p.commands && (cmd < 0 || cmd >= d.K);
        if (bad && k == 0 && nn == 0) atomicOr(p.status, RLX_CIL_STATUS_BAD_COMMAND);
        if (!col_ok) continue;
        const long long o = ((long long)k * B + row) * A + nn;
        if (p.y) p.y[o] = yc;
        if (!kTrain) {
            if (p.values && cmd == k) p.values[row * p.ld_values + nn] = yc;
            continue;
        }
        const float yt = acc[kSets - 1][r];
        const float target = cmd == k ? p.actions[row * p.ld_actions + nn] : yc;
        const float e = yt - target;
        const double ed = e, ea = fabs(ed);
        float g;
        if (p.huber) {                                   // tf.losses.huber_loss, delta = 1
            lsum += ea <= 1.0 ? 0.5 * ed * ed : ea - 0.5;
            g = e > 1.f ? 1.f : e < -1.f ? -1.f : e;
        } else {                                         // tf.losses.mean_squared_error
            lsum += ed * ed;
            g = 2.f * e;
        }
        if (p.y_train) p.y_train[o] = yt;
        p.dy[o] = p.dy_scale * g;
    }
    if (kTrain) {
        lsum = wave_sum_f64(lsum);
        if (tid == 0) p.partials[(long long)k * gridDim.x + blockIdx.x] = lsum;
    }
}

__global__ void __launch_bounds__(64) cil_loss_finish_kernel(const double *partials, int tiles, int K, float loss_scale,
                                                             float *losses, long long *draw, long long *draw_used) {
    __shared__ double head[RLX_CIL_MAX_BRANCHES];
    const int k = threadIdx.x;
    if (k < K) {
        double s = 0.0;
        for (int t = 0; t < tiles; ++t) s += partials[(long long)k * tiles + t];
        head[k] = (double)loss_scale * s;
        losses[k] = (float)head[k];
    }
    __syncthreads();
    if (k == 0) {
        double total = 0.0;
        for (int j = 0; j < K; ++j) total += head[j];
        losses[K] = (float)total;
        const long long used = *draw;
        *draw_used = used;
        *draw = used + 1;
    }
}

struct CilBwd {
    const float *dy, *h1, *h2;
    Dropout drop;
    const long long *draw_used;
    float *dz2, *dz1;
};

// t [16][N + 4] (LDS) holds dh; in place: dz = dh * mask * scale * act'(h * keep), rows beyond B zero; dz also to global
__device__ __forceinline__ void mask_and_derive(float *t, int N, const float *h, float *dz, const Dropout &dr, uint32_t thr,
                                                float scale, float keep, long long draw, int branch, int layer, int act,
                                                int row0, int B) {
    const int ld = N + 4;
    for (int i = threadIdx.x; i < kTile * (N / 4); i += kThreads) {
        const int m = i / (N / 4), c4 = i % (N / 4), row = row0 + m;
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (row < B) {
            const long long o = (long long)row * N + 4 * c4;
            const f32x4 hv = *reinterpret_cast<const f32x4 *>(h + o);
            g = *reinterpret_cast<const f32x4 *>(t + m * ld + 4 * c4);
            if (thr) g = dropped(g, mask_words(dr, draw, branch, layer, row, c4), thr, scale);
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] *= rlx::act_deriv_out(hv[q] * keep, act);
            *reinterpret_cast<f32x4 *>(dz + o) = g;
        }
        *reinterpret_cast<f32x4 *>(t + m * ld + 4 * c4) = g;
    }
}

__global__ void __launch_bounds__(kThreads) cil_backward_kernel(const rlx_cil_desc d, const CilBwd p) {
    extern __shared__ float lds[];
    const int k = blockIdx.y, row0 = blockIdx.x * kTile, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, kk = lane >> 4, nn = lane & 15;
    const int B = d.B, H1 = d.H1, H2 = d.H2, A = d.A;
    const int ldy = kTile + 4, ld1 = H1 + 4, ld2 = H2 + 4;
    float *dys = lds, *t2 = dys + kTile * ldy, *t1 = t2 + kTile * ld2;
    const long long draw = *p.draw_used;
    {
        const int m = tid >> 4, a = tid & 15, row = row0 + m;
        dys[m * ldy + a] = (row < B && a < A) ? p.dy[((long long)k * B + row) * A + a] : 0.f;
    }
    __syncthreads();
    const float *w3 = d.w3 + k * d.stride3;
    for (int c0 = 16 * wave; c0 < H2; c0 += 16 * kWaves) {                // dh2 = dy W3^T, reduction over a = 4 j + kk
        const int col = c0 + nn;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int a = 4 * j + kk;
            const float b = a < A ? w3[(long long)col * A + a] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dys[nn * ldy + a], b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) t2[(4 * kk + r) * ld2 + col] = acc[r];
    }
    __syncthreads();
    mask_and_derive(t2, H2, p.h2 + (long long)k * B * H2, p.dz2 + (long long)k * B * H2, p.drop, p.drop.thr2,
                    p.drop.scale2, p.drop.keep2, draw, k, 1, d.activation, row0, B);
    __syncthreads();
    const float *w2 = d.w2 + k * d.stride2;
    for (int c0 = 16 * wave; c0 < H1; c0 += 16 * kWaves) {                // dh1 = dz2 W2^T: rows of W2 are the B operand
        const int col = c0 + nn;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float *ap = t2 + nn * ld2 + 4 * kk;
        const float *bp = w2 + (long long)col * H2 + 4 * kk;
        for (int k0 = 0; k0 < H2; k0 += 16) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(ap + k0);
            const f32x4 b = *reinterpret_cast<const f32x4 *>(bp + k0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) t1[(4 * kk + r) * ld1 + col] = acc[r];
    }
    __syncthreads();
    mask_and_derive(t1, H1, p.h1 + (long long)k * B * H1, p.dz1 + (long long)k * B * H1, p.drop, p.drop.thr1,
                    p.drop.scale1, p.drop.keep1, draw, k, 0, d.activation, row0, B);
}

// obs [B][D] -> x [B][D - 1] (the columns around class_column, in order) and commands [B] = the class column as an
// integer; a thread per element of obs.  A value that is not finite, not integral or outside int32 becomes -1, which
// the branch kernels report as a bad command.
__global__ void __launch_bounds__(256) cil_split_observation_kernel(const float *obs, long long ld_obs, int B, int D,
                                                                    int class_column, float *x, long long ld_x,
                                                                    int *commands) {
    const long long n = (long long)B * D;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += 256ll * gridDim.x) {
        const int b = (int)(i / D), c = (int)(i % D);
        const float v = obs[b * ld_obs + c];
        if (c == class_column)
            commands[b] = (v >= 0.f && v < 2147483648.f && v == truncf(v)) ? (int)v : -1;
        else
            x[b * ld_x + (c < class_column ? c : c - 1)] = v;
    }
}

bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

int check_desc(const char *fn, const rlx_cil_desc *dp) {
    RLX_REQUIRE(dp, "%s: null descriptor", fn);
    const rlx_cil_desc &d = *dp;
    RLX_REQUIRE(d.K >= 2 && d.K <= RLX_CIL_MAX_BRANCHES, "%s: K = %d branches is not served ([2, %d])", fn, d.K,
                RLX_CIL_MAX_BRANCHES);
    RLX_REQUIRE(d.F % 16 == 0 && d.F >= 16 && d.F <= 512, "%s: F = %d is not served (a multiple of 16 in [16, 512]; no padding)",
                fn, d.F);
    RLX_REQUIRE(d.H1 % 16 == 0 && d.H1 >= 16 && d.H1 <= 256,
                "%s: H1 = %d is not served (a multiple of 16 in [16, 256]; no padding)", fn, d.H1);
    RLX_REQUIRE(d.H2 % 16 == 0 && d.H2 >= 16 && d.H2 <= 256,
                "%s: H2 = %d is not served (a multiple of 16 in [16, 256]; no padding)", fn, d.H2);
    RLX_REQUIRE(d.A >= 1 && d.A <= 16, "%s: A = %d is not served ([1, 16])", fn, d.A);
    RLX_REQUIRE(d.B >= 1 && d.B <= 1024, "%s: B = %d is not served ([1, 1024])", fn, d.B);
    RLX_REQUIRE(d.activation == RLX_ACT_NONE || d.activation == RLX_ACT_RELU || d.activation == RLX_ACT_TANH,
                "%s: activation = %d is not served (NONE, RELU, TANH)", fn, d.activation);
    RLX_REQUIRE(d.x && d.w1 && d.b1 && d.w2 && d.b2 && d.w3 && d.b3, "%s: null pointer (x, w1, b1, w2, b2, w3, b3)", fn);
    RLX_REQUIRE(d.ld_x >= d.F && d.ld_x % 4 == 0 && aligned16(d.x), "%s: ld_x = %lld (>= F, rows 16-byte aligned)", fn, d.ld_x);
    RLX_REQUIRE(d.stride1 % 4 == 0 && d.stride1 >= (long long)d.F * d.H1 && aligned16(d.w1) && aligned16(d.b1),
                "%s: stride1 = %lld (a multiple of 4, >= F * H1; w1 and b1 16-byte aligned)", fn, d.stride1);
    RLX_REQUIRE(d.stride2 % 4 == 0 && d.stride2 >= (long long)d.H1 * d.H2 && aligned16(d.w2) && aligned16(d.b2),
                "%s: stride2 = %lld (a multiple of 4, >= H1 * H2; w2 and b2 16-byte aligned)", fn, d.stride2);
    RLX_REQUIRE(d.stride3 >= (long long)d.H2 * d.A, "%s: stride3 = %lld (>= H2 * A)", fn, d.stride3);
    return RLX_OK;
}

int make_dropout(const char *fn, float rate1, float rate2, unsigned seed, unsigned rank, Dropout *out) {
    RLX_REQUIRE(rate1 >= 0.f && rate1 < 1.f && rate2 >= 0.f && rate2 < 1.f, "%s: dropout rates %g, %g (each in [0, 1))", fn,
                (double)rate1, (double)rate2);
    const auto thr = [](float rate) { return (uint32_t)((double)rate * 4294967296.0); };     // floor(rate * 2^32)
    *out = Dropout{thr(rate1), thr(rate2), 1.f / (1.f - rate1), 1.f / (1.f - rate2), 1.f - rate1, 1.f - rate2, seed, rank};
    return RLX_OK;
}

size_t forward_lds(const rlx_cil_desc &d, bool drop) {
    return sizeof(float) * kTile * ((d.F + 4) + (drop ? 2 : 1) * ((d.H1 + 4) + (d.H2 + 4)));
}

}  // namespace

extern "C" {

int rlx_cil_branches_forward(const rlx_cil_desc *desc_host, const int *commands, float *y, float *values,
                             long long ld_values, int *status, void *stream) {
    const char *fn = "rlx_cil_branches_forward";
    if (int rc = check_desc(fn, desc_host)) return rc;
    const rlx_cil_desc &d = *desc_host;
    RLX_REQUIRE(y || values, "%s: null pointer (y and values)", fn);
    RLX_REQUIRE(!commands == !values, "%s: commands and values come together", fn);
    RLX_REQUIRE(!values || (status && ld_values >= d.A), "%s: values needs status and ld_values = %lld >= A", fn, ld_values);
    CilRun p{};
    p.commands = commands; p.y = y; p.values = values; p.ld_values = ld_values; p.status = status;
    const size_t lds = forward_lds(d, false);
    RLX_HIP((rlx::allow_lds<cil_branches_kernel<false, false>>(lds)));
    RLX_LAUNCH((cil_branches_kernel<false, false>), dim3((d.B + kTile - 1) / kTile, d.K), kThreads, (unsigned)lds,
               rlx::as_stream(stream), d, p);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_cil_branches_train(const rlx_cil_desc *desc_host, const int *commands, const float *actions,
                           long long ld_actions, float rate1, float rate2, int huber, float loss_weight, float grad_scale,
                           unsigned int seed, unsigned int rank, long long *draw, long long *draw_used, float *y,
                           float *y_train, float *dy, float *h1, float *h2, float *losses, double *workspace, int *status,
                           void *stream) {
    const char *fn = "rlx_cil_branches_train";
    if (int rc = check_desc(fn, desc_host)) return rc;
    const rlx_cil_desc &d = *desc_host;
    RLX_REQUIRE(commands && actions && draw && draw_used && y && dy && h1 && h2 && losses && workspace && status,
                "%s: null pointer (commands, actions, draw, draw_used, y, dy, h1, h2, losses, workspace, status)", fn);
    RLX_REQUIRE(ld_actions >= d.A, "%s: ld_actions = %lld < A", fn, ld_actions);
    RLX_REQUIRE(draw != draw_used, "%s: draw_used must not be draw", fn);
    RLX_REQUIRE(aligned16(h1) && aligned16(h2), "%s: h1 and h2 are 16-byte aligned", fn);
    CilRun p{};
    if (int rc = make_dropout(fn, rate1, rate2, seed, rank, &p.drop)) return rc;
    p.commands = commands; p.y = y; p.actions = actions; p.ld_actions = ld_actions; p.draw = draw; p.huber = huber;
    p.loss_scale = loss_weight / (float)d.B; p.dy_scale = grad_scale * p.loss_scale;
    p.y_train = y_train; p.dy = dy; p.h1 = h1; p.h2 = h2; p.partials = workspace; p.status = status;
    const bool drop = p.drop.thr1 || p.drop.thr2;
    const int tiles = (d.B + kTile - 1) / kTile;
    const size_t lds = forward_lds(d, drop);
    hipStream_t s = rlx::as_stream(stream);
    if (drop) {
        RLX_HIP((rlx::allow_lds<cil_branches_kernel<true, true>>(lds)));
        RLX_LAUNCH((cil_branches_kernel<true, true>), dim3(tiles, d.K), kThreads, (unsigned)lds, s, d, p);
    } else {
        RLX_HIP((rlx::allow_lds<cil_branches_kernel<true, false>>(lds)));
        RLX_LAUNCH((cil_branches_kernel<true, false>), dim3(tiles, d.K), kThreads, (unsigned)lds, s, d, p);
    }
    RLX_LAUNCH_CHECK();
    RLX_LAUNCH((cil_loss_finish_kernel), 1, 64, 0, s, (const double *)workspace, tiles, d.K, p.loss_scale, losses, draw,
               draw_used);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_cil_branches_backward(const rlx_cil_desc *desc_host, const float *dy, const float *h1, const float *h2,
                              float rate1, float rate2, unsigned int seed, unsigned int rank,
                              const long long *draw_used, float *dz2, float *dz1, void *stream) {
    const char *fn = "rlx_cil_branches_backward";
    if (int rc = check_desc(fn, desc_host)) return rc;
    const rlx_cil_desc &d = *desc_host;
    RLX_REQUIRE(dy && h1 && h2 && draw_used && dz2 && dz1, "%s: null pointer (dy, h1, h2, draw_used, dz2, dz1)", fn);
    RLX_REQUIRE(aligned16(h1) && aligned16(h2) && aligned16(dz1) && aligned16(dz2), "%s: h1, h2, dz1, dz2 are 16-byte aligned", fn);
    CilBwd p{};
    if (int rc = make_dropout(fn, rate1, rate2, seed, rank, &p.drop)) return rc;
    p.dy = dy; p.h1 = h1; p.h2 = h2; p.draw_used = draw_used; p.dz2 = dz2; p.dz1 = dz1;
    const size_t lds = sizeof(float) * kTile * ((kTile + 4) + (d.H1 + 4) + (d.H2 + 4));
    RLX_HIP(rlx::allow_lds<cil_backward_kernel>(lds));
    RLX_LAUNCH((cil_backward_kernel), dim3((d.B + kTile - 1) / kTile, d.K), kThreads, (unsigned)lds, rlx::as_stream(stream),
               d, p);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_cil_split_observation(const float *obs, long long ld_obs, int B, int D, int class_column, float *x,
                               long long ld_x, int *commands, void *stream) {
    const char *fn = "rlx_cil_split_observation";
    RLX_REQUIRE(obs && x && commands, "%s: null pointer (obs, x, commands)", fn);
    RLX_REQUIRE(B >= 1 && D >= 2 && D <= 4096, "%s: B = %d rows of D = %d columns is not served (B >= 1, D in [2, 4096])", fn, B, D);
    RLX_REQUIRE(class_column >= 0 && class_column < D, "%s: class_column = %d outside [0, %d)", fn, class_column, D);
    RLX_REQUIRE(ld_obs >= D && ld_x >= D - 1, "%s: ld_obs = %lld < D or ld_x = %lld < D - 1", fn, ld_obs, ld_x);
    const long long n = (long long)B * D;
    const int blocks = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    RLX_LAUNCH((cil_split_observation_kernel), blocks, 256, 0, rlx::as_stream(stream), obs, ld_obs, B, D, class_column, x,
               ld_x, commands);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
