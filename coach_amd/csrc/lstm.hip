// LSTM middleware (rl_coach/architectures/tensorflow_components/middlewares/lstm_middleware.py: tf BasicLSTMCell(H,
// state_is_tuple=True), forget_bias 1): the recurrence over a window and its back-propagation through time, one launch
// each.  One kernel matrix [I + H][4H] (rows 0 .. I-1 multiply the input, rows I .. multiply h_{t-1}), gate column blocks
// i, j, f, o:
//   c_t = c_{t-1} * sigmoid(f + 1) + sigmoid(i) * tanh(j),   h_t = tanh(c_t) * sigmoid(o)
// The input projection Gx = X kernel[0:I] + bias of all rows and the weight / input gradients from dGates are ordinary
// products (rlx_gemm); what is sequential lives here.
//
// Work split (both kernels): S independent sequences of T steps, row s * T + t.  One workgroup per tile of 16 sequences
// (the M of v_mfma_f32_16x16x4_f32) owns ALL gate columns, because step t + 1 needs all of h_t: H / 16 waves, wave w owns
// cells [16 w, 16 w + 16) and the matching 16 columns of each of the four gate blocks.  No synchronisation between
// workgroups, no atomics; every sum has one order, so two launches give the same bits.
//
// lstm_forward_kernel.  h_{t-1} of the tile sits in LDS ([16][H + 4], two buffers: step t reads one and writes the
// other, ONE barrier per step).  The recurrent block is streamed from L2 / HBM every step with 16-byte loads along
// the 4H axis: lane (k = lane / 16, n = lane % 16) loads columns 4 c .. 4 c + 3 (c = n % 4) of the wave's 16 cells in gate
// block n / 4, for the four rows 16 s + 4 k + j.  Component q of that load is the B operand of accumulator q, so
// accumulator q holds, in column n, gate n / 4 of cell 4 c + q: the four accumulators together hold the wave's 16 x 64
// gate tile, but a cell's four gates lie in four lanes.  A 4 x 4 transposition between those lanes (three xor
// shuffles per accumulator row, once per step, after the K loop) brings i, j, f, o of cell 4 c + n / 4 into one lane; from
// there on c and h of a wave's cells live in that wave's registers for the whole window.
//
// lstm_backward_kernel.  Per step, last to first: the owning lane forms the pre-activation gate gradients from the saved
// activated gates and c (tanh c_t recomputed by the forward pass's own function), writes them to dGates[t] and to an
// LDS tile [16][4H + 4]; after a barrier dh_carry = dGates[t] * kernel[I:]^T, wave w producing its own 16 cells.  The
// transposed operand is read as ROWS of the recurrent block: the reduction index (4H) is the contiguous one there, so
// lane (k, n) takes 16 bytes of row 16 w + n per four MFMAs and no transposed copy has to be made per window.  Here the
// MFMA's output layout (column n = cell 16 w + n) is the owning layout, so nothing is exchanged.  Two barriers per
// step (the LDS tile is single: 64 KB at H = 256).
#include "lstm_math.hpp"
#include "rlx_device.hpp"

namespace {

using rlx::f32x4;

constexpr int kTile = 16;          // sequences per workgroup
constexpr int kMinCells = 16, kMaxCells = 256;

struct LstmFwd {
    const float *x;                // [S * T][ld_x], copied into xh[:, 0:I] (null with xh)
    long long ld_x;
    const float *gx;               // [S * T][ld_gx]: X kernel[0:I] + bias
    long long ld_gx;
    const float *wh;               // kernel[I:], [H][ld_w]
    long long ld_w;
    const float *c0, *h0;          // [S][H] or null (zeros)
    float *h_out;                  // [S * T][ld_h]
    long long ld_h;
    float *gates, *c_out;          // [S * T][4H], [S * T][H] or null
    float *xh;                     // [S * T][ld_xh] or null
    long long ld_xh;
    int I;
    float *c_fin, *h_fin;          // [S][H]
    float *c_prev, *h_prev;        // [S][H] or null
    int S, T, H;
};

__device__ __forceinline__ float sel4(float a, float b, float c, float d, int i) {
    return i == 0 ? a : i == 1 ? b : i == 2 ? c : d;
}

__global__ void __launch_bounds__(1024) lstm_forward_kernel(const LstmFwd p) {
    extern __shared__ float lds[];
    const int H = p.H, T = p.T, ldh = H + 4;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int kk = lane >> 4, nn = lane & 15, gq = nn >> 2, c4 = nn & 3;
    const int s0 = blockIdx.x * kTile;
    const int cell = 16 * w + 4 * c4 + gq;                     // the cell this lane updates, for rows 4 kk + r
    const long long gcol = (long long)gq * H + 16 * w + 4 * c4;   // first of the lane's four columns in a 4H row
    float creg[4], hreg[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = 4 * kk + r, s = s0 + m;
        const bool ok = s < p.S;
        const size_t o = (size_t)s * H + cell;
        creg[r] = (ok && p.c0) ? p.c0[o] : 0.f;
        hreg[r] = (ok && p.h0) ? p.h0[o] : 0.f;
        lds[m * ldh + cell] = hreg[r];
        if (ok && p.c_prev) {
            p.c_prev[o] = creg[r];
            p.h_prev[o] = hreg[r];
        }
    }
    if (p.xh) {             // xh[:, 0:I] = x for the tile's rows (sequence-major: one contiguous run of rows), once
        const long long r0 = (long long)s0 * T, rows = (long long)min(kTile, p.S - s0) * T;
        for (long long r = tid / 16; r < rows; r += blockDim.x / 16)
            for (int col = tid & 15; col < p.I; col += 16) p.xh[(r0 + r) * p.ld_xh + col] = p.x[(r0 + r) * p.ld_x + col];
    }
    __syncthreads();
    for (int step = 0; step < T; ++step) {
        const float *hc = lds + (step & 1) * kTile * ldh;
        float *hn = lds + ((step + 1) & 1) * kTile * ldh;
        f32x4 acc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = s0 + 4 * kk + r;
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
            if (s < p.S) g = *reinterpret_cast<const f32x4 *>(p.gx + ((long long)s * T + step) * p.ld_gx + gcol);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q][r] = g[q];
        }
        for (int k0 = 0; k0 < H; k0 += 16) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(hc + nn * ldh + k0 + 4 * kk);
            f32x4 b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                b[j] = *reinterpret_cast<const f32x4 *>(p.wh + (long long)(k0 + 4 * kk + j) * p.ld_w + gcol);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j][q], acc[q], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // the four lanes n = 4 g + c4 hold gate g of cells 4 c4 + q in acc[q]; lane g takes cell 4 c4 + g of every gate
            float rv[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const float snd = sel4(acc[0][r], acc[1][r], acc[2][r], acc[3][r], gq ^ x);
                rv[x] = x ? __shfl_xor(snd, 4 * x, 64) : snd;             // = gate gq ^ x of this lane's cell
            }
            const float pi = sel4(rv[0], rv[1], rv[2], rv[3], gq), pj = sel4(rv[0], rv[1], rv[2], rv[3], gq ^ 1);
            const float pf = sel4(rv[0], rv[1], rv[2], rv[3], gq ^ 2), po = sel4(rv[0], rv[1], rv[2], rv[3], gq ^ 3);
            const float gi = rlx::lstm_sigmoid(pi), gj = rlx::lstm_tanh(pj);
            const float gf = rlx::lstm_sigmoid(pf + 1.f), go = rlx::lstm_sigmoid(po);
            const float cn = creg[r] * gf + gi * gj;
            const float hv = rlx::lstm_tanh(cn) * go;
            const int m = 4 * kk + r, s = s0 + m;
            const bool ok = s < p.S;
            if (ok) {
                const long long row = (long long)s * T + step;
                if (p.xh) p.xh[row * p.ld_xh + p.I + cell] = hreg[r];
                p.h_out[row * p.ld_h + cell] = hv;
                if (p.gates) {
                    float *g = p.gates + row * 4 * H + cell;
                    g[0] = gi;
                    g[H] = gj;
                    g[2 * H] = gf;
                    g[3 * H] = go;
                    p.c_out[row * H + cell] = cn;
                }
            }
            creg[r] = ok ? cn : 0.f;
            hreg[r] = ok ? hv : 0.f;
            hn[m * ldh + cell] = hreg[r];
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int s = s0 + 4 * kk + r;
        if (s < p.S) {
            p.c_fin[(size_t)s * H + cell] = creg[r];
            p.h_fin[(size_t)s * H + cell] = hreg[r];
        }
    }
}

struct LstmBwd {
    const float *dh_out;           // [S * T][ld_dh]: gradient of the loss with respect to every h_t
    long long ld_dh;
    const float *gates, *c;        // what the forward pass saved
    const float *c0;               // [S][H] or null (zeros)
    const float *wh;
    long long ld_w;
    float *dgates;                 // [S * T][4H]
    int S, T, H;
};

__global__ void __launch_bounds__(1024) lstm_backward_kernel(const LstmBwd p) {
    extern __shared__ float lds[];
    const int H = p.H, T = p.T, ldg = 4 * H + 4;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int kk = lane >> 4, nn = lane & 15;
    const int s0 = blockIdx.x * kTile;
    const int cell = 16 * w + nn;                              // rows 4 kk + r: the MFMA's own output layout
    float dhc[4] = {0.f, 0.f, 0.f, 0.f}, dcc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int step = T - 1; step >= 0; --step) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 4 * kk + r, s = s0 + m;
            float di = 0.f, dj = 0.f, df = 0.f, dout = 0.f;
            if (s < p.S) {
                const long long row = (long long)s * T + step;
                const float *g = p.gates + row * 4 * H + cell;
                const float gi = g[0], gj = g[H], gf = g[2 * H], go = g[3 * H];
                const float ct = p.c[row * H + cell];
                const float cp = step > 0 ? p.c[(row - 1) * H + cell] : (p.c0 ? p.c0[(size_t)s * H + cell] : 0.f);
                const float dh = p.dh_out[row * p.ld_dh + cell] + dhc[r];
                const float tc = rlx::lstm_tanh(ct);
                const float dc = dcc[r] + dh * go * (1.f - tc * tc);
                dcc[r] = dc * gf;
                di = dc * gj * gi * (1.f - gi);
                dj = dc * gi * (1.f - gj * gj);
                df = dc * cp * gf * (1.f - gf);
                dout = dh * tc * go * (1.f - go);
                float *d = p.dgates + row * 4 * H + cell;
                d[0] = di;
                d[H] = dj;
                d[2 * H] = df;
                d[3 * H] = dout;
            }
            float *t = lds + m * ldg + cell;
            t[0] = di;
            t[H] = dj;
            t[2 * H] = df;
            t[3 * H] = dout;
        }
        if (step == 0) break;
        __syncthreads();
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float *ap = lds + nn * ldg + 4 * kk;
        const float *bp = p.wh + (long long)cell * p.ld_w + 4 * kk;
        for (int k0 = 0; k0 < 4 * H; k0 += 16) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(ap + k0);
            const f32x4 b = *reinterpret_cast<const f32x4 *>(bp + k0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dhc[r] = acc[r];
        __syncthreads();
    }
}

int check_shape(const char *fn, int S, int T, int H) {
    RLX_REQUIRE(H % 16 == 0 && H >= kMinCells && H <= kMaxCells,
                "%s: cells = %d is not served (a multiple of 16 in [%d, %d]; no padding)", fn, H, kMinCells, kMaxCells);
    RLX_REQUIRE(T >= 1, "%s: T = %d (a sequence has at least one step)", fn, T);
    RLX_REQUIRE(S >= 1, "%s: S = %d (at least one sequence)", fn, S);
    RLX_REQUIRE((long long)S * T < (1ll << 31), "%s: S * T = %lld rows", fn, (long long)S * T);
    return RLX_OK;
}

bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

extern "C" {

int rlx_lstm_forward(const float *x, long long ld_x, const float *gx, long long ld_gx, const float *recurrent,
                     long long ld_w, const float *c0, const float *h0, float *h_out, long long ld_h, float *gates,
                     float *c_out, float *xh, long long ld_xh, int input_features, float *c_final, float *h_final,
                     float *c_previous, float *h_previous, int S, int T, int cells, void *stream) {
    const char *fn = "rlx_lstm_forward";
    if (int rc = check_shape(fn, S, T, cells)) return rc;
    const int H = cells;
    RLX_REQUIRE(gx && recurrent && h_out && c_final && h_final, "%s: null pointer (gx, recurrent, h_out, c_final, h_final)", fn);
    RLX_REQUIRE(!c0 == !h0, "%s: c0 and h0 come together", fn);
    RLX_REQUIRE(!gates == !c_out, "%s: gates and c_out come together", fn);
    RLX_REQUIRE(!c_previous == !h_previous, "%s: c_previous and h_previous come together", fn);
    RLX_REQUIRE(!c_previous || (c_previous != c_final && c_previous != c0 && h_previous != h_final && h_previous != h0),
                "%s: c_previous / h_previous must not be the state they are a copy of (c0 / h0, c_final / h_final)", fn);
    RLX_REQUIRE(!xh || (x && input_features >= 1 && ld_x >= input_features && ld_xh >= input_features + H),
                "%s: xh needs x and input_features = %d <= ld_x = %lld, input_features + cells <= ld_xh = %lld", fn,
                input_features, ld_x, ld_xh);
    RLX_REQUIRE(ld_gx >= 4 * H && ld_gx % 4 == 0 && aligned16(gx), "%s: ld_gx = %lld (>= 4 * cells, rows 16-byte aligned)",
                fn, ld_gx);
    RLX_REQUIRE(ld_w >= 4 * H && ld_w % 4 == 0 && aligned16(recurrent),
                "%s: ld_w = %lld (>= 4 * cells, rows 16-byte aligned)", fn, ld_w);
    RLX_REQUIRE(ld_h >= H, "%s: ld_h = %lld < cells", fn, ld_h);
    const LstmFwd p{x, ld_x, gx, ld_gx, recurrent, ld_w, c0, h0, h_out, ld_h, gates, c_out, xh, ld_xh, input_features,
                    c_final, h_final, c_previous, h_previous, S, T, H};
    const size_t lds = (size_t)2 * kTile * (H + 4) * sizeof(float);
    RLX_HIP(rlx::allow_lds<lstm_forward_kernel>(lds));
    RLX_LAUNCH((lstm_forward_kernel), (S + kTile - 1) / kTile, 4 * H, (unsigned)lds, rlx::as_stream(stream), p);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_lstm_backward(const float *dh_out, long long ld_dh, const float *gates, const float *c, const float *c0,
                      const float *recurrent, long long ld_w, float *dgates, int S, int T, int cells, void *stream) {
    const char *fn = "rlx_lstm_backward";
    if (int rc = check_shape(fn, S, T, cells)) return rc;
    const int H = cells;
    RLX_REQUIRE(dh_out && gates && c && recurrent && dgates, "%s: null pointer (dh_out, gates, c, recurrent, dgates)", fn);
    RLX_REQUIRE(ld_dh >= H, "%s: ld_dh = %lld < cells", fn, ld_dh);
    RLX_REQUIRE(ld_w >= 4 * H && ld_w % 4 == 0 && aligned16(recurrent),
                "%s: ld_w = %lld (>= 4 * cells, rows 16-byte aligned)", fn, ld_w);
    const LstmBwd p{dh_out, ld_dh, gates, c, c0, recurrent, ld_w, dgates, S, T, H};
    const size_t lds = (size_t)kTile * (4 * H + 4) * sizeof(float);
    RLX_HIP(rlx::allow_lds<lstm_backward_kernel>(lds));
    RLX_LAUNCH((lstm_backward_kernel), (S + kTile - 1) / kTile, 4 * H, (unsigned)lds, rlx::as_stream(stream), p);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
