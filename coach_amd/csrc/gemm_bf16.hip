// bf16 mixed-precision dense layer: Y = act(X W + b), dX = dZ W^T, dW = X^T dZ (+ db = column sums of dZ) on the bf16
// matrix pipe of gfx950 (v_mfma_f32_16x16x32_bf16 / v_mfma_f32_32x32x16_bf16) with fp32 accumulators.
//
// Contract (include/rlx.h, DESIGN.md section 8 "bf16 dense path"): every operand and result in memory is fp32; each operand
// element is rounded fp32 -> bf16 (round to nearest even, NaN / Inf kept: bf16_rne below, the one conversion of the
// file) exactly once, on its way from the staging registers into LDS; two bf16 values multiply exactly in fp32, so only
// the fp32 accumulation rounds; bias, db and the activation are fp32.  No atomics, no partial sums in global memory: the
// order of every sum is a function of (M, K, N) alone.  The activation DERIVATIVE is not in here: G.Dense.backward
// applies it to dZ in place (rlx_act_backward) before it calls the two gradient products, as it does on the fp32 path.
//
// One kernel serves the three products as C[Mo, No] = A[Mo, Kr] B[Kr, No] with strided operands; what differs is which
// index of an operand is contiguous in memory:
//     forward      A = X  (reduction index contiguous)   B = W    (output column contiguous)   Kr = K
//     input_grad   A = dZ (reduction index contiguous)   B = W^T  (reduction index contiguous) Kr = N
//     weight_grad  A = X^T (output row contiguous)       B = dZ   (output column contiguous)   Kr = M
//
// Tiling.  A workgroup of 4 waves owns one BT x BT output tile and walks the reduction in slabs of 128.  Inside a slab the
// REDUCTION is split over the waves: wave w multiplies k in [32 w, 32 w + 32) of the slab for the whole tile (2 x 2
// accumulator tiles per wave), so every wave reads every operand row but only a quarter of its slab, and a long
// reduction over a small output (the weight gradient at batch 32 .. 256, the forward pass at K = 3136) keeps four matrix
// pipes busy without a second workgroup.  When the slabs are done the four partial tiles are added through LDS as
// (w0 + w1) + (w2 + w3): a fixed order, so two launches, and a replay of a captured graph, give the same bits.
//     small: BT = 32, v_mfma_f32_16x16x32_bf16 (one MFMA per accumulator tile and slab) -- every product whose OUTPUT has
//            fewer than 256 tiles of 64 x 64 (one per CU): the forward pass and the input gradient of a batch of 1 .. 64
//            rows at any layer width of this engine, and the weight gradient of its narrower layers;
//     large: BT = 64, v_mfma_f32_32x32x16_bf16 (two MFMAs per accumulator tile and slab) -- at least 256 tiles of 64 x 64
//            (the output of a weight gradient is K x N: at K = 3136, N = 512 it takes these at any batch).
// Ragged edges: loads beyond M / K / N are predicated off and zero-fill the LDS tile; stores are predicated.
//
// Fills and conversion.  Each thread fetches groups of 8 reduction-consecutive fp32 values of one operand row into
// registers -- two 16-byte loads where the reduction index is contiguous and the rows are 16-byte aligned, 8 coalesced
// 4-byte loads (the lanes of a wave run along the contiguous index) where it is not -- for slab s + 1 BEFORE the MFMAs
// of slab s are issued; the loads fly under the products, and the conversion and the one 16-byte LDS store per group
// come after them, between the two barriers that hand the single LDS tile pair from one slab to the next.
//
// LDS layout.  Both operand tiles are K-major: row r of the tile (an output row of A, an output column of B) holds its
// 128 bf16 of the slab, rows 136 bf16 (272 bytes, 68 banks' worth) apart.  A lane's MFMA operand is the 8 consecutive
// bf16 at [r][32 w + 8 q] -- one ds_read_b128; consecutive rows start 4 banks apart, so the 16 / 32 rows that the lanes
// of one read phase touch fall on distinct banks, and the staging stores (same shape: 16 bytes per lane, lanes along
// the rows or along one row) are conflict-free as well.
//
// weight_grad's db.  The workgroups of output-row tile 0 already hold the unrounded fp32 dZ slabs in their staging
// registers (dZ is their B operand): each thread adds the values it stages -- always the same column, rows in ascending
// order -- into one fp32 partial, and the 256 / BT partials of a column are added in ascending order through LDS at the
// end.  db sums the fp32 values, not their bf16 roundings.
#include <cstdint>
#include "rlx_device.hpp"

namespace rlx {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kThreads = 256;
constexpr int kSlab = 128;            // reduction elements per slab: 4 waves x 32
constexpr int kLdt = kSlab + 8;       // bf16 per LDS tile row (see "LDS layout")

// fp32 -> bf16, round to nearest even; NaN stays NaN (quiet bit set, so a payload in the low half cannot turn it into
// Inf), Inf stays Inf, a finite value beyond the largest bf16 rounds to Inf as IEEE rounding does.
__device__ __forceinline__ unsigned bf16_rne(float v) {
    const unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

struct Bf16Problem {
    const float *A;          // A(i, k) = A[i * a_os + k * a_ks]
    const float *B;          // B(k, j) = B[j * b_os + k * b_ks]
    float *C;                // C(i, j) = C[i * ldc + j]
    const float *bias;       // [No] or nullptr
    float *colsum;           // [No] or nullptr: sum_k B(k, j) in fp32 (kColsum kernels)
    long long a_os, a_ks, b_os, b_ks, ldc;
    int Mo, No, Kr, act;
    int a_vec, b_vec;        // 16-byte loads along the reduction index are aligned for every row
};

// Group p of this thread in a BT x 128 operand tile: (tile row, first reduction index / 8).
template <int BT, bool kKContig>
__device__ __forceinline__ void stage_group(int p, int &row, int &kg) {
    const int g = p * kThreads + (int)threadIdx.x;
    if (kKContig) {
        kg = g & 15;
        row = g >> 4;
    } else {
        row = g & (BT - 1);
        kg = g / BT;
    }
}

// raw[p][0 .. 7] = P(o0 + row, k0 + 8 kg + 0 .. 7), zero outside the operand
template <int BT, bool kKContig>
__device__ __forceinline__ void stage_load(float (&raw)[BT * 16 / kThreads][8], const float *P, long long os, long long ks,
                                           int o0, int o_end, int k0, int k_end, bool vec) {
#pragma unroll
    for (int p = 0; p < BT * 16 / kThreads; ++p) {
        int row, kg;
        stage_group<BT, kKContig>(p, row, kg);
        const int o = o0 + row, k = k0 + 8 * kg;
        const bool in = o < o_end;
        if (kKContig) {
            const float *src = in ? P + (long long)o * os + k : P;      // (no address is formed for a row beyond the operand)
            if (in && vec && k + 8 <= k_end) {
                const float4 lo = *reinterpret_cast<const float4 *>(src);
                const float4 hi = *reinterpret_cast<const float4 *>(src + 4);
                raw[p][0] = lo.x, raw[p][1] = lo.y, raw[p][2] = lo.z, raw[p][3] = lo.w;
                raw[p][4] = hi.x, raw[p][5] = hi.y, raw[p][6] = hi.z, raw[p][7] = hi.w;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) raw[p][j] = (in && k + j < k_end) ? src[j] : 0.f;
            }
        } else {
            const float *src = in ? P + o + (long long)k * ks : P;
#pragma unroll
            for (int j = 0; j < 8; ++j) raw[p][j] = (in && k + j < k_end) ? src[(long long)j * ks] : 0.f;
        }
    }
}

// the staged groups, rounded to bf16, into the K-major LDS tile: one 16-byte store per group
template <int BT, bool kKContig>
__device__ __forceinline__ void stage_store(const float (&raw)[BT * 16 / kThreads][8], unsigned short *tile) {
#pragma unroll
    for (int p = 0; p < BT * 16 / kThreads; ++p) {
        int row, kg;
        stage_group<BT, kKContig>(p, row, kg);
        uint4 v;
        v.x = bf16_rne(raw[p][0]) | (bf16_rne(raw[p][1]) << 16);
        v.y = bf16_rne(raw[p][2]) | (bf16_rne(raw[p][3]) << 16);
        v.z = bf16_rne(raw[p][4]) | (bf16_rne(raw[p][5]) << 16);
        v.w = bf16_rne(raw[p][6]) | (bf16_rne(raw[p][7]) << 16);
        *reinterpret_cast<uint4 *>(tile + row * kLdt + 8 * kg) = v;
    }
}

__device__ __forceinline__ bf16x8 lds_operand(const unsigned short *p) {
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(p));
}

// kLarge: 64 x 64 tile on 32x32x16 MFMAs, else 32 x 32 on 16x16x32.  kAK / kBK: the reduction index of A / B is the
// contiguous one.  kColsum: the workgroups of output-row tile 0 also write colsum.
template <bool kLarge, bool kAK, bool kBK, bool kColsum>
__global__ __launch_bounds__(kThreads) void dense_bf16_kernel(Bf16Problem g) {
    constexpr int BT = kLarge ? 64 : 32;
    constexpr int SUB = BT / 2;                    // one MFMA accumulator tile
    constexpr int GR = BT * 16 / kThreads;         // staged groups per thread and operand
    constexpr int NACC = kLarge ? 16 : 4;          // accumulator registers per MFMA tile
    constexpr int LDR = BT + 1;                    // fp32 row stride of the partial tiles in the wave reduction
    static_assert(2 * BT * LDR * 4 <= 2 * BT * kLdt * 2, "the two partial tiles reuse the operand tiles' LDS");
    static_assert(kThreads * 4 <= 2 * BT * kLdt * 2, "so do the column-sum partials");
    __shared__ __attribute__((aligned(16))) unsigned short lds[2 * BT * kLdt];
    unsigned short *As = lds, *Bs = lds + BT * kLdt;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i0 = blockIdx.y * BT, j0 = blockIdx.x * BT;
    const bool sums = kColsum && blockIdx.y == 0;

    float ra[GR][8], rb[GR][8];
    float acc[2][2][NACC];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < NACC; ++r) acc[a][b][r] = 0.f;
    float csum = 0.f;

    auto fetch = [&](int k0) {
        stage_load<BT, kAK>(ra, g.A, g.a_os, g.a_ks, i0, g.Mo, k0, g.Kr, g.a_vec != 0);
        stage_load<BT, kBK>(rb, g.B, g.b_os, g.b_ks, j0, g.No, k0, g.Kr, g.b_vec != 0);
        if (sums) {        // this thread's column (tid % BT), rows ascending; entries outside the operand are zeros
#pragma unroll
            for (int p = 0; p < GR; ++p)
#pragma unroll
                for (int j = 0; j < 8; ++j) csum += rb[p][j];
        }
    };
    auto commit = [&]() {
        stage_store<BT, kAK>(ra, As);
        stage_store<BT, kBK>(rb, Bs);
    };

    // lane -> (row inside an MFMA tile, first reduction index of its operand inside the wave's 32)
    const int lrow = kLarge ? (lane & 31) : (lane & 15);
    const int lk = kLarge ? 8 * (lane >> 5) : 8 * (lane >> 4);

    fetch(0);
    commit();
    __syncthreads();
    for (int k0 = 0; k0 < g.Kr; k0 += kSlab) {
        const bool more = k0 + kSlab < g.Kr;
        if (more) fetch(k0 + kSlab);
#pragma unroll
        for (int step = 0; step < (kLarge ? 2 : 1); ++step) {
            const int kofs = 32 * w + 16 * step + lk;
            bf16x8 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = lds_operand(As + (t * SUB + lrow) * kLdt + kofs);
                b[t] = lds_operand(Bs + (t * SUB + lrow) * kLdt + kofs);
            }
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj) {
                    if constexpr (kLarge) {
                        f32x16 c;
#pragma unroll
                        for (int r = 0; r < 16; ++r) c[r] = acc[ti][tj][r];
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ti], b[tj], c, 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[ti][tj][r] = c[r];
                    } else {
                        f32x4 c;
#pragma unroll
                        for (int r = 0; r < 4; ++r) c[r] = acc[ti][tj][r];
                        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ti], b[tj], c, 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[ti][tj][r] = c[r];
                    }
                }
        }
        __syncthreads();             // every wave has read the tiles of this slab
        if (more) commit();
        __syncthreads();
    }

    // ---- the four waves' partial tiles: (w0 + w1) + (w2 + w3) through two fp32 tiles in LDS
    float *part = reinterpret_cast<float *>(lds) + (w >> 1) * BT * LDR;
    auto element = [&](int ti, int tj, int r) {       // tile-local offset of accumulator register r
        const int row = kLarge ? ti * 32 + mfma_row(r, lane >> 5) : ti * 16 + 4 * (lane >> 4) + r;
        const int col = kLarge ? tj * 32 + (lane & 31) : tj * 16 + (lane & 15);
        return row * LDR + col;
    };
    auto dump = [&]() {
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < NACC; ++r) part[element(ti, tj, r)] = acc[ti][tj][r];
    };
    if (w & 1) dump();
    __syncthreads();
    if (!(w & 1)) {
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < NACC; ++r) acc[ti][tj][r] += part[element(ti, tj, r)];
    }
    __syncthreads();
    if (!(w & 1)) dump();
    __syncthreads();

    // ---- epilogue, all 256 threads, rows of the tile coalesced: bias and activation in fp32
    const float *p0 = reinterpret_cast<const float *>(lds), *p1 = p0 + BT * LDR;
    for (int e = tid; e < BT * BT; e += kThreads) {
        const int r = e / BT, c = e % BT;
        const int row = i0 + r, col = j0 + c;
        if (row < g.Mo && col < g.No) {
            float v = p0[r * LDR + c] + p1[r * LDR + c];
            if (g.bias) v += g.bias[col];
            g.C[(long long)row * g.ldc + col] = act_apply(v, g.act);
        }
    }
    if (sums) {                      // (blockIdx.y is uniform: every thread of the workgroup takes the barriers)
        float *red = reinterpret_cast<float *>(lds);
        __syncthreads();
        red[tid] = csum;
        __syncthreads();
        if (tid < BT && j0 + tid < g.No) {
            float s = red[tid];
            for (int q = 1; q < kThreads / BT; ++q) s += red[tid + q * BT];
            g.colsum[j0 + tid] = s;
        }
    }
}

bool aligned16(const void *p, long long row_stride) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && row_stride % 4 == 0;
}

template <bool kAK, bool kBK, bool kColsum>
int launch_bf16(Bf16Problem g, void *stream) {
    g.a_vec = kAK && aligned16(g.A, g.a_os);
    g.b_vec = kBK && aligned16(g.B, g.b_os);
    const long long tiles64 = (long long)((g.Mo + 63) / 64) * ((g.No + 63) / 64);
    const dim3 block(kThreads);
    if (tiles64 >= 256) {
        const dim3 grid((g.No + 63) / 64, (g.Mo + 63) / 64);
        RLX_LAUNCH((dense_bf16_kernel<true, kAK, kBK, kColsum>), grid, block, 0, as_stream(stream), g);
    } else {
        const dim3 grid((g.No + 31) / 32, (g.Mo + 31) / 32);
        RLX_LAUNCH((dense_bf16_kernel<false, kAK, kBK, kColsum>), grid, block, 0, as_stream(stream), g);
    }
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int check_shape(const char *what, int M, int K, int N) {
    RLX_REQUIRE(M >= 1 && M <= 4096, "%s: M = %d is outside 1 .. 4096", what, M);
    RLX_REQUIRE(K >= 1 && K <= 8192, "%s: K = %d is outside 1 .. 8192", what, K);
    RLX_REQUIRE(N >= 1 && N <= 8192, "%s: N = %d is outside 1 .. 8192", what, N);
    return RLX_OK;
}

}  // namespace
}  // namespace rlx

using namespace rlx;

extern "C" int rlx_dense_bf16_forward(const float *x, long long ldx, const float *w, long long ldw, const float *bias,
                                      float *y, long long ldy, int M, int K, int N, int activation, void *stream) {
    RLX_REQUIRE(x && w && y, "rlx_dense_bf16_forward: null x, w or y");
    if (int e = check_shape("rlx_dense_bf16_forward", M, K, N)) return e;
    RLX_REQUIRE(ldx >= K && ldw >= N && ldy >= N, "rlx_dense_bf16_forward: a row stride is shorter than its row");
    RLX_REQUIRE(activation >= RLX_ACT_NONE && activation <= RLX_ACT_TANH,
                "rlx_dense_bf16_forward: activation %d is not served (none, relu, tanh)", activation);
    Bf16Problem g{};
    g.A = x, g.a_os = ldx, g.a_ks = 1;
    g.B = w, g.b_os = 1, g.b_ks = ldw;
    g.C = y, g.ldc = ldy, g.bias = bias;
    g.Mo = M, g.No = N, g.Kr = K, g.act = activation;
    return launch_bf16<true, false, false>(g, stream);
}

extern "C" int rlx_dense_bf16_input_grad(const float *dz, long long lddz, const float *w, long long ldw, float *dx,
                                         long long lddx, int M, int K, int N, void *stream) {
    RLX_REQUIRE(dz && w && dx, "rlx_dense_bf16_input_grad: null dz, w or dx");
    if (int e = check_shape("rlx_dense_bf16_input_grad", M, K, N)) return e;
    RLX_REQUIRE(lddz >= N && ldw >= N && lddx >= K, "rlx_dense_bf16_input_grad: a row stride is shorter than its row");
    Bf16Problem g{};
    g.A = dz, g.a_os = lddz, g.a_ks = 1;
    g.B = w, g.b_os = ldw, g.b_ks = 1;              // B(n, k) = W[k][n]
    g.C = dx, g.ldc = lddx;
    g.Mo = M, g.No = K, g.Kr = N, g.act = RLX_ACT_NONE;
    return launch_bf16<true, true, false>(g, stream);
}

extern "C" int rlx_dense_bf16_weight_grad(const float *x, long long ldx, const float *dz, long long lddz, float *dw,
                                          long long lddw, float *db, int M, int K, int N, void *stream) {
    RLX_REQUIRE(x && dz && dw, "rlx_dense_bf16_weight_grad: null x, dz or dw");
    if (int e = check_shape("rlx_dense_bf16_weight_grad", M, K, N)) return e;
    RLX_REQUIRE(ldx >= K && lddz >= N && lddw >= N, "rlx_dense_bf16_weight_grad: a row stride is shorter than its row");
    Bf16Problem g{};
    g.A = x, g.a_os = 1, g.a_ks = ldx;              // A(k, m) = X[m][k]
    g.B = dz, g.b_os = 1, g.b_ks = lddz;
    g.C = dw, g.ldc = lddw, g.colsum = db;
    g.Mo = K, g.No = N, g.Kr = M, g.act = RLX_ACT_NONE;
    return db ? launch_bf16<false, false, true>(g, stream) : launch_bf16<false, false, false>(g, stream);
}
