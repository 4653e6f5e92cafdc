// Factorised NoisyNet dense layer (Fortunato et al. 2017; rl_coach/architectures/tensorflow_components/layers.py:196-257):
//   W = weight_mean + weight_stddev * (f_in outer f_out),  b = bias_mean + bias_stddev * f_b,  y = act(x W + b)
// with the noise vectors f = [f_in (K) | f_out (N) | f_b (N)] sampled per pass by rlx_noisy_sample (csrc/noise.hip).
// The noisy matrix W is never formed: the factorisation moves the noise onto the operands,
//   forward : y  = act( x Wm + ((x * f_in) Ws) * f_out + bm + bs * f_b )
//   dx      : dx = ( dz Wm^T + ((dz * f_out) Ws^T) * f_in ) * act'(x)
//   dW      : dWm = x^T dz, dWs[k][n] = dWm[k][n] f_in[k] f_out[n], dbm = 1^T dz, dbs = dbm * f_b
// so forward and dx are the SAME product kernel (two fp32 MFMA accumulators per 32 x 32 output tile, one per weight
// matrix, each weight matrix read once per 32 rows of the batch), with the weights read plain or transposed, and the
// weight gradient is one product whose epilogue writes both matrices.
//
// noisy_prod_kernel: a workgroup (4 waves) owns a 32 x 32 output tile and one chunk of the reduction index.  Per step
// of 64 reduction elements the operand rows (plain and pre-scaled by the noise along the reduction index) and both
// weight tiles are staged in LDS as [row][65] images (odd stride: the 32 lanes of a half wave, which read one column
// of 32 rows, hit 32 banks); each wave runs a quarter of the step through v_mfma_f32_32x32x2_f32 (exact fp32, k-ordered
// chains), the four wave partials are added in a fixed order through LDS.  The reduction index is split over
// workgroups by shape alone (about 512 workgroups), the partial tiles go to a workspace and noisy_reduce_kernel adds
// them in split order and applies the epilogue: sums are bit-identical run to run.  With one split the epilogue
// runs in the product kernel.
#include "rlx_device.hpp"

namespace {

using rlx::f32x16;

constexpr int kRC = 64;            // reduction elements per staged step
constexpr int kLd = kRC + 1;       // LDS row stride in floats
constexpr int kTargetWgs = 512;

struct NoisyProd {
    const float *a;            // [M][lda]: x (forward) or dz (input gradient)
    long long lda;
    const float *wm, *ws;      // weight_mean, weight_stddev [K][N] row-major
    int ldw;                   // N
    const float *rscale;       // noise along the reduction index (f_in forward, f_out input gradient)
    const float *oscale;       // noise along the output column (f_out forward, f_in input gradient)
    const float *bm, *bs, *fb; // forward epilogue: bias_mean, bias_stddev, f_b (null: input gradient)
    const float *aux;          // input gradient epilogue: the lower layer's output (null: none)
    long long ld_aux;
    float *out;
    long long ldo;
    float *partials;           // [splits][M][J]
    int M, R, J;               // rows, reduction length, output columns
    int splits, rchunk;        // rchunk: a multiple of kRC
    int act, deriv;
};

__device__ __forceinline__ float nd_epilogue(const NoisyProd &p, float v, int m, int j) {
    if (p.bm) {
        v += p.bm[j] + p.bs[j] * p.fb[j];
        return rlx::act_apply(v, p.act);
    }
    if (p.aux) v *= rlx::act_deriv_out(p.aux[(size_t)m * p.ld_aux + j], p.deriv);
    return v;
}

// TRANS = false: the weight element of (reduction r, column j) is w[r * ldw + j] (forward);
// TRANS = true : w[j * ldw + r] (input gradient: the reduction runs over the layer's units).
template <bool TRANS>
__global__ void __launch_bounds__(256) noisy_prod_kernel(const NoisyProd p) {
    __shared__ float smem[4 * 32 * kLd];
    float(*as0)[kLd] = reinterpret_cast<float(*)[kLd]>(smem);
    float(*as1)[kLd] = reinterpret_cast<float(*)[kLd]>(smem + 32 * kLd);
    float(*bs0)[kLd] = reinterpret_cast<float(*)[kLd]>(smem + 2 * 32 * kLd);
    float(*bs1)[kLd] = reinterpret_cast<float(*)[kLd]>(smem + 3 * 32 * kLd);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int j0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
    const int r_begin = blockIdx.z * p.rchunk;
    const int r_end = min(p.R, r_begin + p.rchunk);
    f32x16 accm, accs;
#pragma unroll
    for (int i = 0; i < 16; ++i) accm[i] = accs[i] = 0.f;

    for (int r0 = r_begin; r0 < r_end; r0 += kRC) {
        {   // operand rows: 4 rows per pass, 64 consecutive reduction elements each
            const int rr = t & 63, r = r0 + rr;
            const float sc = r < r_end ? p.rscale[r] : 0.f;
            for (int i = t >> 6; i < 32; i += 4) {
                const int m = m0 + i;
                const float v = (m < p.M && r < r_end) ? p.a[(size_t)m * p.lda + r] : 0.f;
                as0[i][rr] = v;
                as1[i][rr] = v * sc;
            }
        }
        if (TRANS) {
            const int rr = t & 63, r = r0 + rr;
            for (int j = t >> 6; j < 32; j += 4) {
                const int jj = j0 + j;
                const bool ok = jj < p.J && r < r_end;
                const size_t o = (size_t)jj * p.ldw + r;
                bs0[j][rr] = ok ? p.wm[o] : 0.f;
                bs1[j][rr] = ok ? p.ws[o] : 0.f;
            }
        } else {
            const int j = t & 31, jj = j0 + j;
            for (int rr = t >> 5; rr < kRC; rr += 8) {
                const int r = r0 + rr;
                const bool ok = jj < p.J && r < r_end;
                const size_t o = (size_t)r * p.ldw + jj;
                bs0[j][rr] = ok ? p.wm[o] : 0.f;
                bs1[j][rr] = ok ? p.ws[o] : 0.f;
            }
        }
        __syncthreads();
        const int rb = wave * (kRC / 4) + (lane >> 5), row = lane & 31;
#pragma unroll
        for (int s = 0; s < kRC / 8; ++s) {
            const int rr = rb + 2 * s;
            accm = __builtin_amdgcn_mfma_f32_32x32x2f32(as0[row][rr], bs0[row][rr], accm, 0, 0, 0);
            accs = __builtin_amdgcn_mfma_f32_32x32x2f32(as1[row][rr], bs1[row][rr], accs, 0, 0, 0);
        }
        __syncthreads();
    }
    // wave partials -> LDS [wave][row][col]; C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2)
    // + 4 (lane >> 5)
    float *red = smem;
    {
        const int col = lane & 31, j = j0 + col;
        const float os = j < p.J ? p.oscale[j] : 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            red[(wave * 32 + row) * 32 + col] = accm[reg] + accs[reg] * os;
        }
    }
    __syncthreads();
    for (int idx = t; idx < 1024; idx += 256) {
        const int row = idx >> 5, col = idx & 31, m = m0 + row, j = j0 + col;
        if (m >= p.M || j >= p.J) continue;
        const float v = ((red[idx] + red[1024 + idx]) + red[2048 + idx]) + red[3072 + idx];
        if (p.splits > 1) p.partials[((size_t)blockIdx.z * p.M + m) * p.J + j] = v;
        else p.out[(size_t)m * p.ldo + j] = nd_epilogue(p, v, m, j);
    }
}

__global__ void __launch_bounds__(256) noisy_reduce_kernel(const NoisyProd p) {
    const long long mj = (long long)p.M * p.J;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < mj; i += gridDim.x * 256ll) {
        const int m = (int)(i / p.J), j = (int)(i - (long long)m * p.J);
        float v = p.partials[i];
        for (int s = 1; s < p.splits; ++s) v += p.partials[(size_t)s * mj + i];
        p.out[(size_t)m * p.ldo + j] = nd_epilogue(p, v, m, j);
    }
}

struct NoisyDw {
    const float *x, *dz;
    long long ldx, lddz;
    const float *f_in, *f_out, *f_b;
    float *dwm, *dws, *dbm, *dbs;
    int M, K, N;
};

// One wave per 32 (k) x 32 (n) tile of dWm = x^T dz, the batch in steps of two rows; operands straight from global
// memory (both are read along their rows: 128-byte segments).  The epilogue writes dWm and dWs; the workgroups of the
// first k block also sum dz's columns (row order) for the two bias gradients.
__global__ void __launch_bounds__(256) noisy_dw_kernel(const NoisyDw p) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n0 = blockIdx.x * 32, k0 = (blockIdx.y * 4 + wave) * 32;
    if (k0 < p.K) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        const int kk = k0 + (lane & 31), nn = n0 + (lane & 31);
        for (int m = 0; m < p.M; m += 2) {
            const int mm = m + (lane >> 5);
            const float a = (mm < p.M && kk < p.K) ? p.x[(size_t)mm * p.ldx + kk] : 0.f;
            const float b = (mm < p.M && nn < p.N) ? p.dz[(size_t)mm * p.lddz + nn] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        if (nn < p.N) {
            const float fo = p.f_out[nn];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int k = k0 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                if (k < p.K) {
                    const size_t o = (size_t)k * p.N + nn;
                    p.dwm[o] = acc[reg];
                    p.dws[o] = acc[reg] * p.f_in[k] * fo;
                }
            }
        }
    }
    if (blockIdx.y == 0 && t < 32 && n0 + t < p.N) {
        const int n = n0 + t;
        float s = 0.f;
        for (int m = 0; m < p.M; ++m) s += p.dz[(size_t)m * p.lddz + n];
        p.dbm[n] = s;
        p.dbs[n] = s * p.f_b[n];
    }
}

// reduction chunking of a product with `tiles` output tiles and reduction length R: by shape alone
void chunking(int tiles, int R, int &splits, int &rchunk) {
    const int steps = (R + kRC - 1) / kRC;
    int want = kTargetWgs / tiles;
    if (want < 1) want = 1;
    if (want > steps) want = steps;
    rchunk = (steps + want - 1) / want * kRC;
    splits = (R + rchunk - 1) / rchunk;
}

int launch_prod(NoisyProd &p, bool trans, float *workspace, long long workspace_floats, const char *fn, hipStream_t s) {
    const int tj = (p.J + 31) / 32, tm = (p.M + 31) / 32;
    chunking(tj * tm, p.R, p.splits, p.rchunk);
    if (p.splits > 1) {
        RLX_REQUIRE(workspace && workspace_floats >= (long long)p.splits * p.M * p.J,
                    "%s: workspace too small (%lld floats, need %lld)", fn, workspace_floats,
                    (long long)p.splits * p.M * p.J);
        p.partials = workspace;
    }
    dim3 grid(tj, tm, p.splits);
    if (trans) RLX_LAUNCH((noisy_prod_kernel<true>), grid, 256, 0, s, p);
    else RLX_LAUNCH((noisy_prod_kernel<false>), grid, 256, 0, s, p);
    RLX_LAUNCH_CHECK();
    if (p.splits > 1) {
        RLX_LAUNCH((noisy_reduce_kernel), rlx::grid_for((long long)p.M * p.J, 256), 256, 0, s, p);
        RLX_LAUNCH_CHECK();
    }
    return RLX_OK;
}

}  // namespace

extern "C" {

int rlx_noisy_dense_workspace_floats(int M, int K, int N, long long *floats_host) {
    RLX_REQUIRE(floats_host, "rlx_noisy_dense_workspace_floats: null pointer");
    RLX_REQUIRE(M > 0 && K > 0 && N > 0, "rlx_noisy_dense_workspace_floats: bad shape (M=%d K=%d N=%d)", M, K, N);
    int sf, sb, rc;
    const int tm = (M + 31) / 32;
    chunking(((N + 31) / 32) * tm, K, sf, rc);
    chunking(((K + 31) / 32) * tm, N, sb, rc);
    const long long f = sf > 1 ? (long long)sf * M * N : 0, b = sb > 1 ? (long long)sb * M * K : 0;
    *floats_host = f > b ? f : b;
    return RLX_OK;
}

int rlx_noisy_dense_forward(const float *x, long long ldx, const float *weight_mean, const float *weight_stddev,
                            const float *bias_mean, const float *bias_stddev, const float *noise, float *y,
                            long long ldy, int M, int K, int N, int activation, float *workspace,
                            long long workspace_floats, void *stream) {
    RLX_REQUIRE(x && weight_mean && weight_stddev && bias_mean && bias_stddev && noise && y,
                "rlx_noisy_dense_forward: null pointer");
    RLX_REQUIRE(M > 0 && K > 0 && N > 0 && ldx >= K && ldy >= N,
                "rlx_noisy_dense_forward: bad shape (M=%d K=%d N=%d ldx=%lld ldy=%lld)", M, K, N, ldx, ldy);
    RLX_REQUIRE(activation >= 0 && activation <= 2, "rlx_noisy_dense_forward: unknown activation");
    NoisyProd p{};
    p.a = x; p.lda = ldx; p.wm = weight_mean; p.ws = weight_stddev; p.ldw = N;
    p.rscale = noise; p.oscale = noise + K; p.bm = bias_mean; p.bs = bias_stddev; p.fb = noise + K + N;
    p.out = y; p.ldo = ldy; p.M = M; p.R = K; p.J = N; p.act = activation;
    return launch_prod(p, false, workspace, workspace_floats, "rlx_noisy_dense_forward", rlx::as_stream(stream));
}

int rlx_noisy_dense_backward(const float *x, long long ldx, const float *weight_mean, const float *weight_stddev,
                             const float *dz, long long lddz, const float *noise, float *d_weight_mean,
                             float *d_weight_stddev, float *d_bias_mean, float *d_bias_stddev, float *dx,
                             long long lddx, int M, int K, int N, int lower_activation, float *workspace,
                             long long workspace_floats, void *stream) {
    RLX_REQUIRE(x && weight_mean && weight_stddev && dz && noise, "rlx_noisy_dense_backward: null pointer");
    const bool dw = d_weight_mean != nullptr;
    RLX_REQUIRE(dw || dx, "rlx_noisy_dense_backward: nothing to produce");
    RLX_REQUIRE(!dw || (d_weight_stddev && d_bias_mean && d_bias_stddev),
                "rlx_noisy_dense_backward: null pointer (the four parameter gradients come together)");
    RLX_REQUIRE(M > 0 && K > 0 && N > 0 && ldx >= K && lddz >= N && (!dx || lddx >= K),
                "rlx_noisy_dense_backward: bad shape (M=%d K=%d N=%d ldx=%lld lddz=%lld lddx=%lld)", M, K, N, ldx, lddz,
                lddx);
    RLX_REQUIRE(lower_activation >= 0 && lower_activation <= 2, "rlx_noisy_dense_backward: unknown activation");
    hipStream_t s = rlx::as_stream(stream);
    if (dw) {
        NoisyDw q{x, dz, ldx, lddz, noise, noise + K, noise + K + N, d_weight_mean, d_weight_stddev, d_bias_mean,
                  d_bias_stddev, M, K, N};
        RLX_LAUNCH((noisy_dw_kernel), dim3((N + 31) / 32, (K + 127) / 128), 256, 0, s, q);
        RLX_LAUNCH_CHECK();
    }
    if (dx) {
        NoisyProd p{};
        p.a = dz; p.lda = lddz; p.wm = weight_mean; p.ws = weight_stddev; p.ldw = N;
        p.rscale = noise + K; p.oscale = noise;
        p.aux = lower_activation ? x : nullptr; p.ld_aux = ldx; p.deriv = lower_activation;
        p.out = dx; p.ldo = lddx; p.M = M; p.R = N; p.J = K;
        return launch_prod(p, true, workspace, workspace_floats, "rlx_noisy_dense_backward", s);
    }
    return RLX_OK;
}

}  // extern "C"
