// The row arithmetic of the continuous PolicyHead (architectures/tensorflow_components/heads/policy_head.py:102-146: a
// bounded mean stream, a softplus standard-deviation stream under ContinuousEntropyParameters or a given std, and
// MultivariateNormalDiag's log_prob and entropy at :75-87), shared by rlx_pg_continuous_head_loss
// (policy_gradient.hip), rlx_a3c_continuous_window_loss (a3c.hip) and rlx_gaussian_policy_forward: one definition, so
// the launches give the same bits for the same pre-activations, action and advantage, and acting sees the mean and std
// the loss kernels use.  Needs -ffp-contract=off (no fused multiply-add) in the file that includes it.
//
// All fp32; a transcendental is taken in fp64 on the fp32 argument and rounded once, as policy_head.hpp does.  Per row,
// D dimensions, sums over j in index order from 0.f:
//   mu_j    = c_j * tanh(m_j)  (bounded: scale c given)        mu_j = m_j  (unbounded: the scale is not read)
//   sigma_j = (max(s_j, 0) + log1p(exp(-|s_j|))) + eps  (learned)          sigma_j = std_j  (given)
//   u_j     = (a_j - mu_j) / sigma_j
//   log pi  = (-1/2 sum u_j^2 - sum log sigma_j) - D/2 log(2 pi)
//   H       = D/2 (1 + log(2 pi)) + sum log sigma_j
// and, for the row's terms -(1/T) log pi adv - (beta/T) H of a window of T rows,
//   dL/dm_j = -(adv/T) (u_j / sigma_j) * dmu_j/dm_j,             dmu/dm = c_j (1 - tanh^2 m_j)  or 1
//   dL/ds_j = (-(adv/T) (u_j^2 - 1) / sigma_j - (beta/T) / sigma_j) * sigmoid(s_j)              (learned std only)
//
// How a launch moves the data (gaussian_head_chunk): ONE workgroup of kPgThreads walks the rows in chunks of 256.  A
// row's operands are up to 3 D floats in row-major buffers, so a thread-per-row read from memory would be strided by
// the leading dimension; instead the chunk's m, s and a are staged into three LDS tiles by loads that run along the
// rows' elements (consecutive lanes, consecutive words of a row), each thread then works on ONE row out of LDS and
// leaves dL/dm and dL/ds in the m and s tiles, and the tiles go back to memory the way they came.  The tiles' row
// stride is D rounded up to an odd number of words (D + 1 for an even D): consecutive lanes' rows then start in
// different banks.  Columns [D, ld) of a buffer are neither read nor written.
#pragma once
#include "policy_head.hpp"

namespace rlx {

constexpr int kGaussMaxDim = 32;
constexpr int kGaussChunk = kPgThreads;                  // rows staged at a time, one per thread
constexpr float kLog2Pi = 1.8378770664093453f;           // log(2 pi), rounded to fp32 once

__host__ __device__ inline int gaussian_tile_stride(int D) { return D | 1; }
// the dynamic LDS of a launch that calls gaussian_head_chunk: the m, s and a tiles
inline size_t gaussian_tiles_bytes(int D) { return (size_t)3 * kGaussChunk * gaussian_tile_stride(D) * sizeof(float); }

struct GaussianHead {
    const float *mean_pre;      // [rows][ld_m]
    long long ld_m;
    const float *std_pre;       // [rows][ld_s], or NULL: the std is `std`
    long long ld_s;
    const float *std;           // [D], read when std_pre is NULL
    const float *scale;         // [D], or NULL: unbounded
    const float *actions;       // [T][D]
    int D;
    float *dmean_pre;           // [rows][ld_dm]
    long long ld_dm;
    float *dstd_pre;            // [rows][ld_ds], written when std_pre is given
    long long ld_ds;
};

// mu_j and dmu_j/dm_j
__device__ __forceinline__ float gaussian_mean(float m, const float *scale, int j, float &dmu_dm) {
    if (!scale) {
        dmu_dm = 1.f;
        return m;
    }
    const float th = (float)tanh((double)m), c = scale[j];
    dmu_dm = c * (1.f - th * th);
    return c * th;
}

// softplus in its overflow-safe form, + eps
__device__ __forceinline__ float gaussian_std(float s) {
    return (fmaxf(s, 0.f) + (float)log1p(exp(-(double)fabsf(s)))) + kPgEps;
}

__device__ __forceinline__ float sigmoidf_exact(float s) { return (float)(1.0 / (1.0 + exp(-(double)s))); }

// One valid row out of the tiles: m / s / a point at the row's D words; adds log pi * adv onto pol and H onto ent and
// overwrites m with dL/dm and (learned std) s with dL/ds.
__device__ __forceinline__ void gaussian_row_loss_grad(const GaussianHead &h, float *m, float *s, const float *a,
                                                       float adv, float beta, float fT, float &pol, float &ent) {
    const int D = h.D;
    const bool learned = h.std_pre != nullptr;
    const float cp = adv / fT, ce = beta / fT;
    float sq = 0.f, ls = 0.f;
    for (int j = 0; j < D; ++j) {
        float dmu_dm;
        const float mu = gaussian_mean(m[j], h.scale, j, dmu_dm);
        const float sigma = learned ? gaussian_std(s[j]) : h.std[j];
        const float u = (a[j] - mu) / sigma;
        sq += u * u;
        ls += (float)log((double)sigma);
        m[j] = -(cp * (u / sigma)) * dmu_dm;
        if (learned) s[j] = (-(cp * ((u * u - 1.f) / sigma)) - ce / sigma) * sigmoidf_exact(s[j]);
    }
    const float hD = 0.5f * (float)D;
    pol += ((-0.5f * sq - ls) - hD * kLog2Pi) * adv;
    ent += hD * (1.f + kLog2Pi) + ls;
}

// Rows [r0, r0 + 256) of a launch over `rows` rows of which the first T are the window's (the others: zero gradient,
// no term).  adv_of(b) is row b's fp32 advantage.  Every thread of the workgroup calls it (barriers inside); `tiles` is
// gaussian_tiles_bytes(D) of LDS, free again when it returns.
template <typename Adv>
__device__ __forceinline__ void gaussian_head_chunk(const GaussianHead &h, float *tiles, int r0, int rows, int T,
                                                    float beta, float fT, Adv adv_of, float &pol, float &ent) {
    const int t = threadIdx.x, D = h.D, S = gaussian_tile_stride(D);
    float *m_t = tiles, *s_t = tiles + kGaussChunk * S, *a_t = tiles + 2 * kGaussChunk * S;
    const int n = min(rows - r0, kGaussChunk);           // rows of this chunk,
    const int nt = max(min(T - r0, n), 0);               // of which the window's
    const bool learned = h.std_pre != nullptr;
    for (int e = t; e < nt * D; e += kPgThreads) {
        const int r = e / D, j = e - r * D;
        const size_t b = (size_t)(r0 + r);
        m_t[r * S + j] = h.mean_pre[b * h.ld_m + j];
        if (learned) s_t[r * S + j] = h.std_pre[b * h.ld_s + j];
        a_t[r * S + j] = h.actions[b * D + j];
    }
    __syncthreads();
    if (t < nt) gaussian_row_loss_grad(h, m_t + t * S, s_t + t * S, a_t + t * S, adv_of(r0 + t), beta, fT, pol, ent);
    __syncthreads();
    for (int e = t; e < n * D; e += kPgThreads) {
        const int r = e / D, j = e - r * D;
        const size_t b = (size_t)(r0 + r);
        h.dmean_pre[b * h.ld_dm + j] = r < nt ? m_t[r * S + j] : 0.f;
        if (learned) h.dstd_pre[b * h.ld_ds + j] = r < nt ? s_t[r * S + j] : 0.f;
    }
    __syncthreads();
}

// Host: the checks the two loss entry points share.
inline int check_gaussian_head(const char *fn, const GaussianHead &h) {
    RLX_REQUIRE(h.mean_pre && h.actions && h.dmean_pre && (h.std_pre ? h.dstd_pre != nullptr : h.std != nullptr),
                "%s: null pointer", fn);
    RLX_REQUIRE(h.D >= 1 && h.D <= kGaussMaxDim, "%s: unsupported action dimension (1 <= D=%d <= %d)", fn, h.D,
                kGaussMaxDim);
    RLX_REQUIRE(h.ld_m >= h.D && h.ld_dm >= h.D && (!h.std_pre || (h.ld_s >= h.D && h.ld_ds >= h.D)),
                "%s: leading dimension < D", fn);
    return RLX_OK;
}

}  // namespace rlx
