// Exploration policies that draw from a distribution formed on the device (per env-step, n_env rows):
//
//   * Boltzmann.get_action        boltzmann.py:52-62         softmax(q / T) in numpy's fp32 order, then
//                                                            np.random.choice(p=) on one host uniform per row
//   * TruncatedNormal.get_action  truncated_normal.py:78-112 scipy truncnorm(a, b, loc, scale).rvs as an inverse CDF
//
// Boltzmann — one wave per row, the waves of a workgroup serve different rows.  Lane l keeps actions l, l + 64, .. in
// registers (up to kPerLane of them).  The row passes through LDS where an order is part of the contract: numpy's
// pairwise fp32 sum reads it (eight running sums held by lanes 0..7 of every 8-lane group, joined by three xor
// shuffles, so every lane ends with the same bits), lane 0 forms np.random.choice's fp64 cumulative sum in index order
// — a running fp64 sum of fp32 values is not associative, so that part stays serial: A additions — and all lanes then
// make the divisions by the last entry and count the entries <= u (the right-sided search on a non-decreasing array).
// explore.hip's categorical kernels search with one THREAD per row inside their own loops; there is no function to
// share with a wave-wide count, so the rule (first entry > u of cdf / cdf[-1]) is restated here once.
//
// TruncatedNormal — one thread per element; fp64 ndtr / ndtri from normal_cdf.hpp; the uniform is the host's or
// Philox4x32-10's (philox.hpp) at a draw counter kept in device memory, advanced by the last workgroup to finish.
//
// Compiled with -ffp-contract=off: the fp32 and fp64 steps round one by one, as tests/boltzmann_ref.py writes them.
#include "rlx_common.hpp"
#include "normal_cdf.hpp"
#include "philox.hpp"

namespace {

constexpr int kRowsPerGroup = 4;                                  // waves of a Boltzmann workgroup
constexpr int kPerLane = RLX_BOLTZMANN_MAX_ACTIONS / 64;          // actions a lane holds

// np.add.reduce over n <= 128 contiguous fp32 values (numpy's pairwise_sum below its block size): fewer than 8 values are
// a running sum from 0; else r[j] runs over a[j], a[j + 8], .., the eight are joined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5)
// + (r6 + r7)) and the n % 8 last values are added one by one.  All 64 lanes call it and all get the result: lane l
// runs r[l % 8], and fp32 addition commutes, so the xor butterfly gives every lane the same three additions.
__device__ __noinline__ float np_sum_block(const float *a, int n, int lane) {
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    const int j = lane & 7, m = n - (n & 7);
    float r = a[j];
    for (int i = 8; i < m; i += 8) r += a[i + j];
    r += __shfl_xor(r, 1, 64);
    r += __shfl_xor(r, 2, 64);
    r += __shfl_xor(r, 4, 64);
    for (int i = m; i < n; ++i) r += a[i];
    return r;
}

// above 128 values numpy adds the sums of two parts, the left one n / 2 rounded down to a multiple of 8.  kDepth = 4
// splits reach 128 from RLX_BOLTZMANN_MAX_ACTIONS (the larger part of n is at most n / 2 + 7.5: 1024 -> 520 -> 268 ->
// 142 -> 79).
template <int kDepth>
__device__ __forceinline__ float np_sum(const float *a, int n, int lane) {
    if constexpr (kDepth > 0) {
        if (n > 128) {
            int n2 = n / 2;
            n2 -= n2 % 8;
            const float left = np_sum<kDepth - 1>(a, n2, lane);
            return left + np_sum<kDepth - 1>(a + n2, n - n2, lane);
        }
    }
    return np_sum_block(a, n, lane);
}

__global__ void __launch_bounds__(64 * kRowsPerGroup)
boltzmann_sample_kernel(const float *__restrict__ q, long long ld, const double *__restrict__ u,
                        const double *__restrict__ temperature, int n_env, int A, float *__restrict__ probs_out,
                        long long ld_out, int *__restrict__ actions, int *__restrict__ status) {
    extern __shared__ double lds[];                               // [waves][A] fp64 cumulative sums, then [waves][A] fp32
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * kRowsPerGroup + wave;
    const bool live = row < n_env;                                // a spare wave repeats the last row and stores nothing:
    const int r = live ? row : n_env - 1;                         // every wave reaches every barrier
    double *cdf = lds + (size_t)wave * A;
    float *sf = reinterpret_cast<float *>(lds + (size_t)kRowsPerGroup * A) + (size_t)wave * A;
    const float *qr = q + (size_t)r * ld;
    const float t = (float)*temperature;                          // float32 array / Python float: fp32 division

    float e[kPerLane], p[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
        const int j = lane + 64 * k;
        e[k] = 0.f;
        if (j < A) {
            e[k] = expf(qr[j] / t);
            sf[j] = e[k];
        }
    }
    __syncthreads();
    const float s = np_sum<4>(sf, A, lane);
    __syncthreads();                                              // the sums are read: the row is overwritten
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
        const int j = lane + 64 * k;
        p[k] = e[k] / s;
        if (j < A) sf[j] = p[k];
    }
    __syncthreads();
    const float last = 1.0f - np_sum<4>(sf, A - 1, lane);         // probabilities[-1] = 1 - np.sum(probabilities[:-1])
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
        const int j = lane + 64 * k;
        if (j == A - 1) {
            p[k] = last;
            sf[j] = last;                                         // (np_sum did not read entry A - 1)
        }
        if (j < A) bad = bad || !(p[k] >= 0.f && p[k] <= 3.402823466e+38f);
    }
    bad = __any(bad);                                             // numpy: "probabilities contain NaN" / "are not non-negative"
    __syncthreads();
    if (lane == 0) {                                              // p.astype(float64).cumsum(), in index order
        double c = 0.0;
        for (int j = 0; j < A; ++j) {
            c += (double)sf[j];
            cdf[j] = c;
        }
    }
    __syncthreads();
    const double total = cdf[A - 1], uu = u[r];
    int count = 0;                                                // searchsorted(u, side='right') of cdf / cdf[-1]
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
        const int j = lane + 64 * k;
        if (j < A && cdf[j] / total <= uu) ++count;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) count += __shfl_xor(count, d, 64);
    int action = count < A ? count : A - 1;
    if (bad && lane == 0) {                                       // np.argmax of the row's values (a NaN is the maximum)
        float bv = qr[0];
        action = 0;
        for (int j = 1; j < A; ++j) rlx::np_argmax_step(qr[j], j, bv, action);
        if (live) atomicOr(status, RLX_EXPLORE_STATUS_BAD_PROBABILITIES);
    }
    if (!live) return;
    if (lane == 0) actions[row] = action;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
        const int j = lane + 64 * k;
        if (j < A) probs_out[(size_t)row * ld_out + j] = p[k];
    }
}

__global__ void __launch_bounds__(256)
truncated_normal_kernel(const float *__restrict__ mean, const float *__restrict__ stddev, int std_kind,
                        const float *__restrict__ low, const float *__restrict__ high, const double *__restrict__ uniforms,
                        long long *draw_state, uint32_t seed, uint32_t rank, int n, int D, float *__restrict__ out,
                        double *__restrict__ out64, int *__restrict__ status) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long draw = uniforms ? 0ull : (unsigned long long)*(volatile long long *)draw_state;
    if (i < (unsigned)n) {
        const int d = (int)(i % (unsigned)D);
        const double m = (double)mean[i];
        const double sd = (double)stddev[std_kind == RLX_TN_STD_SCALAR ? 0 : (std_kind == RLX_TN_STD_PER_DIM ? d : (int)i)];
        const double lo = (double)low[d], hi = (double)high[d];
        double x = rlx::np_clip(m, lo, hi);                       // what a refused or vanished window gives
        if (!(sd > 0.0) || !(lo < hi)) {
            atomicOr(status, RLX_EXPLORE_STATUS_BAD_WINDOW);
        } else {
            double uu;
            if (uniforms) {
                uu = uniforms[i];
            } else {
                const rlx::U4 w = rlx::philox4x32_10(i, RLX_TN_STREAM, (uint32_t)draw,
                                                     (uint32_t)(draw >> 32) ^ rlx::kNoiseTag, seed, rank);
                uu = rlx::philox_unit(w.x, w.y);
            }
            const double a = (lo - m) / sd, b = (hi - m) / sd;
            double mass, z;
            if (a > 0.0) {                                        // the window lies right of the centre: upper tail
                const double qa = rlx::ndtr_upper(a), qb = rlx::ndtr_upper(b);
                mass = qa - qb;
                z = -rlx::ndtri(qa - uu * mass);
            } else {
                const double ca = rlx::ndtr(a), cb = rlx::ndtr(b);
                mass = cb - ca;
                z = rlx::ndtri(ca + uu * mass);
            }
            if (mass > 0.0) {
                x = m + sd * z;
                x = x > lo ? x : lo;                              // the last-ulp overshoot, and ndtri's +-inf at u = 0 / 1
                x = x < hi ? x : hi;
            }
        }
        out[i] = (float)x;                                        // low / high are fp32: the rounded value stays inside
        if (out64) out64[i] = x;
    }
    if (uniforms) return;
    __syncthreads();                                              // every thread of the workgroup has read the counter
    if (threadIdx.x == 0) {
        unsigned long long *ticket = reinterpret_cast<unsigned long long *>(draw_state + 1);
        __threadfence();
        if (atomicAdd(ticket, 1ull) == (unsigned long long)gridDim.x - 1ull) {     // the last workgroup to get here
            *ticket = 0ull;
            draw_state[0] = (long long)(draw + 1ull);
        }
    }
}

}  // namespace

extern "C" {

int rlx_boltzmann_sample(const float *q_values, long long ld, const double *uniforms, const double *temperature,
                         int n_env, int n_actions, float *probs_out, long long ld_out, int *actions, int *status,
                         void *stream) {
    RLX_REQUIRE(q_values && uniforms && temperature && probs_out && actions && status, "rlx_boltzmann_sample: null pointer");
    RLX_REQUIRE(n_env > 0 && n_actions > 0 && ld >= n_actions && ld_out >= n_actions, "rlx_boltzmann_sample: bad shape");
    RLX_REQUIRE(n_actions <= RLX_BOLTZMANN_MAX_ACTIONS, "rlx_boltzmann_sample: at most %d actions (got %d)",
                RLX_BOLTZMANN_MAX_ACTIONS, n_actions);
    const unsigned lds = (unsigned)(kRowsPerGroup * n_actions * (sizeof(double) + sizeof(float)));    // <= 48 KB
    RLX_LAUNCH((boltzmann_sample_kernel), (n_env + kRowsPerGroup - 1) / kRowsPerGroup, 64 * kRowsPerGroup, lds,
               rlx::as_stream(stream), q_values, ld, uniforms, temperature, n_env, n_actions, probs_out, ld_out, actions,
               status);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_truncated_normal_sample(const float *mean, const float *stddev, int std_kind, const float *clip_low,
                                const float *clip_high, const double *uniforms, long long *draw_state,
                                unsigned int seed, unsigned int rank, int n_env, int action_dim, float *actions,
                                double *actions_f64, int *status, void *stream) {
    RLX_REQUIRE(mean && stddev && clip_low && clip_high && actions && status, "rlx_truncated_normal_sample: null pointer");
    RLX_REQUIRE(uniforms || draw_state, "rlx_truncated_normal_sample: give the uniforms or the device draw counter");
    RLX_REQUIRE(std_kind == RLX_TN_STD_SCALAR || std_kind == RLX_TN_STD_PER_DIM || std_kind == RLX_TN_STD_PER_ELEMENT,
                "rlx_truncated_normal_sample: bad std_kind %d", std_kind);
    RLX_REQUIRE(n_env > 0 && action_dim > 0 && (long long)n_env * action_dim <= 0x7FFFFFFFLL,
                "rlx_truncated_normal_sample: bad shape");
    const int n = n_env * action_dim;
    RLX_LAUNCH((truncated_normal_kernel), (n + 255) / 256, 256, 0, rlx::as_stream(stream), mean, stddev, std_kind, clip_low,
               clip_high, uniforms, draw_state, (uint32_t)seed, (uint32_t)rank, n, action_dim, actions, actions_f64, status);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
