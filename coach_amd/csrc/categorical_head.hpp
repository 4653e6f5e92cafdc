// What the categorical heads (c51.hip, rainbow.hip) share on the device: the ONE softmax over an action's atoms, the fp64
// expectation, the projection of a shifted support onto the atoms and the body of the acting kernels.  A head that first
// merges two streams (rainbow.hip) does so with dfp_merge.hpp and then runs exactly this arithmetic on the merged logits,
// so for equal logits both heads give equal bits.
//
//   softmax:     mx = max_j x_j;  e_j = (float)exp((double)(x_j - mx));  s = sum_{j = 0 .. N-1, in this order} e_j (fp32);
//                p_j = e_j / s
//   expectation: q = sum_{j ascending} (double)p_j * z_j (fp64)
//   projection:  tz_j = fmax(fmin(shift + scale * z_j, z_{N-1}), z_0), bj = (tz_j - z_0) / (z_1 - z_0), l = floor(bj),
//                u = ceil(bj); m[l] += p_j (u - bj), m[u] += p_j (bj - l) for j ascending, the l-term then the u-term
// Needs -ffp-contract=off in the file that includes it (the fp64 arithmetic rounds like numpy).
#pragma once
#include "dfp_merge.hpp"
#include "distributional_head.hpp"

namespace rlx {

constexpr int kCatMaxAtoms = kDistLossThreads;   // one thread per atom in the loss kernels
constexpr int kCatMaxActions = kDistMaxActions;

// Softmax of `rows` rows of N values held in LDS, in place.  mx[r] / sum[r] keep each row's maximum and fp32 sum of
// exponentials.  The serial parts (maximum, sum in atom order) are one thread per row; the exponentials and the
// divisions are spread over the workgroup.  Ends with a barrier.
template <int THREADS>
__device__ __forceinline__ void softmax_rows(float *x, float *mx, float *sum, int rows, int N, int t) {
    if (t < rows) {
        const float *r = x + t * N;
        float m = r[0];
        for (int j = 1; j < N; ++j) m = fmaxf(m, r[j]);
        mx[t] = m;
    }
    __syncthreads();
    for (int c = t; c < rows * N; c += THREADS) x[c] = (float)exp((double)(x[c] - mx[c / N]));
    __syncthreads();
    if (t < rows) {
        const float *r = x + t * N;
        float s = 0.f;
        for (int j = 0; j < N; ++j) s += r[j];
        sum[t] = s;
    }
    __syncthreads();
    for (int c = t; c < rows * N; c += THREADS) x[c] = x[c] / sum[c / N];
    __syncthreads();
}

__device__ __forceinline__ double expectation(const float *p, const double *z, int N) {
    double q = 0.0;
    for (int j = 0; j < N; ++j) q += (double)p[j] * z[j];
    return q;
}

// The projection, first half: thread j (< N) forms atom j's two contributions from its probability p.  The caller
// synchronises before project_gather.
__device__ __forceinline__ void project_scatter(const double *z_s, int N, int j, double shift, double scale, double p,
                                                int *l_s, int *u_s, double *wl_s, double *wu_s) {
    const double z0 = z_s[0], zl = z_s[N - 1];
    const double tz = fmax(fmin(shift + scale * z_s[j], zl), z0);
    const double bj = (tz - z0) / (z_s[1] - z0);
    const double lo = floor(bj), up = ceil(bj);
    l_s[j] = (int)lo;
    u_s[j] = (int)up;
    wl_s[j] = p * (up - bj);      // both are 0 when bj is an integer: that atom's mass is dropped, as in the reference
    wu_s[j] = p * (bj - lo);
}

// Second half: thread k, which owns output atom k, adds the contributions in the reference's order: j ascending, the
// l-term then the u-term.  No atomics: the sum is bit-identical to the Python loop.
// On a support whose (z_{N-1} - z_0) / (z_1 - z_0) rounds above N - 1 (linspace(-10, 10, 256); not the default 51
// atoms) an atom clipped at v_max has u == N, where the reference raises IndexError: no thread owns that atom, so
// the contribution (weight bj - l, a rounding error) is left out and nothing is written out of bounds.
__device__ __forceinline__ double project_gather(int N, int k, const int *l_s, const int *u_s, const double *wl_s,
                                                 const double *wu_s) {
    double acc = 0.0;
    for (int j = 0; j < N; ++j) {
        if (l_s[j] == k) acc += wl_s[j];
        if (u_s[j] == k) acc += wu_s[j];
    }
    return acc;
}

// The acting kernels' body, one wave per env: the softmax of each action's logits in LDS, lanes a < A form the fp64
// expectations (-> q, LDS, and q_out where given).  MERGE: the logits are the dueling merge of v [N] and x [A][N]
// (dfp_merge.hpp); otherwise x is the head's output itself and v is not read.  Ends with a barrier.
template <bool MERGE>
__device__ __forceinline__ void categorical_act_q(const float *__restrict__ v, const float *__restrict__ x,
                                                  const double *__restrict__ z, int N, int A, int e, int t,
                                                  double *__restrict__ q_out, double *q) {
    __shared__ float p_s[kCatMaxActions * kCatMaxAtoms];
    __shared__ double z_s[kCatMaxAtoms];
    __shared__ float mx_s[kCatMaxActions], sum_s[kCatMaxActions];
    if (MERGE) {
        dfp_merge_row(v, x, A, N, p_s, t, 64);
    } else {
        for (int c = t; c < A * N; c += 64) p_s[c] = x[c];
    }
    for (int j = t; j < N; j += 64) z_s[j] = z[j];
    __syncthreads();
    softmax_rows<64>(p_s, mx_s, sum_s, A, N, t);
    if (t < A) {
        q[t] = expectation(p_s + t * N, z_s, N);
        if (q_out) q_out[(size_t)e * A + t] = q[t];
    }
    __syncthreads();
}

}  // namespace rlx
