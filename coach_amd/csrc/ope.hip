// Off-policy evaluation of a Q network's softmax policy on the evaluation set of a Batch RL dataset, on gfx950:
// inverse propensity score (IPS), direct method (DM), doubly robust (DR), sequential doubly robust and weighted
// importance sampling (WIS), and the behaviour probabilities that are stored while the dataset is collected.
//
// Replaces, in the reference (paths under rl_coach/):
//   * OpeManager._prepare_ope_shared_stats / evaluate        off_policy_evaluators/ope_manager.py:49-151
//     (a Batch per 128 rows, one update_info per transition)
//   * DoublyRobust.evaluate                                   off_policy_evaluators/bandits/doubly_robust.py:34-38
//   * SequentialDoublyRobust.evaluate                         off_policy_evaluators/rl/sequential_doubly_robust.py:40-51
//   * WeightedImportanceSampling.evaluate                     off_policy_evaluators/rl/weighted_importance_sampling.py:41-55
//     (two nested Python loops over episodes and transitions each)
//   * QHead's softmax output                                  architectures/tensorflow_components/heads/q_head.py:56-68
//   * what ValueOptimizationAgent.choose_action stores as all_action_probabilities   agents/value_optimization_agent.py:98-102
//
// The arithmetic is stated once, in include/rlx.h, and restated in numpy by tests/ope_ref.py.  The softmax is fp32 and
// shared by the acting side and the evaluation side (softmax_row below); everything behind it is fp64 computed from the
// fp32 values widened once.  This file is compiled with -ffp-contract=off, so that a product and the sum it feeds round
// separately as they do in numpy.
//
// rlx_ope_rows: one lane per evaluation row, a loop over the A <= 18 actions.
// rlx_ope_reduce: the sequential doubly robust recurrence acc_j = A_j + B_j * acc_{j+1} is a composition of affine maps
// (the pattern of returns.hip's reverse scan, kept here as a copy), and only the composed map of a whole episode is
// needed: one wave per episode reduces 64 rows per pass with an ordered shuffle tree and folds the passes in row order;
// the product of the importance ratios rides in the same tree.  A second launch of one workgroup sums the three per-row
// columns and the three per-episode columns in a fixed-shape fp64 tree and writes the five estimates.  No floating-point
// atomics anywhere: the same bits on every call.
#include "rlx_common.hpp"

namespace {

constexpr int kMaxActions = RLX_OPE_MAX_ACTIONS;
constexpr int kRowThreads = 256;
constexpr int kEpisodeThreads = 256;                     // 4 waves: 4 episodes per workgroup
constexpr int kSumThreads = 1024;

// softmax(q / T) of one row in fp32 (heads/q_head.py:56-68): z = q / T, minus the row maximum, expf, the sum in action
// order, one division per entry.  out may alias nothing of q.
__device__ __forceinline__ void softmax_row(const float *__restrict__ q, int A, float T, float *__restrict__ out) {
    float z[kMaxActions];
    float m = -INFINITY;
    for (int k = 0; k < A; ++k) {
        z[k] = q[k] / T;
        m = z[k] > m ? z[k] : m;
    }
    float s = 0.f;
    for (int k = 0; k < A; ++k) {
        z[k] = expf(z[k] - m);
        s = s + z[k];
    }
    for (int k = 0; k < A; ++k) out[k] = z[k] / s;
}

__global__ void __launch_bounds__(64)
behaviour_probabilities_kernel(const float *__restrict__ q, long long ld_q, const double *__restrict__ explore_u,
                               double epsilon, int force_uniform, float T, int n_env, int A,
                               float *__restrict__ out, long long ld_out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    float *o = out + (size_t)e * (size_t)ld_out;
    if (force_uniform || explore_u[e] < epsilon) {           // the comparison of rlx_egreedy on the same draw
        const float p = 1.0f / (float)A;
        for (int k = 0; k < A; ++k) o[k] = p;
        return;
    }
    softmax_row(q + (size_t)e * (size_t)ld_q, A, T, o);
}

struct RowsArgs {
    const float *q; long long ld_q;
    const float *rm; long long ld_rm; long long divisor;
    const int *actions; const float *rewards;
    const float *mu; long long ld_mu;
    float T; long long n; int A;
    float *pi; long long ld_pi;
    double *cols;                                            // [RLX_OPE_ROW_COLUMNS][n]
    int *status;
};

__global__ void __launch_bounds__(kRowThreads) ope_rows_kernel(const RowsArgs a) {
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < a.n; j += (long long)gridDim.x * blockDim.x) {
        const int A = a.A;
        const float *q = a.q + (size_t)j * (size_t)a.ld_q;
        float *pi = a.pi + (size_t)j * (size_t)a.ld_pi;
        softmax_row(q, A, a.T, pi);
        const float *rm_dm = a.rm + (size_t)(j / a.divisor) * (size_t)a.ld_rm;     // i(j) = j / d <= j < n
        double v = 0.0, dm = 0.0;
        for (int k = 0; k < A; ++k) {
            const double p = (double)pi[k];
            v = v + p * (double)q[k];
            dm = dm + p * (double)rm_dm[k];
        }
        const int act = a.actions[j];
        double rho = 0.0, qa = 0.0, ips = 0.0, dr = 0.0;
        if (act < 0 || act >= A) {                           // the row contributes zero terms
            atomicOr(a.status, 1);
            v = 0.0;
            dm = 0.0;
        } else {
            const double r = (double)a.rewards[j];
            rho = (double)pi[act] / (double)a.mu[(size_t)j * (size_t)a.ld_mu + act];   // IEEE: inf or NaN where mu is 0
            qa = (double)q[act];
            ips = rho * r;
            dr = rho * (r - (double)a.rm[(size_t)j * (size_t)a.ld_rm + act]);
        }
        a.cols[RLX_OPE_COL_RHO * a.n + j] = rho;
        a.cols[RLX_OPE_COL_V * a.n + j] = v;
        a.cols[RLX_OPE_COL_Q_TAKEN * a.n + j] = qa;
        a.cols[RLX_OPE_COL_IPS * a.n + j] = ips;
        a.cols[RLX_OPE_COL_DM * a.n + j] = dm;
        a.cols[RLX_OPE_COL_DR * a.n + j] = dr;
    }
}

struct Affine {
    double a, b;   // x -> b + a * x
};

// later ∘ earlier  (apply `earlier` first)
__device__ __forceinline__ Affine compose(const Affine later, const Affine earlier) {
    Affine r;
    r.a = later.a * earlier.a;
    r.b = later.b + later.a * earlier.b;
    return r;
}

// One wave per episode.  Row j's map x -> A_j + B_j x is applied AFTER row j + 1's, so the episode's map is
// f_first ∘ f_first+1 ∘ ... ∘ f_last and the estimate is its value at 0.  A pass reduces 64 consecutive rows with an
// ordered tree (lane i takes lane i + d as the EARLIER map; lanes past the end hold the identity), lane 0 folds the
// passes in row order.  The product of rho takes the same tree.
__global__ void __launch_bounds__(kEpisodeThreads)
ope_episodes_kernel(const int *__restrict__ offsets, int E, long long n, const double *__restrict__ cols,
                    const float *__restrict__ rewards, const double *__restrict__ returns, double gamma,
                    double *__restrict__ ep_out) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * (kEpisodeThreads / 64) + (threadIdx.x >> 6);
    if (e >= E) return;                                      // uniform over the wave; no workgroup barrier below
    long long beg = offsets[e], end = offsets[e + 1];
    if (beg < 0) beg = 0;
    if (end > n) end = n;                                    // a bad table cannot make the launch read past the rows
    const double *rho_c = cols + RLX_OPE_COL_RHO * n, *v_c = cols + RLX_OPE_COL_V * n;
    const double *qa_c = cols + RLX_OPE_COL_Q_TAKEN * n;
    Affine total{1.0, 0.0};
    double w = 1.0;
    for (long long t0 = beg; t0 < end; t0 += 64) {
        const long long j = t0 + lane;
        Affine f{1.0, 0.0};
        double p = 1.0;
        if (j < end) {
            const double rho = rho_c[j];
            f.a = gamma * rho;
            f.b = v_c[j] + rho * ((double)rewards[j] - qa_c[j]);
            p = rho;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double oa = __shfl_down(f.a, d, 64), ob = __shfl_down(f.b, d, 64), op = __shfl_down(p, d, 64);
            if (j + d < end) {                               // (a lane past the end takes no part: no inf * 0 from padding)
                f = compose(f, Affine{oa, ob});
                p = p * op;
            }
        }
        total = compose(total, f);                           // meaningful in lane 0
        w = w * p;
    }
    if (lane == 0) {
        ep_out[RLX_OPE_EP_SEQ_DR * (long long)E + e] = total.b;
        ep_out[RLX_OPE_EP_W * (long long)E + e] = w;
        ep_out[RLX_OPE_EP_WR * (long long)E + e] = beg < end ? w * returns[beg] : 0.0;
    }
}

__device__ __forceinline__ double block_sum(const double *__restrict__ x, long long n, double *red) {
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long i = tid; i < n; i += kSumThreads) s = s + x[i];
    red[tid] = s;
    __syncthreads();
    for (int d = kSumThreads >> 1; d > 0; d >>= 1) {
        if (tid < d) red[tid] = red[tid] + red[tid + d];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kSumThreads)
ope_sums_kernel(int E, long long n, const double *__restrict__ cols, const double *__restrict__ ep_out,
                double *__restrict__ out) {
    __shared__ double red[kSumThreads];
    const double ips = block_sum(cols + RLX_OPE_COL_IPS * n, n, red);
    const double dm = block_sum(cols + RLX_OPE_COL_DM * n, n, red);
    const double dr = block_sum(cols + RLX_OPE_COL_DR * n, n, red);
    const double seq = block_sum(ep_out + RLX_OPE_EP_SEQ_DR * (long long)E, E, red);
    const double sw = block_sum(ep_out + RLX_OPE_EP_W * (long long)E, E, red);
    const double swr = block_sum(ep_out + RLX_OPE_EP_WR * (long long)E, E, red);
    if (threadIdx.x == 0) {
        const double direct = dm / (double)n;
        out[0] = ips / (double)n;
        out[1] = direct;
        out[2] = dr / (double)n + direct;
        out[3] = seq / (double)E;
        out[4] = sw != 0.0 ? swr / sw : 0.0;                 // weighted_importance_sampling.py:50-55
        out[5] = sw;
        out[6] = (double)E;
    }
}

}  // namespace

extern "C" {

int rlx_behaviour_probabilities(const float *q_values, long long ld_q, const double *explore_uniforms, double epsilon,
                                int force_uniform, double temperature, int n_env, int n_actions, float *probs_out,
                                long long ld_out, void *stream) {
    RLX_REQUIRE(probs_out && (force_uniform || (q_values && explore_uniforms)), "rlx_behaviour_probabilities: null pointer");
    RLX_REQUIRE(n_env > 0 && n_actions >= 1 && n_actions <= kMaxActions,
                "rlx_behaviour_probabilities: bad sizes (n_env=%d, 1 <= actions=%d <= %d)", n_env, n_actions, kMaxActions);
    RLX_REQUIRE(ld_out >= n_actions && (force_uniform || ld_q >= n_actions),
                "rlx_behaviour_probabilities: leading dimension < actions (%d)", n_actions);
    RLX_LAUNCH((behaviour_probabilities_kernel), (n_env + 63) / 64, 64, 0, rlx::as_stream(stream), q_values, ld_q,
               explore_uniforms, epsilon, force_uniform, (float)temperature, n_env, n_actions, probs_out, ld_out);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_ope_rows(const float *q_values, long long ld_q, const float *reward_model, long long ld_rm,
                 long long dm_row_divisor, const int *actions, const float *rewards, const float *behaviour_probs,
                 long long ld_mu, double temperature, long long n_rows, int n_actions, float *pi_out, long long ld_pi,
                 double *row_columns, int *status, void *stream) {
    RLX_REQUIRE(q_values && reward_model && actions && rewards && behaviour_probs && pi_out && row_columns && status,
                "rlx_ope_rows: null pointer");
    RLX_REQUIRE(n_rows > 0 && n_actions >= 1 && n_actions <= kMaxActions,
                "rlx_ope_rows: bad sizes (rows=%lld, 1 <= actions=%d <= %d)", n_rows, n_actions, kMaxActions);
    RLX_REQUIRE(dm_row_divisor >= 1, "rlx_ope_rows: dm_row_divisor %lld < 1", dm_row_divisor);
    RLX_REQUIRE(ld_q >= n_actions && ld_rm >= n_actions && ld_mu >= n_actions && ld_pi >= n_actions,
                "rlx_ope_rows: leading dimension < actions (%d)", n_actions);
    RowsArgs a;
    a.q = q_values; a.ld_q = ld_q; a.rm = reward_model; a.ld_rm = ld_rm; a.divisor = dm_row_divisor;
    a.actions = actions; a.rewards = rewards; a.mu = behaviour_probs; a.ld_mu = ld_mu;
    a.T = (float)temperature; a.n = n_rows; a.A = n_actions; a.pi = pi_out; a.ld_pi = ld_pi;
    a.cols = row_columns; a.status = status;
    RLX_LAUNCH((ope_rows_kernel), rlx::grid_for(n_rows, kRowThreads), kRowThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_ope_reduce(const int *episode_offsets, int n_episodes, long long n_rows, const double *row_columns,
                   const float *rewards, const double *returns, double discount, double *episode_columns, double *out,
                   void *stream) {
    RLX_REQUIRE(episode_offsets && row_columns && rewards && returns && episode_columns && out,
                "rlx_ope_reduce: null pointer");
    RLX_REQUIRE(n_episodes > 0 && n_rows > 0, "rlx_ope_reduce: bad sizes (episodes=%d, rows=%lld)", n_episodes, n_rows);
    hipStream_t s = rlx::as_stream(stream);
    const int per_block = kEpisodeThreads / 64;
    RLX_LAUNCH((ope_episodes_kernel), (n_episodes + per_block - 1) / per_block, kEpisodeThreads, 0, s, episode_offsets,
               n_episodes, n_rows, row_columns, rewards, returns, discount, episode_columns);
    RLX_LAUNCH_CHECK();
    RLX_LAUNCH((ope_sums_kernel), 1, kSumThreads, 0, s, n_episodes, n_rows, row_columns, episode_columns, out);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
