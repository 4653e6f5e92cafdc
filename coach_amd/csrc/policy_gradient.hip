// Vanilla Policy Gradients on gfx950: the update window of one episode and the discrete PolicyHead's loss.
//
// Replaces, in the reference (paths under rl_coach/):
//   * Episode.update_discounted_rewards (n_step = -1)            core_types.py:780-801
//   * PolicyOptimizationAgent.update_episode_statistics          agents/policy_optimization_agent.py:72-83
//   * PolicyGradientsAgent.learn_from_batch's rescaling loop     agents/policy_gradients_agent.py:102-126
//   * PolicyHead, discrete branch (loss, entropy regularisation) architectures/tensorflow_components/heads/policy_head.py:75-100
//   * the 'Entropy' sample of choose_action                      agents/policy_optimization_agent.py:154
//
// These are latency-bound row kernels over tens to hundreds of rows, launched once per update window: each is ONE
// workgroup, so every sum has a fixed order and no float atomics or hand-offs between workgroups are needed.
// tests/pg_ref.py is the numpy restatement; it states every fp32 / fp64 rounding point named here.
// Compiled with -ffp-contract=off so the fp64 arithmetic rounds like numpy.
#include "policy_head.hpp"
#include "episode_returns.hpp"

namespace {

constexpr int kPgThreads = rlx::kPgThreads;
constexpr int kPgMaxActions = rlx::kPgMaxActions;
constexpr int kPgStage = 2048;            // fp64 values staged in LDS for the serial sums (longer windows read HBM)
constexpr float kEps = rlx::kPgEps;

// numpy's pairwise summation of n fp64 values elem(0) .. elem(n-1) (numpy/core/src/umath/loops_utils.h, pairwise_sum),
// as np.add.reduce runs it over a contiguous array: blocks of <= 128 values are summed in eight interleaved accumulators
// combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) plus a serial tail, longer ranges split at n/2 rounded down to a
// multiple of 8.  Run by ONE thread (a window has tens to hundreds of values); the recursion is an explicit stack.
template <typename F>
__device__ double pairwise_block(F elem, int off, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += elem(off + i);
        return res;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = elem(off + j);
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += elem(off + i + j);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += elem(off + i);
    return res;
}

template <typename F>
__device__ double pairwise_sum(F elem, int n) {
    struct Frame { int off, n, phase; double left; };
    Frame st[32];                        // a range halves at every level: 32 levels cover any int length
    int sp = 0;
    double ret = 0.0;
    st[sp++] = Frame{0, n, 0, 0.0};
    while (sp > 0) {
        Frame f = st[sp - 1];
        if (f.n <= 128) {
            ret = pairwise_block(elem, f.off, f.n);
            --sp;
            continue;
        }
        int n2 = f.n / 2;
        n2 -= n2 % 8;
        if (f.phase == 0) {
            st[sp - 1].phase = 1;
            st[sp++] = Frame{f.off, n2, 0, 0.0};
        } else if (f.phase == 1) {
            st[sp - 1].phase = 2;
            st[sp - 1].left = ret;
            st[sp++] = Frame{f.off + n2, f.n - n2, 0, 0.0};
        } else {
            ret = f.left + ret;
            --sp;
        }
    }
    return ret;
}

// np.mean and np.std (ddof 0) of x[0 .. n): mean = sum / n; std = sqrt(sum((x - mean) * (x - mean)) / n).  One thread.
__device__ void mean_std(const double *x, int n, double *mean_out, double *std_out) {
    const double mean = pairwise_sum([x](int i) { return x[i]; }, n) / (double)n;
    const double var = pairwise_sum([x, mean](int i) { const double d = x[i] - mean; return d * d; }, n) / (double)n;
    *mean_out = mean;
    *std_out = sqrt(var);
}

struct WindowArgs {
    const float *rewards;       // [length] the episode's filtered rewards so far
    int length, start;          // the window is episode[start:]
    double discount;
    int rescaler;
    double *mean_over_episodes; // [max_length] mean_return_over_multiple_episodes
    double *episodes_seen;      // [max_length] num_episodes_where_step_has_been_seen
    int max_length;
    double *returns;            // [max_length] out: n_step_discounted_rewards of the whole episode
    double *rescaled;           // [max_length] out: the window's rescaled returns (fp64), entries [0, length - start)
    float *advantages;          // [max_length] out: the same, rounded to fp32 once
    double *stats;              // [4] out: Returns Mean, Returns Variance (np.std), the episode's mean and std (or 0, 0)
    int *status;
};

__global__ void __launch_bounds__(kPgThreads) pg_episode_window_kernel(const WindowArgs a) {
    __shared__ double stage[kPgStage];
    __shared__ double ep_s[2];
    const int t = threadIdx.x, L = a.length, T = a.length - a.start;
    if (L > a.max_length) {          // the per-timestep arrays end at max_length: nothing is read or written
        if (t == 0) atomicOr(a.status, RLX_PG_STATUS_EPISODE_TOO_LONG);
        return;
    }
    const bool normalized = a.rescaler == RLX_PG_FUTURE_RETURN_NORMALIZED_BY_EPISODE ||
                            a.rescaler == RLX_PG_FUTURE_RETURN_NORMALIZED_BY_TIMESTEP;
    const bool staged = L <= kPgStage;
    // update_transitions_rewards_and_bootstrap_data: the returns of the WHOLE episode so far
    for (int i = t; i < L; i += kPgThreads) {
        const double r = rlx::episode_nstep_return(a.rewards, i, L, L, a.discount, [](int k) { return k; });
        a.returns[i] = r;
        if (staged) stage[i] = r;
        // update_episode_statistics, the two-statement form (policy_optimization_agent.py:77-81)
        if (normalized) {
            const double n = a.episodes_seen[i] + 1.0;
            a.episodes_seen[i] = n;
            double m = a.mean_over_episodes[i];
            m -= m / n;
            m += r / n;
            a.mean_over_episodes[i] = m;
        }
    }
    __syncthreads();
    if (t == 0) {
        ep_s[0] = 0.0;
        ep_s[1] = 0.0;
        if (normalized) mean_std(staged ? stage : a.returns, L, &ep_s[0], &ep_s[1]);
        a.stats[2] = ep_s[0];
        a.stats[3] = ep_s[1];
    }
    __syncthreads();
    // the rescaling loop (policy_gradients_agent.py:102-118); i is the position in the BATCH
    const double ep_mean = ep_s[0], ep_std = ep_s[1];
    for (int i = t; i < T; i += kPgThreads) {
        double v = a.returns[a.start + i];
        if (a.rescaler == RLX_PG_TOTAL_RETURN) v = a.returns[a.start];
        else if (a.rescaler == RLX_PG_FUTURE_RETURN_NORMALIZED_BY_EPISODE) v = ep_std != 0.0 ? (v - ep_mean) / ep_std : 0.0;
        else if (a.rescaler == RLX_PG_FUTURE_RETURN_NORMALIZED_BY_TIMESTEP) v -= a.mean_over_episodes[i];
        a.rescaled[i] = v;
        a.advantages[i] = (float)v;
    }
    __syncthreads();
    if (staged)
        for (int i = t; i < T; i += kPgThreads) stage[i] = a.rescaled[i];
    __syncthreads();
    if (t == 0) mean_std(staged ? stage : a.rescaled, T, &a.stats[0], &a.stats[1]);
}

// The row arithmetic of the discrete PolicyHead is policy_head.hpp's (shared with a3c.hip).
struct HeadLossArgs {
    const float *logits;
    long long ld;
    const int *actions;
    const float *advantages;
    float beta;
    int rows, T, A;
    float *dlogits;
    long long ld_d;
    float *scalars;             // [2]: loss, mean entropy
    int *status;
};

// ONE workgroup: thread t owns rows t, t + 256, ...; a thread adds its rows' terms in row order and the workgroup sums
// the 256 partials in a fixed tree.  Rows [T, rows) are padding: zero gradient, no term.
__global__ void __launch_bounds__(kPgThreads) pg_head_loss_kernel(const HeadLossArgs a) {
    __shared__ float pol_s[kPgThreads], ent_s[kPgThreads];
    const int t = threadIdx.x, A = a.A;
    const float fT = (float)a.T;
    float pol = 0.f, ent = 0.f;
    for (int b = t; b < a.rows; b += kPgThreads) {
        float *d = a.dlogits + (size_t)b * a.ld_d;
        const int act = b < a.T ? a.actions[b] : 0;
        const bool valid = b < a.T && rlx::taken_action_valid(act, A, 0, a.status);
        if (!valid) {
            for (int j = 0; j < A; ++j) d[j] = 0.f;
            continue;
        }
        rlx::pg_row_loss_grad(a.logits + (size_t)b * a.ld, A, act, a.advantages[b], a.beta, fT, d, pol, ent);
    }
    pol_s[t] = pol;
    ent_s[t] = ent;
    __syncthreads();
    for (int s = kPgThreads >> 1; s > 0; s >>= 1) {
        if (t < s) {
            pol_s[t] += pol_s[t + s];
            ent_s[t] += ent_s[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        const float mean_h = ent_s[0] / fT;
        a.scalars[0] = -(pol_s[0] / fT) - a.beta * mean_h;
        a.scalars[1] = mean_h;
    }
}

__global__ void action_entropy_kernel(const float *__restrict__ probs, long long ld, int n_env, int A,
                                      float *__restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    const float *p = probs + (size_t)e * ld;
    float s = 0.f;
    for (int j = 0; j < A; ++j) s += p[j] * (float)log((double)(p[j] + kEps));
    out[e] = -s;
}

}  // namespace

extern "C" {

int rlx_pg_episode_window(const float *rewards, int length, int start, double discount, int rescaler,
                          double *mean_over_episodes, double *episodes_seen, int max_length, double *returns_out,
                          double *rescaled_out, float *advantages_out, double *stats_out, int *status, void *stream) {
    RLX_REQUIRE(rewards && mean_over_episodes && episodes_seen && returns_out && rescaled_out && advantages_out &&
                    stats_out && status,
                "rlx_pg_episode_window: null pointer");
    RLX_REQUIRE(max_length >= 1 && length >= 1 && start >= 0 && start < length,
                "rlx_pg_episode_window: bad window (length %d, start %d, max_length %d)", length, start, max_length);
    RLX_REQUIRE(rescaler >= RLX_PG_TOTAL_RETURN && rescaler <= RLX_PG_FUTURE_RETURN_NORMALIZED_BY_TIMESTEP,
                "rlx_pg_episode_window: the policy gradient rescaler %d is not one of the four return rescalers",
                rescaler);
    WindowArgs a{rewards, length, start, discount, rescaler, mean_over_episodes, episodes_seen, max_length, returns_out,
                 rescaled_out, advantages_out, stats_out, status};
    RLX_LAUNCH((pg_episode_window_kernel), 1, kPgThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_pg_head_loss(const float *logits, long long ld, const int *actions, const float *advantages, float beta_entropy,
                     int rows, int true_rows, int n_actions, float *dlogits, long long ld_dlogits, float *scalars,
                     int *status, void *stream) {
    RLX_REQUIRE(logits && actions && advantages && dlogits && scalars && status, "rlx_pg_head_loss: null pointer");
    RLX_REQUIRE(n_actions >= 1 && n_actions <= kPgMaxActions && true_rows >= 1 && rows >= true_rows,
                "rlx_pg_head_loss: unsupported sizes (1 <= actions=%d <= 18, 1 <= true rows=%d <= rows=%d)", n_actions,
                true_rows, rows);
    RLX_REQUIRE(ld >= n_actions && ld_dlogits >= n_actions, "rlx_pg_head_loss: leading dimension < A");
    HeadLossArgs a{logits, ld, actions, advantages, beta_entropy, rows, true_rows, n_actions, dlogits, ld_dlogits,
                   scalars, status};
    RLX_LAUNCH((pg_head_loss_kernel), 1, kPgThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_action_entropy(const float *probs, long long ld, int n_env, int n_actions, float *entropy_out, void *stream) {
    RLX_REQUIRE(probs && entropy_out, "rlx_action_entropy: null pointer");
    RLX_REQUIRE(n_env >= 1 && n_actions >= 1 && ld >= n_actions, "rlx_action_entropy: bad shape");
    RLX_LAUNCH((action_entropy_kernel), (n_env + 63) / 64, 64, 0, rlx::as_stream(stream), probs, ld, n_env, n_actions,
               entropy_out);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
