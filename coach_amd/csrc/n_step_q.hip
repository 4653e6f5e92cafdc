// N-step Q on gfx950: everything between the forward and the backward pass of one update window, one launch.
//
// Replaces, in the reference (paths under rl_coach/):
//   * NStepQAgent.learn_from_batch's targets ('N-Step', '1-Step')       agents/n_step_q_agent.py:99-140
//   * QHead's loss (MSE, or Huber under replace_mse_with_huber_loss)    .../heads/head.py:143-186 (losses_body.hpp)
//     (... = architectures/tensorflow_components)
//
// A latency-bound row kernel over a few to a few hundred rows: ONE workgroup, so the reverse recurrence has the
// reference's order, the batch sum has a fixed order and there are no float atomics.  The target network's Q values do
// not leave the device: a window is forward (online and target), this launch, backward.  tests/n_step_q_ref.py is the
// numpy restatement; it states every fp32 / fp64 rounding point named here.  Compiled with -ffp-contract=off so the
// fp64 arithmetic rounds like numpy.
#include "distributional_head.hpp"
#include "losses_body.hpp"

namespace {

constexpr int kThreads = 256;

struct NStepQArgs {
    const float *q_online;          // [T][ld_q]
    long long ld_q;
    const float *q_target;          // [rows_t][ld_t]: the TARGET network's rows
    long long ld_t;
    int rows_t;
    const int *actions;             // [T]
    const float *rewards;           // [T]
    const unsigned char *game_over; // the last transition's flag
    int T, A;
    double discount;
    int horizon, huber;
    float *targets;                 // [T] out (in with RLX_NSTEPQ_TARGETS_GIVEN)
    float *td_targets;              // [T][ld_tt] or null
    long long ld_tt;
    float *dq;                      // [T][ld_dq]
    long long ld_dq;
    float *scalars;                 // [1]: the loss
    int *status;
};

__device__ __forceinline__ float row_max(const float *q, int A) {
    float mx = q[0];
    for (int j = 1; j < A; ++j) mx = fmaxf(mx, q[j]);
    return mx;
}

__global__ void __launch_bounds__(kThreads) nstep_q_window_loss_kernel(const NStepQArgs a) {
    __shared__ double r_s[kThreads];    // a chunk of the window: the recurrence's rewards, overwritten by its results
    __shared__ float sum_s[kThreads];
    const int t = threadIdx.x, T = a.T, A = a.A;
    // RLX_NSTEPQ_TARGETS_GIVEN: targets already holds the window's values and no target row is read
    const bool given = a.horizon == RLX_NSTEPQ_TARGETS_GIVEN, n_step = a.horizon == RLX_NSTEPQ_N_STEP;
    const bool terminal = !given && *a.game_over != 0;
    if (!given && (n_step ? (!terminal && a.rows_t < 1) : a.rows_t < T)) {   // nothing is read or written
        if (t == 0) atomicOr(a.status, RLX_NSTEPQ_STATUS_NO_TARGET_ROWS);
        return;
    }
    if (n_step) {
        // lane 0's carried product discount * R, across chunks.  :124, first pass: an fp32 product of fp32(discount)
        // and the fp32 maximum; R is fp64 from the first sum on (n_step_q_ref.py)
        double p = terminal ? 0.0 : (double)((float)a.discount * row_max(a.q_target, A));
        for (int c = (T + kThreads - 1) / kThreads - 1; c >= 0; --c) {
            const int i = c * kThreads + t;
            if (i < T) r_s[t] = (double)a.rewards[i];
            __syncthreads();
            if (t == 0) {                                              // the sequential recurrence, the reference's order
                const int hi = min(T - c * kThreads, kThreads);
                for (int k = hi - 1; k >= 0; --k) {
                    const double R = r_s[k] + p;                       // R = r_i + discount * R
                    p = a.discount * R;
                    r_s[k] = R;
                }
            }
            __syncthreads();
            // :125, the assignment into the fp32 prediction: the one rounding (a row without a valid action keeps its entry)
            if (i < T && a.actions[i] >= 0 && a.actions[i] < A) a.targets[i] = (float)r_s[t];
            __syncthreads();
        }
    }
    // the head, one row per thread: thread t owns rows t, t + 256, ... (it wrote their targets itself) and adds their
    // terms in row order; the workgroup sums the 256 partials in a fixed tree
    float sum = 0.f;
    for (int b = t; b < T; b += kThreads) {
        const float *q = a.q_online + (size_t)b * a.ld_q;
        float *d = a.dq + (size_t)b * a.ld_dq;
        float *td = a.td_targets ? a.td_targets + (size_t)b * a.ld_tt : nullptr;
        for (int j = 0; j < A; ++j) {
            d[j] = 0.f;                        // the target matrix equals the online prediction there
            if (td) td[j] = q[j];
        }
        const int act = a.actions[b];
        if (!rlx::taken_action_valid(act, A, 0, a.status)) continue;
        if (!given && !n_step) {
            // :112-114: (1.0 - game_over) * discount is fp64 before it meets the fp32 maximum, so the product is fp64
            const double over = (terminal && b == T - 1) ? 1.0 : 0.0;
            const double mx = (double)row_max(a.q_target + (size_t)b * a.ld_t, A);
            a.targets[b] = (float)((double)a.rewards[b] + ((1.0 - over) * a.discount) * mx);
        }
        const float tgt = a.targets[b];
        float l, g;
        rlx_losses::regression_terms(q[act] - tgt, a.huber, l, g);
        sum += l;
        d[act] = rlx_losses::regression_grad(1.f, 1.f, g, T);
        if (td) td[act] = tgt;
    }
    sum_s[t] = sum;
    __syncthreads();
    for (int s = kThreads >> 1; s > 0; s >>= 1) {
        if (t < s) sum_s[t] += sum_s[t + s];
        __syncthreads();
    }
    if (t == 0) a.scalars[0] = sum_s[0] / (float)T;
}

}  // namespace

extern "C" {

int rlx_nstep_q_window_loss(const float *q_online, long long ld_q, const float *q_target, long long ld_t, int rows_t,
                            const int *actions, const float *rewards, const unsigned char *game_over, int T,
                            int n_actions, double discount, int horizon, int huber, float *targets, float *td_targets,
                            long long ld_tt, float *dq, long long ld_dq, float *scalars, int *status, void *stream) {
    const bool given = horizon == RLX_NSTEPQ_TARGETS_GIVEN;
    RLX_REQUIRE(horizon == RLX_NSTEPQ_N_STEP || horizon == RLX_NSTEPQ_ONE_STEP || given,
                "rlx_nstep_q_window_loss: the targets horizon %d is neither N-Step nor 1-Step", horizon);
    RLX_REQUIRE(q_online && actions && targets && dq && scalars && status && (given || (rewards && game_over)) &&
                    (given || rows_t <= 0 || q_target),
                "rlx_nstep_q_window_loss: null pointer");
    RLX_REQUIRE(n_actions >= 1 && T >= 1 && rows_t >= 0,
                "rlx_nstep_q_window_loss: unsupported sizes (1 <= actions=%d, 1 <= T=%d, 0 <= target rows=%d)",
                n_actions, T, rows_t);
    RLX_REQUIRE(ld_q >= n_actions && ld_dq >= n_actions && (!td_targets || ld_tt >= n_actions) &&
                    (given || rows_t <= 0 || ld_t >= n_actions),
                "rlx_nstep_q_window_loss: leading dimension < A");
    NStepQArgs a{q_online, ld_q, q_target, ld_t, given ? 0 : rows_t, actions, rewards, game_over, T, n_actions, discount,
                 horizon, huber != 0, targets, td_targets, ld_tt, dq, ld_dq, scalars, status};
    RLX_LAUNCH((nstep_q_window_loss_kernel), 1, kThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
