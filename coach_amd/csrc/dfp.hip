// Direct Future Prediction (DFP) on gfx950: the head's loss and gradients, the acting reduction and the episode-end
// future-measurement targets.
//
// Replaces, in the reference (paths under rl_coach/):
//   * DFPAgent.learn_from_batch                     agents/dfp_agent.py:150-167 (targets = prediction, the taken action's
//                                                   row = the stored future measurements)
//   * MeasurementsPredictionHead                    architectures/tensorflow_components/heads/
//                                                   measurements_prediction_head.py:39-62 (merge of the two streams, NaN
//                                                   targets replaced by the prediction, sum over (a, k) of the batch mean)
//   * DFPAgent.choose_action + EGreedy.get_action   dfp_agent.py:169-199, exploration_policies/e_greedy.py:84-101
//   * DFPAgent._update_measurements_targets         dfp_agent.py:235-255
//
// E is the expectation stream's Dense output [B][K], X the action stream's [B][A*K] (column a*K + k), K = S * M: step s,
// measurement m is column s*M + m.  The merge is rlx::dfp_merge_row (dfp_merge.hpp).  64-lane waves, no float atomics,
// fixed summation orders; compiled with -ffp-contract=off so that tests/dfp_ref.py restates every rounding.
#include "dfp_merge.hpp"
#include "distributional_head.hpp"

namespace {

constexpr int kDfpThreads = rlx::kDistLossThreads;    // ticketed_batch_sum: batch <= threads
constexpr int kDfpMaxActions = rlx::kDistMaxActions;
constexpr int kDfpMaxColumns = 64;
constexpr int kDfpMaxSteps = 8, kDfpMaxMeasurements = 8;

struct DfpLossArgs {
    const float *e;             // [B, ld_e]
    long long ld_e;
    const float *x;             // [B, ld_x]
    long long ld_x;
    const int *actions;
    const float *future;        // [B, K], may hold NaN
    int n_actions, n_columns, batch;
    float grad_scale;
    float *de;                  // [B, ld_de]
    long long ld_de;
    float *dx;                  // [B, ld_dx]
    long long ld_dx;
    float *row_partials;        // [B] workspace
    unsigned int *ticket;       // one zero-initialised word, left at zero
    float *loss;
    int *status;
    float *y_out;               // [B, A*K] or null
    float *targets_out;         // [B, A*K] or null
};

// One workgroup per batch row b; thread k < K owns column k of the row.
__global__ void __launch_bounds__(kDfpThreads) dfp_head_loss_kernel(const DfpLossArgs a) {
    __shared__ float y_s[kDfpMaxActions * kDfpMaxColumns];
    __shared__ float sq_s[kDfpMaxColumns];
    __shared__ float red[kDfpThreads];
    __shared__ bool last_s;
    const int b = blockIdx.x, t = threadIdx.x, A = a.n_actions, K = a.n_columns;
    const int act = a.actions[b];
    const bool valid = rlx::taken_action_valid(act, A, t, a.status);
    rlx::dfp_merge_row(a.e + (size_t)b * a.ld_e, a.x + (size_t)b * a.ld_x, A, K, y_s, t, kDfpThreads);
    if (t < K) {
        // only this thread wrote column t of y_s: no barrier needed before it reads the column back
        const float fm = a.future[(size_t)b * K + t];
        const bool term = valid && !__builtin_isnan(fm);
        float g = 0.f, sq = 0.f;
        if (term) {
            const float y = y_s[act * K + t];
            const float d = fm - y;
            sq = d * d;
            g = ((a.grad_scale * 2.f) * (y - fm)) / (float)a.batch;
        }
        sq_s[t] = sq;
        a.de[(size_t)b * a.ld_de + t] = g;
        const float inv = 1.f / (float)A;
        for (int k = 0; k < A; ++k) {
            const float c = (k == act ? 1.f : 0.f) - inv;
            a.dx[(size_t)b * a.ld_dx + k * K + t] = term ? g * c : 0.f;
            const float y = y_s[k * K + t];
            if (a.y_out) a.y_out[((size_t)b * A + k) * K + t] = y;
            if (a.targets_out) a.targets_out[((size_t)b * A + k) * K + t] = (term && k == act) ? fm : y;
        }
    }
    __syncthreads();
    float row = 0.f;
    if (t == 0)
        for (int k = 0; k < K; ++k) row += sq_s[k];
    if (!rlx::ticketed_batch_sum<kDfpThreads>(row, b, a.batch, a.row_partials, a.ticket, red, &last_s, t)) return;
    // the workgroup that drew the last ticket: every row partial is visible (the fence inside).  The loss is the rows
    // summed in ROW order, so one thread adds them (batch <= 256), not the tree left in red.
    if (t == 0) {
        float s = 0.f;
        for (int r = 0; r < a.batch; ++r)
            s += __hip_atomic_load(&a.row_partials[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.loss[0] = s / (float)a.batch;
    }
}

struct DfpActArgs {
    const float *e;
    long long ld_e;
    const float *x;
    long long ld_x;
    const double *goal;         // [M]
    const double *weights;      // [W]
    int n_steps, n_measurements, n_weights, n_actions;
    double *q_out;              // [n_env, A] or null
    int *actions;
};

// The fp64 score of every action of env e into q[0 .. A): one wave per env, lane a < A scores action a.
// v[a] = sum_{j = 0 .. W-1} (sum_{m = 0 .. M-1} (double)y[a][(S - W + j)*M + m] * goal[m]) * w[j], both sums from 0.0 in
// index order (np.dot of dfp_agent.py:184-186 for the sizes in use).  Ends with a barrier.
__device__ __forceinline__ void dfp_scores(const DfpActArgs &p, int e, int t, float *y_s, double *q) {
    const int A = p.n_actions, S = p.n_steps, M = p.n_measurements, W = p.n_weights, K = S * M;
    rlx::dfp_merge_row(p.e + (size_t)e * p.ld_e, p.x + (size_t)e * p.ld_x, A, K, y_s, t, 64);
    __syncthreads();
    if (t < A) {
        const float *y = y_s + t * K;
        double v = 0.0;
        for (int j = 0; j < W; ++j) {
            const int s = S - W + j;
            double f = 0.0;
            for (int m = 0; m < M; ++m) f += (double)y[s * M + m] * p.goal[m];
            v += f * p.weights[j];
        }
        q[t] = v;
        if (p.q_out) p.q_out[(size_t)e * A + t] = v;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(64) dfp_egreedy_kernel(const DfpActArgs p, const double *__restrict__ explore_u,
                                                         const int *__restrict__ random_act,
                                                         const double *__restrict__ tie_rand, double epsilon) {
    __shared__ float y_s[kDfpMaxActions * kDfpMaxColumns];
    __shared__ double q[kDfpMaxActions];
    const int e = blockIdx.x, t = threadIdx.x;
    dfp_scores(p, e, t, y_s, q);
    if (t == 0)
        p.actions[e] = rlx::egreedy_choice_f64(q, p.n_actions, explore_u[e], random_act[e],
                                               tie_rand + (size_t)e * p.n_actions, epsilon);
}

// ParameterNoise acting (exploration_policies/parameter_noise.py:62-68): np.argmax of the same scores, no draws.
__global__ void __launch_bounds__(64) dfp_argmax_kernel(const DfpActArgs p) {
    __shared__ float y_s[kDfpMaxActions * kDfpMaxColumns];
    __shared__ double q[kDfpMaxActions];
    const int e = blockIdx.x, t = threadIdx.x;
    dfp_scores(p, e, t, y_s, q);
    if (t == 0) p.actions[e] = rlx::first_argmax_f64(q, p.n_actions);
}

// _update_measurements_targets for ONE completed episode of T transitions in a time-major ring (row of step k =
// ((s0 + k) mod ring_steps) * n_env + env).  One thread per (transition i, step s).
__global__ void dfp_future_measurements_kernel(const double *__restrict__ meas, float *__restrict__ out,
                                               const double *__restrict__ scale, long long s0, int T, int env, int n_env,
                                               long long ring_steps, int S, int M, int last_step_mode) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (long long)T * S) return;
    const int i = (int)(c / S), s = (int)(c - (long long)i * S);
    auto row = [&](long long k) { return ((s0 + k) % ring_steps) * n_env + env; };
    float *o = out + (size_t)row(i) * S * M + (size_t)s * M;
    long long off = (long long)i + (1LL << s);
    if (off >= T) {
        if (!last_step_mode) {
            for (int m = 0; m < M; ++m) o[m] = __builtin_nanf("");
            return;
        }
        off = T - 1;                                   // transitions[-1].state
    }
    const double *mo = meas + (size_t)row(off) * M, *mi = meas + (size_t)row(i) * M;
    for (int m = 0; m < M; ++m) o[m] = (float)(scale[m] * (mo[m] - mi[m]));
}

// use_accumulated_reward_as_measurement (agents/agent.py:920-925, :958) for n_env envs after one vector step.  The reference
// injects its running sum of shaped rewards into the NEXT state's measurements BEFORE observe_transition adds the step's
// reward, so the measurement lags by one step: the state after step t carries the rewards of steps 1 .. t-1, and the first
// two states of an episode both carry 0.  One thread per env: the measurements of the state the step was taken in go to
// state_out (the replay's column), the next state's accumulated-reward measurement becomes the sum before this step's
// reward (0 after a game over: the post-reset state of a new episode), the sum takes the reward (0 after a game over).
__global__ void dfp_accumulated_reward_kernel(const float *__restrict__ reward, const unsigned char *__restrict__ game_over,
                                              double *__restrict__ acc, double *__restrict__ cur, float *__restrict__ cur32,
                                              double *__restrict__ state_out, int n_env, int M, int col) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    if (state_out)
        for (int m = 0; m < M; ++m) state_out[(size_t)e * M + m] = cur[(size_t)e * M + m];
    const bool over = game_over[e] != 0;
    const double a = acc[e];
    const double next = over ? 0.0 : a;
    cur[(size_t)e * M + col] = next;
    if (cur32) cur32[(size_t)e * M + col] = (float)next;
    acc[e] = over ? 0.0 : a + (double)reward[e];
}

int check_act_shape(const char *fn, int n_steps, int n_measurements, int n_weights, int n_env, int n_actions,
                    long long ld_e, long long ld_x) {
    const long long K = (long long)n_steps * n_measurements;
    RLX_REQUIRE(n_env > 0 && n_actions >= 1 && n_actions <= kDfpMaxActions && n_steps >= 1 && n_measurements >= 1 &&
                    K <= kDfpMaxColumns && n_weights >= 1 && n_weights <= n_steps,
                "%s: unsupported sizes (actions=%d <= 18, steps=%d * measurements=%d <= 64, 1 <= weights=%d <= steps)", fn,
                n_actions, n_steps, n_measurements, n_weights);
    RLX_REQUIRE(ld_e >= K && ld_x >= K * n_actions, "%s: leading dimension too small", fn);
    return RLX_OK;
}

}  // namespace

extern "C" {

int rlx_dfp_head_loss(const float *expectation, long long ld_e, const float *action_stream, long long ld_x,
                      const int *actions, const float *future_measurements, int n_actions, int n_columns, int batch,
                      float grad_scale, float *d_expectation, long long ld_de, float *d_action_stream, long long ld_dx,
                      float *row_partials, unsigned int *ticket, float *loss_scalar, int *status, float *y_out,
                      float *targets_out, void *stream) {
    RLX_REQUIRE(expectation && action_stream && actions && future_measurements && d_expectation && d_action_stream &&
                    row_partials && ticket && loss_scalar && status,
                "rlx_dfp_head_loss: null pointer");
    RLX_REQUIRE(n_actions >= 1 && n_actions <= kDfpMaxActions && n_columns >= 1 && n_columns <= kDfpMaxColumns &&
                    batch >= 1 && batch <= kDfpThreads,
                "rlx_dfp_head_loss: unsupported sizes (1 <= actions=%d <= 18, 1 <= columns=%d <= 64, batch=%d <= 256)",
                n_actions, n_columns, batch);
    const long long row = (long long)n_actions * n_columns;
    RLX_REQUIRE(ld_e >= n_columns && ld_de >= n_columns && ld_x >= row && ld_dx >= row,
                "rlx_dfp_head_loss: leading dimension too small");
    DfpLossArgs a;
    a.e = expectation; a.ld_e = ld_e; a.x = action_stream; a.ld_x = ld_x; a.actions = actions;
    a.future = future_measurements; a.n_actions = n_actions; a.n_columns = n_columns; a.batch = batch;
    a.grad_scale = grad_scale; a.de = d_expectation; a.ld_de = ld_de; a.dx = d_action_stream; a.ld_dx = ld_dx;
    a.row_partials = row_partials; a.ticket = ticket; a.loss = loss_scalar; a.status = status; a.y_out = y_out;
    a.targets_out = targets_out;
    RLX_LAUNCH((dfp_head_loss_kernel), batch, kDfpThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_dfp_egreedy(const float *expectation, long long ld_e, const float *action_stream, long long ld_x,
                    const double *goal, const double *weights, int n_steps, int n_measurements, int n_weights,
                    const double *explore_uniforms, const int *random_actions, const double *tie_break_uniforms,
                    double epsilon, int n_env, int n_actions, double *q_out, int *actions, void *stream) {
    RLX_REQUIRE(expectation && action_stream && goal && weights && explore_uniforms && random_actions &&
                    tie_break_uniforms && actions,
                "rlx_dfp_egreedy: null pointer");
    if (const int rc = check_act_shape("rlx_dfp_egreedy", n_steps, n_measurements, n_weights, n_env, n_actions, ld_e, ld_x))
        return rc;
    const DfpActArgs p{expectation, ld_e, action_stream, ld_x, goal, weights, n_steps, n_measurements, n_weights,
                       n_actions, q_out, actions};
    RLX_LAUNCH((dfp_egreedy_kernel), n_env, 64, 0, rlx::as_stream(stream), p, explore_uniforms, random_actions,
               tie_break_uniforms, epsilon);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_dfp_argmax(const float *expectation, long long ld_e, const float *action_stream, long long ld_x,
                   const double *goal, const double *weights, int n_steps, int n_measurements, int n_weights, int n_env,
                   int n_actions, double *q_out, int *actions, void *stream) {
    RLX_REQUIRE(expectation && action_stream && goal && weights && actions, "rlx_dfp_argmax: null pointer");
    if (const int rc = check_act_shape("rlx_dfp_argmax", n_steps, n_measurements, n_weights, n_env, n_actions, ld_e, ld_x))
        return rc;
    const DfpActArgs p{expectation, ld_e, action_stream, ld_x, goal, weights, n_steps, n_measurements, n_weights,
                       n_actions, q_out, actions};
    RLX_LAUNCH((dfp_argmax_kernel), n_env, 64, 0, rlx::as_stream(stream), p);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_dfp_future_measurements(const double *measurements, float *future_measurements, const double *scale,
                                long long first_step, int length, int env, int n_env, long long ring_steps, int n_steps,
                                int n_measurements, int last_step_mode, void *stream) {
    RLX_REQUIRE(measurements && future_measurements && scale, "rlx_dfp_future_measurements: null pointer");
    RLX_REQUIRE(length > 0 && n_env > 0 && env >= 0 && env < n_env && ring_steps >= length && first_step >= 0,
                "rlx_dfp_future_measurements: bad episode geometry (length=%d ring_steps=%lld)", length, ring_steps);
    RLX_REQUIRE(n_steps >= 1 && n_steps <= kDfpMaxSteps && n_measurements >= 1 && n_measurements <= kDfpMaxMeasurements,
                "rlx_dfp_future_measurements: unsupported sizes (1 <= steps=%d <= 8, 1 <= measurements=%d <= 8)", n_steps,
                n_measurements);
    RLX_REQUIRE(last_step_mode == 0 || last_step_mode == 1, "rlx_dfp_future_measurements: mode is 0 (NAN) or 1 (LastStep)");
    const long long n = (long long)length * n_steps;
    RLX_LAUNCH((dfp_future_measurements_kernel), (unsigned)((n + 255) / 256), 256, 0, rlx::as_stream(stream), measurements,
               future_measurements, scale, first_step, length, env, n_env, ring_steps, n_steps, n_measurements,
               last_step_mode);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_dfp_accumulated_reward_step(const float *rewards, const unsigned char *game_overs, double *accumulated,
                                    double *measurements, float *measurements32, double *state_measurements_out, int n_env,
                                    int n_measurements, int column, void *stream) {
    RLX_REQUIRE(rewards && game_overs && accumulated && measurements, "rlx_dfp_accumulated_reward_step: null pointer");
    RLX_REQUIRE(n_env > 0 && n_measurements >= 1 && n_measurements <= kDfpMaxMeasurements && column >= 0 &&
                    column < n_measurements,
                "rlx_dfp_accumulated_reward_step: bad sizes (n_env=%d, 1 <= measurements=%d <= 8, column=%d)", n_env,
                n_measurements, column);
    RLX_LAUNCH((dfp_accumulated_reward_kernel), (n_env + 63) / 64, 64, 0, rlx::as_stream(stream), rewards, game_overs,
               accumulated, measurements, measurements32, state_measurements_out, n_env, n_measurements, column);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
