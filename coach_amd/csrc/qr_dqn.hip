// Quantile-Regression DQN on gfx950: the head's loss + gradient and the acting reduction.
//
// Replaces, in the reference (paths under rl_coach/):
//   * QuantileRegressionDQNAgent.learn_from_batch   agents/qr_dqn_agent.py:99-137   (target action, TD targets,
//                                                   quantile midpoints reordered by an argsort)
//   * QuantileRegressionQHead loss                  architectures/tensorflow_components/heads/
//                                                   quantile_regression_q_head.py:55-74 (quantile Huber loss)
//   * get_q_values + EGreedy.get_action             qr_dqn_agent.py:75-76, exploration_policies/e_greedy.py:84-101
//
// theta is the head's output [B, A*N]: column a*N + j is atom j of action a.  The Q value of an action is the fp64 mean
// of its atoms (np.dot(float32 quantiles, np.ones(N) / N) promotes to fp64); both kernels accumulate it as
//   q = sum_{j = 0 .. N-1, in this order} (double)theta[a*N + j] * (1.0 / N)
// (numpy's BLAS dot may associate differently: the means agree to a few ulp, the decisions on them exactly unless two
// actions are within that distance).  Compiled with -ffp-contract=off so the fp64 arithmetic rounds like numpy.
#include "distributional_head.hpp"

namespace {

constexpr int kQrThreads = rlx::kDistLossThreads;
constexpr int kQrMaxActions = rlx::kDistMaxActions;

__device__ __forceinline__ double atom_mean(const float *row, int n_atoms, double w) {
    double s = 0.0;
    for (int j = 0; j < n_atoms; ++j) s += (double)row[j] * w;
    return s;
}

// One workgroup per batch row b.  LDS holds the taken action's quantiles theta_i, the TD targets T_j and the
// midpoints tau_i of the row; thread i owns atom i of the taken action.
struct QrArgs {
    const float *theta;         // online output [B, ld_theta]
    long long ld_theta;
    const float *theta_next;    // target output on the next states [B, ld_next]
    long long ld_next;
    const int *actions;
    const float *rewards;
    const unsigned char *game_overs;
    double discount;
    float kappa;
    int n_atoms, n_actions, batch;
    float grad_scale;
    float *dtheta;              // [B, ld_dtheta]
    long long ld_dtheta;
    float *row_partials;        // [B] workspace
    unsigned int *ticket;       // one zero-initialised word, left at zero
    float *loss;
    int *status;
    float *targets_out;         // [B, N] or null
    float *tau_out;             // [B, N] or null
    int *target_actions_out;    // [B] or null
};

__global__ void __launch_bounds__(kQrThreads) qr_dqn_head_loss_kernel(const QrArgs a) {
    __shared__ float th[kQrThreads];     // theta[b, a_b, :]
    __shared__ float tgt[kQrThreads];    // T[b, :]
    __shared__ int sigma[kQrThreads];    // argsort of th
    __shared__ double qn[kQrMaxActions];
    __shared__ float red[kQrThreads];
    __shared__ float tn_s[kQrMaxActions * kQrThreads];   // the target's row, staged with coalesced loads
    __shared__ int best_s;
    __shared__ bool last_s;
    const int b = blockIdx.x, t = threadIdx.x, N = a.n_atoms, A = a.n_actions;
    const double w = 1.0 / (double)N;
    const float *tn = a.theta_next + (size_t)b * a.ld_next;
    const int act = a.actions[b];
    const bool valid = rlx::taken_action_valid(act, A, t, a.status);

    // (2) a*_b = argmax_a of the TARGET network's fp64 means
    for (int c = t; c < A * N; c += kQrThreads) tn_s[c] = tn[c];
    __syncthreads();
    if (t < A) qn[t] = atom_mean(tn_s + t * N, N, w);
    if (t < N) th[t] = valid ? a.theta[(size_t)b * a.ld_theta + (size_t)act * N + t] : 0.f;
    __syncthreads();
    if (t == 0) {
        const int best = rlx::first_argmax_f64(qn, A);
        best_s = best;
        if (a.target_actions_out) a.target_actions_out[b] = best;
    }
    __syncthreads();
    const int best = best_s;
    float tau_t = 0.f;
    if (t < N) {
        // (3) T_j = r + (1.0 - done) * gamma * theta'[a*, j] in fp64, rounded to fp32 once (the fp32 placeholder)
        const double y = (double)a.rewards[b] + (1.0 - (a.game_overs[b] ? 1.0 : 0.0)) * a.discount *
                                                    (double)tn_s[best * N + t];
        tgt[t] = (float)y;
        if (a.targets_out) a.targets_out[(size_t)b * N + t] = (float)y;
        // (4) sigma = argsort(theta[b, a_b, :]), ties by index (a stable sort): atom t goes to position rank(t)
        const float x = th[t];
        int r = 0;
        for (int k = 0; k < N; ++k) {
            const float v = th[k];
            r += (v < x || (v == x && k < t)) ? 1 : 0;
        }
        sigma[r] = t;
    }
    __syncthreads();
    float term = 0.f, g = 0.f;
    if (t < N) {
        // tau[i] = tau_hat[sigma[i]], tau_hat_k = 0.5 * (k/N + (k+1)/N) in fp64, then fp32.  The reference indexes the
        // midpoints by the argsort ITSELF, not by its inverse (the rank): reproduced as it is, not "fixed".
        const int k = sigma[t];
        tau_t = (float)(0.5 * ((double)(k + 1) / (double)N + (double)k / (double)N));
        if (a.tau_out) a.tau_out[(size_t)b * N + t] = tau_t;
    }
    if (t < N && valid) {
        // (5) sum_j |tau_i - 1{e_ij < 0}| * huber_kappa(e_ij), e_ij = T_j - theta_i, all fp32
        // (6) dL/dtheta_i = -(1/N) sum_j |tau_i - 1{e_ij < 0}| * sign(e_ij) * min(|e_ij|, kappa)
        const float ti = th[t], kappa = a.kappa;
        for (int j = 0; j < N; ++j) {
            const float e = tgt[j] - ti;
            const float ae = fabsf(e);
            const float q = fminf(ae, kappa);
            const float h = kappa * (ae - q) + 0.5f * (q * q);
            const float wq = fabsf(tau_t - (e < 0.f ? 1.f : 0.f));
            term += wq * h;
            const float sg = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
            g += wq * (sg * q);
        }
    }
    // dtheta: the taken action's atoms, exact zeros elsewhere
    float *drow = a.dtheta + (size_t)b * a.ld_dtheta;
    for (int c = t; c < A * N; c += kQrThreads)
        if (!valid || c / N != act) drow[c] = 0.f;
    if (t < N && valid) drow[(size_t)act * N + t] = a.grad_scale * (-(g / (float)N));
    red[t] = term;
    __syncthreads();
    for (int d = kQrThreads >> 1; d > 0; d >>= 1) {
        if (t < d) red[t] += red[t + d];
        __syncthreads();
    }
    // the batch sum: the row partials, summed in a fixed tree by the workgroup that draws the last ticket
    if (!rlx::ticketed_batch_sum<kQrThreads>(red[0], b, a.batch, a.row_partials, a.ticket, red, &last_s, t)) return;
    if (t == 0) a.loss[0] = red[0] / (float)N;
}

// One wave per env: lanes a < A form the fp64 means (order above), lane 0 makes the epsilon-greedy choice on them
// (distributional_head.hpp: numpy's isclose in fp64, e_greedy.py:93-94).
__global__ void __launch_bounds__(64) quantile_egreedy_kernel(const float *__restrict__ quant, long long ld, int n_atoms,
                                                              const double *__restrict__ explore_u,
                                                              const int *__restrict__ random_act,
                                                              const double *__restrict__ tie_rand, double epsilon,
                                                              int n_env, int n_actions, double *__restrict__ q_out,
                                                              int *__restrict__ actions) {
    __shared__ double q[64];
    const int e = blockIdx.x, t = threadIdx.x;
    const double w = 1.0 / (double)n_atoms;
    if (t < n_actions) {
        q[t] = atom_mean(quant + (size_t)e * ld + (size_t)t * n_atoms, n_atoms, w);
        if (q_out) q_out[(size_t)e * n_actions + t] = q[t];
    }
    __syncthreads();
    if (t != 0) return;
    actions[e] = rlx::egreedy_choice_f64(q, n_actions, explore_u[e], random_act[e], tie_rand + (size_t)e * n_actions,
                                         epsilon);
}

// ParameterNoise acting (exploration_policies/parameter_noise.py:62-68): np.argmax of the same fp64 means — the first
// maximum, no draws.
__global__ void __launch_bounds__(64) quantile_argmax_kernel(const float *__restrict__ quant, long long ld, int n_atoms,
                                                             int n_actions, double *__restrict__ q_out,
                                                             int *__restrict__ actions) {
    __shared__ double q[64];
    const int e = blockIdx.x, t = threadIdx.x;
    const double w = 1.0 / (double)n_atoms;
    if (t < n_actions) {
        q[t] = atom_mean(quant + (size_t)e * ld + (size_t)t * n_atoms, n_atoms, w);
        if (q_out) q_out[(size_t)e * n_actions + t] = q[t];
    }
    __syncthreads();
    if (t == 0) actions[e] = rlx::first_argmax_f64(q, n_actions);
}

}  // namespace

extern "C" {

int rlx_qr_dqn_head_loss(const float *theta, long long ld_theta, const float *theta_next_target, long long ld_next,
                         const int *actions, const float *rewards, const unsigned char *game_overs, double discount,
                         float kappa, int n_atoms, int n_actions, int batch, float grad_scale, float *dtheta,
                         long long ld_dtheta, float *row_partials, unsigned int *ticket, float *loss_scalar,
                         int *status, float *targets_out, float *tau_out, int *target_actions_out, void *stream) {
    RLX_REQUIRE(theta && theta_next_target && actions && rewards && game_overs && dtheta && row_partials && ticket &&
                    loss_scalar && status,
                "rlx_qr_dqn_head_loss: null pointer");
    if (const int rc = rlx::check_head_loss_shape("rlx_qr_dqn_head_loss", 1, n_atoms, n_actions, batch, ld_theta,
                                                  ld_next, ld_dtheta))
        return rc;
    QrArgs a;
    a.theta = theta; a.ld_theta = ld_theta; a.theta_next = theta_next_target; a.ld_next = ld_next;
    a.actions = actions; a.rewards = rewards; a.game_overs = game_overs; a.discount = discount; a.kappa = kappa;
    a.n_atoms = n_atoms; a.n_actions = n_actions; a.batch = batch; a.grad_scale = grad_scale;
    a.dtheta = dtheta; a.ld_dtheta = ld_dtheta; a.row_partials = row_partials; a.ticket = ticket;
    a.loss = loss_scalar; a.status = status; a.targets_out = targets_out; a.tau_out = tau_out;
    a.target_actions_out = target_actions_out;
    RLX_LAUNCH((qr_dqn_head_loss_kernel), batch, kQrThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_quantile_egreedy(const float *quantiles, long long ld, int n_atoms, const double *explore_uniforms,
                         const int *random_actions, const double *tie_break_uniforms, double epsilon, int n_env,
                         int n_actions, double *q_out, int *actions, void *stream) {
    RLX_REQUIRE(quantiles && explore_uniforms && random_actions && tie_break_uniforms && actions,
                "rlx_quantile_egreedy: null pointer");
    RLX_REQUIRE(n_env > 0 && n_atoms > 0 && n_actions > 0 && n_actions <= 64 && ld >= (long long)n_atoms * n_actions,
                "rlx_quantile_egreedy: bad shape");
    RLX_LAUNCH((quantile_egreedy_kernel), n_env, 64, 0, rlx::as_stream(stream), quantiles, ld, n_atoms,
               explore_uniforms, random_actions, tie_break_uniforms, epsilon, n_env, n_actions, q_out, actions);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_quantile_argmax(const float *quantiles, long long ld, int n_atoms, int n_env, int n_actions, double *q_out,
                        int *actions, void *stream) {
    RLX_REQUIRE(quantiles && actions, "rlx_quantile_argmax: null pointer");
    RLX_REQUIRE(n_env > 0 && n_atoms > 0 && n_actions > 0 && n_actions <= 64 && ld >= (long long)n_atoms * n_actions,
                "rlx_quantile_argmax: bad shape");
    RLX_LAUNCH((quantile_argmax_kernel), n_env, 64, 0, rlx::as_stream(stream), quantiles, ld, n_atoms, n_actions, q_out,
               actions);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
