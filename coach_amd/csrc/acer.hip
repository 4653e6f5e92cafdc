// ACER on gfx950: everything between the forward and the backward pass of one update window, one launch.
//
// Replaces, in the reference (paths under rl_coach/):
//   * ACERAgent._learn_from_batch's state values, importance weights and Q-retrace targets   agents/acer_agent.py:127-154
//   * QHead's loss (MSE under loss_weight) on the aliased target matrix       .../heads/head.py:143-186 (losses_body.hpp)
//   * ACERPolicyHead (truncated importance weights, bias correction, KL, trust region)
//                                                                     .../heads/acer_policy_head.py:47-113 (acer_head.hpp)
//     (... = architectures/tensorflow_components)
//
// A latency-bound row kernel over a few to a few hundred rows: ONE workgroup, so the retrace recurrence has the
// reference's order, every batch sum has a fixed order and there are no float atomics.  Nothing leaves the device: a
// window is forward (online on T + 1 states, average network on T), this launch, backward.  tests/acer_ref.py is the
// numpy restatement; it states every fp32 / fp64 rounding point named here.  Compiled with -ffp-contract=off so the
// arithmetic rounds like numpy.
#include "acer_head.hpp"
#include "losses_body.hpp"

namespace {

constexpr int kThreads = rlx::kPgThreads;

struct AcerArgs {
    const float *q;                 // [rows][ld_q]: the online Q head
    long long ld_q;
    const float *logits;            // [rows][ld_z]: the online policy head
    long long ld_z;
    int rows;
    const float *avg_logits;        // [T][ld_az]: the average network's policy head
    long long ld_az;
    const float *mu;                // [T][ld_mu]: the behaviour policy's probabilities
    long long ld_mu;
    const int *actions;             // [T]
    const float *rewards;           // [T]
    const unsigned char *game_over; // the last transition's flag
    int T, A;
    double discount;
    float c, delta, beta, q_weight;
    int mode;
    float *V;                       // [T]          out (in with RLX_ACER_TARGETS_GIVEN, as the four below)
    float *rho;                     // [T][ld_rho]
    long long ld_rho;
    float *rho_i;                   // [T]
    float *avg_p;                   // [T][ld_ap]
    long long ld_ap;
    float *q_retrace;               // [T]
    float *boot;                    // [1] out: sum Q p of the state behind the window (0 on a game over)
    float *td_targets;              // [T][ld_tt] or null: out (in with RLX_ACER_TARGETS_GIVEN)
    long long ld_tt;
    float *dq;                      // [rows][ld_dq]
    long long ld_dq;
    float *dlogits;                 // [rows][ld_dz]
    long long ld_dz;
    float *scalars;                 // [7]
    int *status;
};

__global__ void __launch_bounds__(kThreads) acer_window_loss_kernel(const AcerArgs a) {
    // a chunk of the window: the recurrence's inputs; r_s is overwritten by its results (T-independent)
    __shared__ double r_s[kThreads];
    __shared__ float qi_s[kThreads], rb_s[kThreads], v_s[kThreads];
    __shared__ float sum_s[5][kThreads];
    const int t = threadIdx.x, T = a.T, A = a.A;
    const bool given = (a.mode & RLX_ACER_TARGETS_GIVEN) != 0, trust = (a.mode & RLX_ACER_TRUST_REGION) != 0;
    if (!given) {
        const bool terminal = *a.game_over != 0;
        if (!terminal && a.rows <= T) {         // the bootstrap row is missing: nothing is read or written
            if (t == 0) atomicOr(a.status, RLX_ACER_STATUS_NO_BOOTSTRAP_ROW);
            return;
        }
        // phase 1, one row per thread (thread t owns rows t, t + 256, ...): p, the average policy, V, rho, rho_a
        rlx::PgRow r;
        for (int b = t; b < T; b += kThreads) {
            const float *q = a.q + (size_t)b * a.ld_q, *mu = a.mu + (size_t)b * a.ld_mu;
            float *rho = a.rho + (size_t)b * a.ld_rho, *ap = a.avg_p + (size_t)b * a.ld_ap;
            rlx::pg_row(a.avg_logits + (size_t)b * a.ld_az, A, r);
            for (int j = 0; j < A; ++j) ap[j] = r.p[j];
            rlx::pg_row(a.logits + (size_t)b * a.ld_z, A, r);
            a.V[b] = rlx::np_sum_row([&](int j) { return r.p[j] * q[j]; }, A);                  // :129
            for (int j = 0; j < A; ++j) rho[j] = r.p[j] / (mu[j] + rlx::kPgEps);                 // :138
            const int act = a.actions[b];
            a.rho_i[b] = (act >= 0 && act < A) ? rho[act] : 0.f;
        }
        // lane 0's carried product discount * Qret, across chunks.  :150, first pass: an fp32 product of fp32(discount)
        // and the fp32 sum of the state behind the window; Qret is fp64 from the first sum on (acer_ref.py)
        double p = 0.0;
        if (t == 0) {
            float boot = 0.f;
            if (!terminal) {
                const float *q = a.q + (size_t)T * a.ld_q;
                rlx::pg_row(a.logits + (size_t)T * a.ld_z, A, r);
                boot = rlx::np_sum_row([&](int j) { return q[j] * r.p[j]; }, A);                 // :147
                p = (double)((float)a.discount * boot);
            }
            a.boot[0] = boot;
        }
        // phase 2, the retrace recurrence: lane 0 walks chunks of 256 rows from the end
        for (int ch = (T + kThreads - 1) / kThreads - 1; ch >= 0; --ch) {
            const int i = ch * kThreads + t;
            if (i < T) {                                               // the values this thread wrote itself
                const int act = a.actions[i];
                const bool ok = act >= 0 && act < A;
                r_s[t] = (double)a.rewards[i];
                qi_s[t] = ok ? a.q[(size_t)i * a.ld_q + act] : 0.f;    // :135, Q_i
                rb_s[t] = fminf(1.f, a.rho_i[i]);                      // :141, rho_bar
                v_s[t] = a.V[i];
            }
            __syncthreads();
            if (t == 0) {                                              // the sequential recurrence, the reference's order
                const int hi = min(T - ch * kThreads, kThreads);
                for (int k = hi - 1; k >= 0; --k) {
                    const double R = r_s[k] + p;                       // :150
                    const double Qret = (double)rb_s[k] * (R - (double)qi_s[k]) + (double)v_s[k];   // :152
                    p = a.discount * Qret;
                    r_s[k] = R;
                }
            }
            __syncthreads();
            if (i < T) a.q_retrace[i] = (float)r_s[t];                 // :151, the store into the fp32 matrix: the rounding
            __syncthreads();
        }
    }
    // phase 3, the two heads, one row per thread again (it wrote the row's values itself); the workgroup sums the 256
    // partials of every scalar in a fixed tree
    const float fT = (float)T;
    float qsum = 0.f;
    rlx::AcerRowSums s{0.f, 0.f, 0.f, 0.f};
    for (int b = t; b < a.rows; b += kThreads) {
        float *dq = a.dq + (size_t)b * a.ld_dq, *dz = a.dlogits + (size_t)b * a.ld_dz;
        for (int j = 0; j < A; ++j) {          // the target matrix equals the prediction off the taken entry; a row
            dq[j] = 0.f;                       // without a term (the bootstrap row, an action out of range) stays zero
            dz[j] = 0.f;
        }
        if (b >= T) continue;
        const float *q = a.q + (size_t)b * a.ld_q;
        float *td = a.td_targets ? a.td_targets + (size_t)b * a.ld_tt : nullptr;
        if (td && !given)
            for (int j = 0; j < A; ++j) td[j] = q[j];
        const int act = a.actions[b];
        if (!rlx::taken_action_valid(act, A, 0, a.status)) continue;
        const float qret = a.q_retrace[b], V = a.V[b];
        if (td && !given) td[act] = qret;                              // :133, :151: Q_head_targets IS Q_values
        float l, g;
        rlx_losses::regression_terms(q[act] - qret, 0, l, g);
        qsum += a.q_weight * l;
        dq[act] = rlx_losses::regression_grad(1.f, a.q_weight, g, T);
        const bool read_td = td && given;
        rlx::acer_row_loss_grad(
            a.logits + (size_t)b * a.ld_z, A, act, [&](int k) { return read_td ? td[k] : (k == act ? qret : q[k]); },
            a.avg_p + (size_t)b * a.ld_ap, a.rho + (size_t)b * a.ld_rho, a.rho_i[b], qret, V, a.c, a.delta, a.beta,
            trust, fT, dz, s);
    }
    sum_s[0][t] = qsum;
    sum_s[1][t] = s.prob;
    sum_s[2][t] = s.bias;
    sum_s[3][t] = s.kl;
    sum_s[4][t] = s.ent;
    __syncthreads();
    for (int d = kThreads >> 1; d > 0; d >>= 1) {
        if (t < d)
            for (int n = 0; n < 5; ++n) sum_s[n][t] += sum_s[n][t + d];
        __syncthreads();
    }
    if (t == 0) {
        const float q_loss = sum_s[0][0] / fT, prob_loss = -(sum_s[1][0] / fT), bias_loss = -(sum_s[2][0] / fT);
        const float policy_loss = prob_loss + bias_loss, mean_h = sum_s[4][0] / fT;
        a.scalars[0] = q_loss + (policy_loss - a.beta * mean_h);
        a.scalars[1] = q_loss;
        a.scalars[2] = policy_loss;
        a.scalars[3] = prob_loss;
        a.scalars[4] = bias_loss;
        a.scalars[5] = sum_s[3][0] / fT;
        a.scalars[6] = mean_h;
    }
}

}  // namespace

extern "C" {

int rlx_acer_window_loss(const float *q, long long ld_q, const float *logits, long long ld_logits, int rows,
                         const float *avg_logits, long long ld_avg_logits, const float *mu, long long ld_mu,
                         const int *actions, const float *rewards, const unsigned char *game_over, int T, int n_actions,
                         double discount, float truncation, float max_kl, float beta_entropy, float q_loss_weight,
                         int mode, float *V, float *rho, long long ld_rho, float *rho_i, float *avg_policy,
                         long long ld_avg_policy, float *q_retrace, float *bootstrap_value, float *td_targets,
                         long long ld_tt, float *dq, long long ld_dq, float *dlogits, long long ld_dlogits,
                         float *scalars, int *status, void *stream) {
    const bool given = (mode & RLX_ACER_TARGETS_GIVEN) != 0;
    RLX_REQUIRE((mode & ~(RLX_ACER_TRUST_REGION | RLX_ACER_TARGETS_GIVEN)) == 0,
                "rlx_acer_window_loss: unknown mode bits in %d", mode);
    RLX_REQUIRE(q && logits && actions && V && rho && rho_i && avg_policy && q_retrace && dq && dlogits && scalars &&
                    status && (given || (avg_logits && mu && rewards && game_over && bootstrap_value)),
                "rlx_acer_window_loss: null pointer");
    RLX_REQUIRE(n_actions >= 1 && n_actions <= rlx::kPgMaxActions && T >= 1 && (rows == T || rows == T + 1),
                "rlx_acer_window_loss: unsupported sizes (1 <= actions=%d <= 18, 1 <= T=%d, rows=%d is T or T + 1)",
                n_actions, T, rows);
    RLX_REQUIRE(ld_q >= n_actions && ld_logits >= n_actions && ld_rho >= n_actions && ld_avg_policy >= n_actions &&
                    ld_dq >= n_actions && ld_dlogits >= n_actions && (!td_targets || ld_tt >= n_actions) &&
                    (given || (ld_avg_logits >= n_actions && ld_mu >= n_actions)),
                "rlx_acer_window_loss: leading dimension < A");
    AcerArgs a{q, ld_q, logits, ld_logits, rows, avg_logits, ld_avg_logits, mu, ld_mu, actions, rewards, game_over, T,
               n_actions, discount, truncation, max_kl, beta_entropy, q_loss_weight, mode, V, rho, ld_rho, rho_i,
               avg_policy, ld_avg_policy, q_retrace, bootstrap_value, td_targets, ld_tt, dq, ld_dq, dlogits, ld_dlogits,
               scalars, status};
    RLX_LAUNCH((acer_window_loss_kernel), 1, kThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
