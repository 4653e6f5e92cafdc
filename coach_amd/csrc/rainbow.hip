// Rainbow DQN on gfx950: the dueling categorical head's loss + gradient and its acting reductions.
//
// Replaces, in the reference (paths under rl_coach/):
//   * RainbowDQNAgent.learn_from_batch     agents/rainbow_dqn_agent.py:88-137 (Double-DQN target action, the projection of
//                                          the support shifted by the n-step return and scaled by discount ** n_step, gated
//                                          by should_bootstrap_next_state)
//   * RainbowQHead                         architectures/tensorflow_components/heads/rainbow_q_head.py:43-70 (a state-value
//                                          stream of N logits and an action-advantage stream of A*N logits, merged per atom,
//                                          softmax over the atoms, softmax_cross_entropy_with_logits)
//   * distribution_prediction_to_q_values + the exploration policy's choice (categorical_dqn_agent.py:86-87)
//
// v is the state-value stream's Dense output [B, N], x the action-advantage stream's [B, A*N] (column a*N + j is atom j
// of action a).  The merge, fp32, per atom j, is dfp_merge.hpp's, i.e. rlx_dueling_combine's order applied per atom:
//   s = 0.f, then += x[a][j] for a ascending;  mean = s / (float)A;  y[a][j] = v[j] + (x[a][j] - mean)
// TensorFlow's own reduce_mean may sum the actions in another order: that rounding is one of those DESIGN §6 lists as
// not pinned.  From the merged logits on, softmax, expectations and projection are categorical_head.hpp's, so for equal
// merged logits the results equal rlx_c51_head_loss's bit for bit.  Compiled with -ffp-contract=off.
#include "categorical_head.hpp"

namespace {

constexpr int kThreads = rlx::kDistLossThreads;
constexpr int kMaxAtoms = rlx::kCatMaxAtoms;
constexpr int kMaxActions = rlx::kCatMaxActions;

using rlx::expectation;
using rlx::softmax_rows;

struct Streams {
    const float *v;   // [B, ld_v], N columns used
    long long ld_v;
    const float *x;   // [B, ld_x], A*N columns used
    long long ld_x;
};

struct RainbowArgs {
    Streams online, target_next, online_next;   // online on s, target on s', online on s'
    const double *z;                  // [N] support
    const int *actions;
    const double *returns;            // [B] n-step discounted rewards
    const unsigned char *bootstrap;   // [B] should_bootstrap_next_state
    double discount_n;                // discount ** n_step, the host's
    int n_atoms, n_actions, batch;
    float grad_scale;
    float *dv;                        // [B, ld_dv]
    long long ld_dv;
    float *dx;                        // [B, ld_dx]
    long long ld_dx;
    double *per_errors;               // [B] or null: the taken action's cross entropy
    float *row_partials;              // [B] workspace
    unsigned int *ticket;             // one zero-initialised word, left at zero
    float *loss;
    int *status;
    float *m_out;                     // [B, N] or null
    int *target_actions_out;          // [B] or null
    float *action_losses_out;         // [B, A] or null
    float *merged_out;                // [B, A*N] or null: the online network's merged logits on s
    float *dlogits_out;               // [B, A*N] or null: the gradient at the merged logits
};

// One workgroup per batch row b.  LDS holds TWO sets of A*N floats, used three times over: first the online network's
// distributions on s' (pn) and on s (po); once a* is known pn is dead and takes the target network's merged logits on s',
// of which only row a* is softmaxed; after the projection pn is dead again and takes the online merged logits on s (the
// same bits as the first merge: same function, same inputs) and then the cross-entropy terms, while po takes dlogits.
__global__ void __launch_bounds__(kThreads) rainbow_head_loss_kernel(const RainbowArgs a) {
    __shared__ float p_s[2 * kMaxActions * kMaxAtoms];
    __shared__ double z_s[kMaxAtoms];
    __shared__ double wl_s[kMaxAtoms], wu_s[kMaxAtoms];
    __shared__ int l_s[kMaxAtoms], u_s[kMaxAtoms];
    __shared__ float m_s[kMaxAtoms];
    __shared__ float mx_s[2 * kMaxActions], sum_s[2 * kMaxActions];
    __shared__ float mxt_s[1], sumt_s[1];
    __shared__ double qn[kMaxActions];
    __shared__ float ce_s[kMaxActions];
    __shared__ float red[kThreads];
    __shared__ int best_s;
    __shared__ bool last_s;
    const int b = blockIdx.x, t = threadIdx.x, N = a.n_atoms, A = a.n_actions, AN = A * N;
    const int act = a.actions[b];
    const bool valid = rlx::taken_action_valid(act, A, t, a.status);
    const float *vo = a.online.v + (size_t)b * a.online.ld_v, *xo = a.online.x + (size_t)b * a.online.ld_x;
    float *pn = p_s, *po = p_s + AN;

    rlx::dfp_merge_row(a.online_next.v + (size_t)b * a.online_next.ld_v,
                       a.online_next.x + (size_t)b * a.online_next.ld_x, A, N, pn, t, kThreads);
    rlx::dfp_merge_row(vo, xo, A, N, po, t, kThreads);
    if (t < N) z_s[t] = a.z[t];
    __syncthreads();
    softmax_rows<kThreads>(p_s, mx_s, sum_s, 2 * A, N, t);

    // Double DQN (rainbow_dqn_agent.py:91-92): a*_b = argmax_a of the ONLINE network's fp64 expectations on s'
    if (t < A) qn[t] = expectation(pn + t * N, z_s, N);
    __syncthreads();
    if (t == 0) {
        const int best = rlx::first_argmax_f64(qn, A);
        best_s = best;
        if (a.target_actions_out) a.target_actions_out[b] = best;
    }
    __syncthreads();

    // the TARGET network's distribution on s' at a*
    rlx::dfp_merge_row(a.target_next.v + (size_t)b * a.target_next.ld_v,
                       a.target_next.x + (size_t)b * a.target_next.ld_x, A, N, pn, t, kThreads);
    __syncthreads();
    float *pt = pn + best_s * N;
    softmax_rows<kThreads>(pt, mxt_s, sumt_s, 1, N, t);

    // the projection (rainbow_dqn_agent.py:109-119), fp64: numpy forms (bootstrap * discount ** n) * z_j, then adds the
    // fp64 returns.  game_over is not read: the last n transitions of an episode do not bootstrap whatever it says.
    if (t < N)
        rlx::project_scatter(z_s, N, t, a.returns[b], (a.bootstrap[b] ? 1.0 : 0.0) * a.discount_n, (double)pt[t], l_s,
                             u_s, wl_s, wu_s);
    __syncthreads();
    if (t < N) {
        const double acc = rlx::project_gather(N, t, l_s, u_s, wl_s, wu_s);
        m_s[t] = (float)acc;                       // rounded to fp32 once (the fp32 target array)
        if (a.m_out) a.m_out[(size_t)b * N + t] = (float)acc;
    }
    __syncthreads();

    // softmax_cross_entropy_with_logits per action against the label (m on the taken action, the online softmax itself
    // elsewhere), dy = grad_scale * (p - m) on the taken action and exactly 0 elsewhere, and dy carried back through
    // the merge in rlx_dueling_combine_backward's arithmetic per atom: s = 0.f, += dy[a][j] for a ascending; dv[j] = s;
    // dx[a][j] = dy[a][j] - s / (float)A.  Thread j owns atom j of every action.
    rlx::dfp_merge_row(vo, xo, A, N, pn, t, kThreads);      // thread j writes and reads column j only: no barrier
    if (t < N) {
        float *dvr = a.dv + (size_t)b * a.ld_dv, *dxr = a.dx + (size_t)b * a.ld_dx;
        float s = 0.f;
        for (int k = 0; k < A; ++k) {
            const int c = k * N + t;
            const bool taken = valid && k == act;
            const float y = pn[c];
            const float label = taken ? m_s[t] : po[c];
            const float g = taken ? a.grad_scale * (po[c] - label) : 0.f;
            pn[c] = label * (logf(sum_s[A + k]) - (y - mx_s[A + k]));
            po[c] = g;
            s += g;
            if (a.merged_out) a.merged_out[(size_t)b * AN + c] = y;
            if (a.dlogits_out) a.dlogits_out[(size_t)b * AN + c] = g;
        }
        dvr[t] = s;
        const float mean = s / (float)A;
        for (int k = 0; k < A; ++k) dxr[k * N + t] = po[k * N + t] - mean;
    }
    __syncthreads();
    if (t < A) {
        const float *r = pn + t * N;
        float s = 0.f;
        for (int j = 0; j < N; ++j) s += r[j];
        ce_s[t] = s;
        if (a.action_losses_out) a.action_losses_out[(size_t)b * A + t] = s;
    }
    __syncthreads();
    // total_loss = reduce_sum over batch AND actions, as C51's: the row's actions in order, then the row partials in a
    // fixed tree by the workgroup that draws the last ticket
    float row = 0.f;
    if (t == 0) {
        for (int k = 0; k < A; ++k) row += ce_s[k];
        if (a.per_errors) a.per_errors[b] = valid ? (double)ce_s[act] : 0.0;
    }
    if (!rlx::ticketed_batch_sum<kThreads>(row, b, a.batch, a.row_partials, a.ticket, red, &last_s, t)) return;
    if (t == 0) a.loss[0] = red[0];
}

__global__ void __launch_bounds__(64) rainbow_egreedy_kernel(const float *__restrict__ v, long long ld_v,
                                                             const float *__restrict__ x, long long ld_x,
                                                             const double *__restrict__ z, int n_atoms,
                                                             const double *__restrict__ explore_u,
                                                             const int *__restrict__ random_act,
                                                             const double *__restrict__ tie_rand, double epsilon,
                                                             int n_actions, double *__restrict__ q_out,
                                                             int *__restrict__ actions) {
    __shared__ double q[kMaxActions];
    const int e = blockIdx.x, t = threadIdx.x, A = n_actions;
    rlx::categorical_act_q<true>(v + (size_t)e * ld_v, x + (size_t)e * ld_x, z, n_atoms, A, e, t, q_out, q);
    if (t == 0)
        actions[e] = rlx::egreedy_choice_f64(q, A, explore_u[e], random_act[e], tie_rand + (size_t)e * A, epsilon);
}

__global__ void __launch_bounds__(64) rainbow_argmax_kernel(const float *__restrict__ v, long long ld_v,
                                                            const float *__restrict__ x, long long ld_x,
                                                            const double *__restrict__ z, int n_atoms, int n_actions,
                                                            double *__restrict__ q_out, int *__restrict__ actions) {
    __shared__ double q[kMaxActions];
    const int e = blockIdx.x, t = threadIdx.x, A = n_actions;
    rlx::categorical_act_q<true>(v + (size_t)e * ld_v, x + (size_t)e * ld_x, z, n_atoms, A, e, t, q_out, q);
    if (t == 0) actions[e] = rlx::first_argmax_f64(q, A);
}

int check_act_shape(const char *fn, int n_env, int n_atoms, int n_actions, long long ld_v, long long ld_x) {
    RLX_REQUIRE(n_env > 0 && n_atoms >= 2 && n_atoms <= kMaxAtoms && n_actions > 0 && n_actions <= kMaxActions &&
                    ld_v >= n_atoms && ld_x >= (long long)n_atoms * n_actions,
                "%s: bad shape (2 <= atoms <= 256, actions <= 18, ld_v >= N, ld_x >= A*N)", fn);
    return RLX_OK;
}

}  // namespace

extern "C" {

int rlx_rainbow_head_loss(const float *v, long long ld_v, const float *x, long long ld_x, const float *v_next_target,
                          long long ld_v_next_target, const float *x_next_target, long long ld_x_next_target,
                          const float *v_next_online, long long ld_v_next_online, const float *x_next_online,
                          long long ld_x_next_online, const double *z, const int *actions,
                          const double *n_step_returns, const unsigned char *bootstrap, double discount_n, int n_atoms,
                          int n_actions, int batch, float grad_scale, float *dv, long long ld_dv, float *dx,
                          long long ld_dx, double *per_errors, float *row_partials, unsigned int *ticket,
                          float *loss_scalar, int *status, float *m_out, int *target_actions_out,
                          float *action_losses_out, float *merged_logits_out, float *dlogits_out, void *stream) {
    RLX_REQUIRE(v && x && v_next_target && x_next_target && v_next_online && x_next_online && z && actions &&
                    n_step_returns && bootstrap && dv && dx && row_partials && ticket && loss_scalar && status,
                "rlx_rainbow_head_loss: null pointer");
    if (const int rc = rlx::check_head_loss_shape("rlx_rainbow_head_loss", 2, n_atoms, n_actions, batch, ld_x,
                                                  ld_x_next_target, ld_x_next_online))
        return rc;
    RLX_REQUIRE(ld_dx >= (long long)n_atoms * n_actions && ld_v >= n_atoms && ld_v_next_target >= n_atoms &&
                    ld_v_next_online >= n_atoms && ld_dv >= n_atoms,
                "rlx_rainbow_head_loss: leading dimension < N (value stream) or < A*N (advantage gradient)");
    RainbowArgs a;
    a.online = {v, ld_v, x, ld_x};
    a.target_next = {v_next_target, ld_v_next_target, x_next_target, ld_x_next_target};
    a.online_next = {v_next_online, ld_v_next_online, x_next_online, ld_x_next_online};
    a.z = z; a.actions = actions; a.returns = n_step_returns; a.bootstrap = bootstrap; a.discount_n = discount_n;
    a.n_atoms = n_atoms; a.n_actions = n_actions; a.batch = batch; a.grad_scale = grad_scale;
    a.dv = dv; a.ld_dv = ld_dv; a.dx = dx; a.ld_dx = ld_dx; a.per_errors = per_errors; a.row_partials = row_partials;
    a.ticket = ticket; a.loss = loss_scalar; a.status = status; a.m_out = m_out;
    a.target_actions_out = target_actions_out; a.action_losses_out = action_losses_out;
    a.merged_out = merged_logits_out; a.dlogits_out = dlogits_out;
    RLX_LAUNCH((rainbow_head_loss_kernel), batch, kThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_rainbow_egreedy(const float *v, long long ld_v, const float *x, long long ld_x, const double *z, int n_atoms,
                        const double *explore_uniforms, const int *random_actions, const double *tie_break_uniforms,
                        double epsilon, int n_env, int n_actions, double *q_out, int *actions, void *stream) {
    RLX_REQUIRE(v && x && z && explore_uniforms && random_actions && tie_break_uniforms && actions,
                "rlx_rainbow_egreedy: null pointer");
    if (const int rc = check_act_shape("rlx_rainbow_egreedy", n_env, n_atoms, n_actions, ld_v, ld_x)) return rc;
    RLX_LAUNCH((rainbow_egreedy_kernel), n_env, 64, 0, rlx::as_stream(stream), v, ld_v, x, ld_x, z, n_atoms,
               explore_uniforms, random_actions, tie_break_uniforms, epsilon, n_actions, q_out, actions);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_rainbow_argmax(const float *v, long long ld_v, const float *x, long long ld_x, const double *z, int n_atoms,
                       int n_env, int n_actions, double *q_out, int *actions, void *stream) {
    RLX_REQUIRE(v && x && z && actions, "rlx_rainbow_argmax: null pointer");
    if (const int rc = check_act_shape("rlx_rainbow_argmax", n_env, n_atoms, n_actions, ld_v, ld_x)) return rc;
    RLX_LAUNCH((rainbow_argmax_kernel), n_env, 64, 0, rlx::as_stream(stream), v, ld_v, x, ld_x, z, n_atoms, n_actions,
               q_out, actions);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
