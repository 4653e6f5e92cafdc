// Categorical DQN (C51) on gfx950: the head's projection, cross entropy + gradient and the acting reduction.
//
// Replaces, in the reference (paths under rl_coach/):
//   * CategoricalDQNAgent.learn_from_batch          agents/categorical_dqn_agent.py:104-167 (target action, the
//                                                   projection of the shifted support onto the atoms)
//   * CategoricalQHead                              architectures/tensorflow_components/heads/categorical_q_head.py:42-58
//                                                   (softmax over the atoms, softmax_cross_entropy_with_logits, q_values)
//   * distribution_prediction_to_q_values + EGreedy.get_action   categorical_dqn_agent.py:86-87,
//                                                   exploration_policies/e_greedy.py:84-101
//
// logits is the head's Dense output [B, A*N]: column a*N + j is atom j of action a.  Both kernels use ONE softmax, defined
// so that a numpy restatement reproduces it bit for bit (tests/c51_ref.py):
//   mx = max_j x_j;  e_j = (float)exp((double)(x_j - mx));  s = sum_{j = 0 .. N-1, in this order} e_j (fp32);  p_j = e_j / s
// (an fp64 exp rounded once is the correctly rounded fp32 exp but for double-rounding cases of probability ~2^-29).
// The Q value of an action is fp64: q = sum_{j ascending} (double)p_j * z_j, z the host's np.linspace (numpy's dot may
// associate differently: a few ulp).  Compiled with -ffp-contract=off so the fp64 arithmetic rounds like numpy.
#include "categorical_head.hpp"

namespace {

constexpr int kC51Threads = rlx::kDistLossThreads;
constexpr int kC51MaxAtoms = rlx::kDistLossThreads;   // one thread per atom
constexpr int kC51MaxActions = rlx::kDistMaxActions;

using rlx::expectation;
using rlx::softmax_rows;

struct C51Args {
    const float *logits;        // online output on s [B, ld_logits]
    long long ld_logits;
    const float *logits_next;   // target output on s' [B, ld_next]
    long long ld_next;
    const double *z;            // [N] support
    const int *actions;
    const float *rewards;
    const unsigned char *game_overs;
    double discount;
    int n_atoms, n_actions, batch;
    float grad_scale;
    float *dlogits;             // [B, ld_dlogits]
    long long ld_dlogits;
    double *per_errors;         // [B] or null: the taken action's cross entropy
    float *row_partials;        // [B] workspace
    unsigned int *ticket;       // one zero-initialised word, left at zero
    float *loss;
    int *status;
    float *m_out;               // [B, N] or null
    int *target_actions_out;    // [B] or null
    float *action_losses_out;   // [B, A] or null
};

// One workgroup per batch row b.  LDS holds the row's 2A distributions (target on s' first, then online on s).
__global__ void __launch_bounds__(kC51Threads) c51_head_loss_kernel(const C51Args a) {
    __shared__ float p_s[2 * kC51MaxActions * kC51MaxAtoms];
    __shared__ double z_s[kC51MaxAtoms];
    __shared__ double wl_s[kC51MaxAtoms], wu_s[kC51MaxAtoms];   // p'[a*, j] * (u - bj), p'[a*, j] * (bj - l)
    __shared__ int l_s[kC51MaxAtoms], u_s[kC51MaxAtoms];
    __shared__ float m_s[kC51MaxAtoms];
    __shared__ float mx_s[2 * kC51MaxActions], sum_s[2 * kC51MaxActions];
    __shared__ double qn[kC51MaxActions];
    __shared__ float ce_s[kC51MaxActions];
    __shared__ float red[kC51Threads];
    __shared__ int best_s;
    __shared__ bool last_s;
    const int b = blockIdx.x, t = threadIdx.x, N = a.n_atoms, A = a.n_actions, AN = A * N;
    const int act = a.actions[b];
    const bool valid = rlx::taken_action_valid(act, A, t, a.status);
    const float *xn = a.logits_next + (size_t)b * a.ld_next;
    const float *xo = a.logits + (size_t)b * a.ld_logits;
    float *pn = p_s, *po = p_s + AN;

    for (int c = t; c < AN; c += kC51Threads) {
        pn[c] = xn[c];
        po[c] = xo[c];
    }
    if (t < N) z_s[t] = a.z[t];
    __syncthreads();
    softmax_rows<kC51Threads>(p_s, mx_s, sum_s, 2 * A, N, t);

    // a*_b = argmax_a of the TARGET network's fp64 expectations
    if (t < A) qn[t] = expectation(pn + t * N, z_s, N);
    __syncthreads();
    if (t == 0) {
        const int best = rlx::first_argmax_f64(qn, A);
        best_s = best;
        if (a.target_actions_out) a.target_actions_out[b] = best;
    }
    __syncthreads();

    // the projection (categorical_dqn_agent.py:141-149), fp64.  Thread j forms atom j's two contributions ...
    if (t < N)
        rlx::project_scatter(z_s, N, t, (double)a.rewards[b], (1.0 - (a.game_overs[b] ? 1.0 : 0.0)) * a.discount,
                             (double)pn[best_s * N + t], l_s, u_s, wl_s, wu_s);
    __syncthreads();
    // ... and thread k, which owns output atom k, adds them in the reference's order (categorical_head.hpp); rounded to
    // fp32 once (the fp32 target array).
    if (t < N) {
        const double acc = rlx::project_gather(N, t, l_s, u_s, wl_s, wu_s);
        m_s[t] = (float)acc;
        if (a.m_out) a.m_out[(size_t)b * N + t] = (float)acc;
    }
    __syncthreads();

    // softmax_cross_entropy_with_logits per action: sum_j label_j * (log(sum) - (x_j - mx)), fp32.  The label of the
    // taken action is m, that of every other action the online softmax itself (its entropy; zero gradient).
    // dlogits = softmax - labels, as TensorFlow's fused op has it (not scaled by sum(labels)).
    float *term = pn;               // the target distributions are no longer needed
    float *drow = a.dlogits + (size_t)b * a.ld_dlogits;
    for (int c = t; c < AN; c += kC51Threads) {
        const int k = c / N;
        const bool taken = valid && k == act;
        const float label = taken ? m_s[c - k * N] : po[c];
        term[c] = label * (logf(sum_s[A + k]) - (xo[c] - mx_s[A + k]));
        drow[c] = taken ? a.grad_scale * (po[c] - label) : 0.f;
    }
    __syncthreads();
    if (t < A) {
        const float *r = term + t * N;
        float s = 0.f;
        for (int j = 0; j < N; ++j) s += r[j];
        ce_s[t] = s;
        if (a.action_losses_out) a.action_losses_out[(size_t)b * A + t] = s;
    }
    __syncthreads();
    // total_loss = reduce_sum over batch AND actions: the row's actions in order, then the row partials summed in a
    // fixed tree by the workgroup that draws the last ticket
    float row = 0.f;
    if (t == 0) {
        for (int k = 0; k < A; ++k) row += ce_s[k];
        if (a.per_errors) a.per_errors[b] = valid ? (double)ce_s[act] : 0.0;
    }
    if (!rlx::ticketed_batch_sum<kC51Threads>(row, b, a.batch, a.row_partials, a.ticket, red, &last_s, t)) return;
    if (t == 0) a.loss[0] = red[0];
}

// One wave per env: categorical_act_q (categorical_head.hpp) forms the fp64 expectations, lane 0 makes the
// epsilon-greedy choice on them (distributional_head.hpp).
__global__ void __launch_bounds__(64) categorical_egreedy_kernel(const float *__restrict__ logits, long long ld,
                                                                 const double *__restrict__ z, int n_atoms,
                                                                 const double *__restrict__ explore_u,
                                                                 const int *__restrict__ random_act,
                                                                 const double *__restrict__ tie_rand, double epsilon,
                                                                 int n_actions, double *__restrict__ q_out,
                                                                 int *__restrict__ actions) {
    __shared__ double q[kC51MaxActions];
    const int e = blockIdx.x, t = threadIdx.x, A = n_actions;
    rlx::categorical_act_q<false>(nullptr, logits + (size_t)e * ld, z, n_atoms, A, e, t, q_out, q);
    if (t == 0)
        actions[e] = rlx::egreedy_choice_f64(q, A, explore_u[e], random_act[e], tie_rand + (size_t)e * A, epsilon);
}

// ParameterNoise acting (exploration_policies/parameter_noise.py:62-68): np.argmax of the same fp64 expectations — the
// first maximum, no draws.
__global__ void __launch_bounds__(64) categorical_argmax_kernel(const float *__restrict__ logits, long long ld,
                                                                const double *__restrict__ z, int n_atoms, int n_actions,
                                                                double *__restrict__ q_out, int *__restrict__ actions) {
    __shared__ double q[kC51MaxActions];
    const int e = blockIdx.x, t = threadIdx.x, A = n_actions;
    rlx::categorical_act_q<false>(nullptr, logits + (size_t)e * ld, z, n_atoms, A, e, t, q_out, q);
    if (t == 0) actions[e] = rlx::first_argmax_f64(q, A);
}

}  // namespace

extern "C" {

int rlx_c51_head_loss(const float *logits, long long ld_logits, const float *logits_next_target, long long ld_next,
                      const double *z, const int *actions, const float *rewards, const unsigned char *game_overs,
                      double discount, int n_atoms, int n_actions, int batch, float grad_scale, float *dlogits,
                      long long ld_dlogits, double *per_errors, float *row_partials, unsigned int *ticket,
                      float *loss_scalar, int *status, float *m_out, int *target_actions_out, float *action_losses_out,
                      void *stream) {
    RLX_REQUIRE(logits && logits_next_target && z && actions && rewards && game_overs && dlogits && row_partials &&
                    ticket && loss_scalar && status,
                "rlx_c51_head_loss: null pointer");
    if (const int rc = rlx::check_head_loss_shape("rlx_c51_head_loss", 2, n_atoms, n_actions, batch, ld_logits, ld_next,
                                                  ld_dlogits))
        return rc;
    C51Args a;
    a.logits = logits; a.ld_logits = ld_logits; a.logits_next = logits_next_target; a.ld_next = ld_next; a.z = z;
    a.actions = actions; a.rewards = rewards; a.game_overs = game_overs; a.discount = discount;
    a.n_atoms = n_atoms; a.n_actions = n_actions; a.batch = batch; a.grad_scale = grad_scale;
    a.dlogits = dlogits; a.ld_dlogits = ld_dlogits; a.per_errors = per_errors; a.row_partials = row_partials;
    a.ticket = ticket; a.loss = loss_scalar; a.status = status; a.m_out = m_out;
    a.target_actions_out = target_actions_out; a.action_losses_out = action_losses_out;
    RLX_LAUNCH((c51_head_loss_kernel), batch, kC51Threads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_categorical_egreedy(const float *logits, long long ld, const double *z, int n_atoms,
                            const double *explore_uniforms, const int *random_actions,
                            const double *tie_break_uniforms, double epsilon, int n_env, int n_actions, double *q_out,
                            int *actions, void *stream) {
    RLX_REQUIRE(logits && z && explore_uniforms && random_actions && tie_break_uniforms && actions,
                "rlx_categorical_egreedy: null pointer");
    RLX_REQUIRE(n_env > 0 && n_atoms >= 2 && n_atoms <= kC51MaxAtoms && n_actions > 0 && n_actions <= kC51MaxActions &&
                    ld >= (long long)n_atoms * n_actions,
                "rlx_categorical_egreedy: bad shape (2 <= atoms <= 256, actions <= 18, ld >= A*N)");
    RLX_LAUNCH((categorical_egreedy_kernel), n_env, 64, 0, rlx::as_stream(stream), logits, ld, z, n_atoms,
               explore_uniforms, random_actions, tie_break_uniforms, epsilon, n_actions, q_out, actions);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_categorical_argmax(const float *logits, long long ld, const double *z, int n_atoms, int n_env, int n_actions,
                           double *q_out, int *actions, void *stream) {
    RLX_REQUIRE(logits && z && actions, "rlx_categorical_argmax: null pointer");
    RLX_REQUIRE(n_env > 0 && n_atoms >= 2 && n_atoms <= kC51MaxAtoms && n_actions > 0 && n_actions <= kC51MaxActions &&
                    ld >= (long long)n_atoms * n_actions,
                "rlx_categorical_argmax: bad shape (2 <= atoms <= 256, actions <= 18, ld >= A*N)");
    RLX_LAUNCH((categorical_argmax_kernel), n_env, 64, 0, rlx::as_stream(stream), logits, ld, z, n_atoms, n_actions,
               q_out, actions);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
