// Actor-Critic (A3C) on gfx950: everything between the forward and the backward pass of one update window, one launch.
//
// Replaces, in the reference (paths under rl_coach/):
//   * ActorCriticAgent.learn_from_batch's targets (A_VALUE, GAE)        agents/actor_critic_agent.py:108-125, 138-165
//   * VHead's loss (MSE under loss_weight)                               .../heads/head.py:170-181
//   * PolicyHead, discrete branch (loss, entropy regularisation)         .../heads/policy_head.py:75-100 (policy_head.hpp)
//   * PolicyHead, continuous branch (Box action spaces)                  .../heads/policy_head.py:102-146 (gaussian_policy_head.hpp)
//     (... = architectures/tensorflow_components)
//
// A latency-bound row kernel over a few to a few hundred rows: ONE workgroup, so the reverse recurrence has the
// reference's order, every batch sum has a fixed order and there are no float atomics.  Neither V nor the targets leave
// the device: a window is forward, this launch, backward.  tests/a3c_ref.py is the numpy restatement; it states every
// fp32 / fp64 rounding point named here.  Compiled with -ffp-contract=off so the fp64 arithmetic rounds like numpy.
#include "a3c_targets.hpp"
#include "gaussian_policy_head.hpp"

namespace {

constexpr int kThreads = rlx::kPgThreads;

struct A3cArgs {
    rlx::A3cWindow w;               // V, the rewards and the flag; the targets, the advantages and dV (a3c_targets.hpp)
    const float *logits;            // [rows][ld]
    long long ld;
    const int *actions;             // [T]
    int A;
    float beta;
    float *dlogits;                 // [rows][ld_d]
    long long ld_d;
    float *scalars;                 // [4]: total loss, value loss, policy loss, mean entropy
};

__global__ void __launch_bounds__(kThreads) a3c_window_loss_kernel(const A3cArgs a) {
    __shared__ double r_s[kThreads], v_s[kThreads], x_s[kThreads];
    __shared__ float val_s[kThreads], pol_s[kThreads], ent_s[kThreads];
    const rlx::A3cWindow &w = a.w;
    const int t = threadIdx.x, T = w.T, A = a.A;
    if (!rlx::a3c_window_targets(w, r_s, v_s, x_s)) return;
    // the two heads, one row per thread: thread t owns rows t, t + 256, ... (it wrote their targets itself) and adds
    // their terms in row order
    const float fT = (float)T;
    float val = 0.f, pol = 0.f, ent = 0.f;
    for (int b = t; b < w.rows; b += kThreads) {
        float *d = a.dlogits + (size_t)b * a.ld_d;
        if (b >= T) {                                              // the bootstrap row: zero gradient, no term
            w.dV[(size_t)b * w.ld_dv] = 0.f;
            for (int j = 0; j < A; ++j) d[j] = 0.f;
            continue;
        }
        const float adv = rlx::a3c_value_row(w, b, fT, val);
        const int act = a.actions[b];
        if (!rlx::taken_action_valid(act, A, 0, w.status)) {
            for (int j = 0; j < A; ++j) d[j] = 0.f;
            continue;
        }
        rlx::pg_row_loss_grad(a.logits + (size_t)b * a.ld, A, act, adv, a.beta, fT, d, pol, ent);
    }
    rlx::tree_sum(kThreads, val_s, val, pol_s, pol, ent_s, ent);
    if (t == 0) rlx::a3c_write_scalars(val_s[0], pol_s[0], ent_s[0], fT, a.beta, a.scalars);
}

struct A3cContinuousArgs {
    rlx::A3cWindow w;
    rlx::GaussianHead h;            // the continuous PolicyHead's buffers (gaussian_policy_head.hpp)
    float beta;
    float *scalars;                 // [4]
};

// The window's targets as above, then the rows in chunks of 256 through the head's LDS tiles (gaussian_head_chunk):
// thread t owns rows t, t + 256, ... here too, and adds their terms in row order.
__global__ void __launch_bounds__(kThreads) a3c_continuous_window_loss_kernel(const A3cContinuousArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tiles[];
    __shared__ double r_s[kThreads], v_s[kThreads], x_s[kThreads];
    __shared__ float val_s[kThreads], pol_s[kThreads], ent_s[kThreads];
    const rlx::A3cWindow &w = a.w;
    const int t = threadIdx.x, T = w.T;
    if (!rlx::a3c_window_targets(w, r_s, v_s, x_s)) return;
    const float fT = (float)T;
    float val = 0.f, pol = 0.f, ent = 0.f;
    float adv = 0.f;                                               // of the thread's row in the current chunk
    for (int r0 = 0; r0 < w.rows; r0 += kThreads) {
        const int b = r0 + t;
        if (b < T) adv = rlx::a3c_value_row(w, b, fT, val);
        else if (b < w.rows) w.dV[(size_t)b * w.ld_dv] = 0.f;      // the bootstrap row: zero gradient, no term
        rlx::gaussian_head_chunk(a.h, tiles, r0, w.rows, T, a.beta, fT, [adv](int) { return adv; }, pol, ent);
    }
    rlx::tree_sum(kThreads, val_s, val, pol_s, pol, ent_s, ent);
    if (t == 0) rlx::a3c_write_scalars(val_s[0], pol_s[0], ent_s[0], fT, a.beta, a.scalars);
}

}  // namespace

extern "C" {

int rlx_a3c_window_loss(const float *V, long long ld_v, const float *logits, long long ld, const int *actions,
                        const float *rewards, const unsigned char *game_over, int T, int rows, int n_actions,
                        double discount, double gae_lambda, int rescaler, int estimate_state_value_using_gae,
                        float beta_entropy, float v_loss_weight, double *targets_out, double *advantages_out, float *dV,
                        long long ld_dv, float *dlogits, long long ld_dlogits, float *scalars, int *status,
                        void *stream) {
    const rlx::A3cWindow w{V, ld_v, rewards, game_over, T, rows, discount, gae_lambda, rescaler,
                           estimate_state_value_using_gae != 0, v_loss_weight, targets_out, advantages_out, dV, ld_dv,
                           status};
    if (int rc = rlx::check_a3c_window("rlx_a3c_window_loss", w, scalars)) return rc;
    RLX_REQUIRE(logits && actions && dlogits, "rlx_a3c_window_loss: null pointer");
    RLX_REQUIRE(n_actions >= 1 && n_actions <= rlx::kPgMaxActions,
                "rlx_a3c_window_loss: unsupported sizes (1 <= actions=%d <= 18)", n_actions);
    RLX_REQUIRE(ld >= n_actions && ld_dlogits >= n_actions, "rlx_a3c_window_loss: leading dimension < A");
    A3cArgs a{w, logits, ld, actions, n_actions, beta_entropy, dlogits, ld_dlogits, scalars};
    RLX_LAUNCH((a3c_window_loss_kernel), 1, kThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_a3c_continuous_window_loss(const float *V, long long ld_v, const float *mean_pre, long long ld_m,
                                   const float *std_pre, long long ld_s, const float *std, const float *scale,
                                   const float *actions, const float *rewards, const unsigned char *game_over, int T,
                                   int rows, int action_dim, double discount, double gae_lambda, int rescaler,
                                   int estimate_state_value_using_gae, float beta_entropy, float v_loss_weight,
                                   double *targets_out, double *advantages_out, float *dV, long long ld_dv,
                                   float *dmean_pre, long long ld_dm, float *dstd_pre, long long ld_ds, float *scalars,
                                   int *status, void *stream) {
    const char *fn = "rlx_a3c_continuous_window_loss";
    const rlx::A3cWindow w{V, ld_v, rewards, game_over, T, rows, discount, gae_lambda, rescaler,
                           estimate_state_value_using_gae != 0, v_loss_weight, targets_out, advantages_out, dV, ld_dv,
                           status};
    const rlx::GaussianHead h{mean_pre, ld_m, std_pre, ld_s, std, scale, actions, action_dim, dmean_pre, ld_dm, dstd_pre,
                              ld_ds};
    if (int rc = rlx::check_a3c_window(fn, w, scalars)) return rc;
    if (int rc = rlx::check_gaussian_head(fn, h)) return rc;
    const size_t lds = rlx::gaussian_tiles_bytes(action_dim);
    RLX_HIP(rlx::allow_lds<a3c_continuous_window_loss_kernel>(lds));
    A3cContinuousArgs a{w, h, beta_entropy, scalars};
    RLX_LAUNCH((a3c_continuous_window_loss_kernel), 1, kThreads, (unsigned)lds, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
