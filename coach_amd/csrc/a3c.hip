// Actor-Critic (A3C) on gfx950: everything between the forward and the backward pass of one update window, one launch.
//
// Replaces, in the reference (paths under rl_coach/):
//   * ActorCriticAgent.learn_from_batch's targets (A_VALUE, GAE)        agents/actor_critic_agent.py:108-125, 138-165
//   * VHead's loss (MSE under loss_weight)                               .../heads/head.py:170-181
//   * PolicyHead, discrete branch (loss, entropy regularisation)         .../heads/policy_head.py:75-100 (policy_head.hpp)
//     (... = architectures/tensorflow_components)
//
// A latency-bound row kernel over a few to a few hundred rows: ONE workgroup, so the reverse recurrence has the
// reference's order, every batch sum has a fixed order and there are no float atomics.  Neither V nor the targets leave
// the device: a window is forward, this launch, backward.  tests/a3c_ref.py is the numpy restatement; it states every
// fp32 / fp64 rounding point named here.  Compiled with -ffp-contract=off so the fp64 arithmetic rounds like numpy.
#include "policy_head.hpp"

namespace {

constexpr int kThreads = rlx::kPgThreads;

struct A3cArgs {
    const float *V;                 // [rows] at stride ld_v
    long long ld_v;
    const float *logits;            // [rows][ld]
    long long ld;
    const int *actions;             // [T]
    const float *rewards;           // [T]
    const unsigned char *game_over; // the last transition's flag
    int T, rows, A;
    double discount, gae_lambda;
    int rescaler, estimate_gae;
    float beta, v_weight;
    double *targets, *advantages;   // [T] out (in with RLX_A3C_TARGETS_GIVEN)
    float *dV;                      // [rows] at stride ld_dv
    long long ld_dv;
    float *dlogits;                 // [rows][ld_d]
    long long ld_d;
    float *scalars;                 // [4]: total loss, value loss, policy loss, mean entropy
    int *status;
};

__global__ void __launch_bounds__(kThreads) a3c_window_loss_kernel(const A3cArgs a) {
    // a chunk of the window: the recurrence's inputs, overwritten by its results (T-independent)
    __shared__ double r_s[kThreads], v_s[kThreads], x_s[kThreads];
    __shared__ float val_s[kThreads], pol_s[kThreads], ent_s[kThreads];
    const int t = threadIdx.x, T = a.T, A = a.A;
    // RLX_A3C_TARGETS_GIVEN: targets / advantages already hold the window's values and nothing is bootstrapped
    const bool given = a.rescaler == RLX_A3C_TARGETS_GIVEN;
    const bool terminal = given || *a.game_over != 0;
    if (!terminal && a.rows <= T) {         // the bootstrap row is missing: nothing is read or written
        if (t == 0) atomicOr(a.status, RLX_A3C_STATUS_NO_BOOTSTRAP_ROW);
        return;
    }
    const bool gae = a.rescaler == RLX_A3C_GAE;
    const float fdisc = (float)a.discount;                         // `discount * <fp32 array>`: an fp32 product
    const float v_last = terminal ? 0.f : a.V[(size_t)T * a.ld_v]; // values[-1] = 0 / R = 0 on a game over
    const double g_adv = a.discount * a.gae_lambda;
    // lane 0's carried products g * y_{i+1} of the recurrences, across chunks
    double p_adv = 0.0, p_ret = 0.0;
    if (gae) p_ret = a.discount * ((double)v_last + 0.0);          // the bootstrap-extended rewards' last element
    else p_ret = terminal ? 0.0 : (double)(fdisc * v_last);        // :152, first pass: fp32 product (a3c_ref.py)
    const int chunks = given ? 0 : (T + kThreads - 1) / kThreads;
    for (int c = chunks - 1; c >= 0; --c) {
        const int i = c * kThreads + t;
        if (i < T) {
            const double r = (double)a.rewards[i], v = (double)a.V[(size_t)i * a.ld_v];
            r_s[t] = r;
            v_s[t] = v;
            if (gae) {                                             // deltas = rewards + discount * values[1:] - values[:-1]
                const float v_next = i + 1 < T ? a.V[(size_t)(i + 1) * a.ld_v] : v_last;
                x_s[t] = (r + (double)(fdisc * v_next)) - v;
            }
        }
        __syncthreads();
        if (t == 0) {                                              // the sequential recurrence, the reference's order
            const int hi = min(T - c * kThreads, kThreads);
            for (int k = hi - 1; k >= 0; --k) {
                if (gae) {
                    const double adv = x_s[k] + p_adv;             // lfilter: y_i = x_i + g * y_{i+1}
                    p_adv = g_adv * adv;
                    double tgt;
                    if (a.estimate_gae) tgt = adv + v_s[k];
                    else {
                        tgt = r_s[k] + p_ret;
                        p_ret = a.discount * tgt;
                    }
                    x_s[k] = adv;
                    r_s[k] = tgt;
                } else {
                    const double R = r_s[k] + p_ret;               // R = r_i + discount * R
                    p_ret = a.discount * R;
                    r_s[k] = R;
                    x_s[k] = R - v_s[k];
                }
            }
        }
        __syncthreads();
        if (i < T) {
            a.targets[i] = r_s[t];
            a.advantages[i] = x_s[t];
        }
        __syncthreads();
    }
    // the two heads, one row per thread: thread t owns rows t, t + 256, ... (it wrote their targets itself) and adds
    // their terms in row order; the workgroup sums the 256 partials in a fixed tree
    const float fT = (float)T;
    float val = 0.f, pol = 0.f, ent = 0.f;
    for (int b = t; b < a.rows; b += kThreads) {
        float *d = a.dlogits + (size_t)b * a.ld_d;
        if (b >= T) {                                              // the bootstrap row: zero gradient, no term
            a.dV[(size_t)b * a.ld_dv] = 0.f;
            for (int j = 0; j < A; ++j) d[j] = 0.f;
            continue;
        }
        // the fp32 casts of the heads' placeholders
        const float tgt = (float)a.targets[b], adv = (float)a.advantages[b];
        const float dv = a.V[(size_t)b * a.ld_v] - tgt;
        val += a.v_weight * (dv * dv);
        a.dV[(size_t)b * a.ld_dv] = (a.v_weight * (2.f * dv)) / fT;
        const int act = a.actions[b];
        if (!rlx::taken_action_valid(act, A, 0, a.status)) {
            for (int j = 0; j < A; ++j) d[j] = 0.f;
            continue;
        }
        rlx::pg_row_loss_grad(a.logits + (size_t)b * a.ld, A, act, adv, a.beta, fT, d, pol, ent);
    }
    val_s[t] = val;
    pol_s[t] = pol;
    ent_s[t] = ent;
    __syncthreads();
    for (int s = kThreads >> 1; s > 0; s >>= 1) {
        if (t < s) {
            val_s[t] += val_s[t + s];
            pol_s[t] += pol_s[t + s];
            ent_s[t] += ent_s[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        const float value_loss = val_s[0] / fT, policy_loss = -(pol_s[0] / fT), mean_h = ent_s[0] / fT;
        a.scalars[0] = value_loss + (policy_loss - a.beta * mean_h);
        a.scalars[1] = value_loss;
        a.scalars[2] = policy_loss;
        a.scalars[3] = mean_h;
    }
}

}  // namespace

extern "C" {

int rlx_a3c_window_loss(const float *V, long long ld_v, const float *logits, long long ld, const int *actions,
                        const float *rewards, const unsigned char *game_over, int T, int rows, int n_actions,
                        double discount, double gae_lambda, int rescaler, int estimate_state_value_using_gae,
                        float beta_entropy, float v_loss_weight, double *targets_out, double *advantages_out, float *dV,
                        long long ld_dv, float *dlogits, long long ld_dlogits, float *scalars, int *status,
                        void *stream) {
    RLX_REQUIRE(V && logits && actions && targets_out && advantages_out && dV && dlogits && scalars && status &&
                    (rescaler == RLX_A3C_TARGETS_GIVEN || (rewards && game_over)),
                "rlx_a3c_window_loss: null pointer");
    RLX_REQUIRE(n_actions >= 1 && n_actions <= rlx::kPgMaxActions && T >= 1 && (rows == T || rows == T + 1),
                "rlx_a3c_window_loss: unsupported sizes (1 <= actions=%d <= 18, 1 <= T=%d, rows=%d is T or T + 1)",
                n_actions, T, rows);
    RLX_REQUIRE(ld >= n_actions && ld_dlogits >= n_actions && ld_v >= 1 && ld_dv >= 1,
                "rlx_a3c_window_loss: leading dimension < A (or < 1 for V)");
    RLX_REQUIRE(rescaler == RLX_A3C_A_VALUE || rescaler == RLX_A3C_GAE || rescaler == RLX_A3C_TARGETS_GIVEN,
                "rlx_a3c_window_loss: the policy gradient rescaler %d is neither A_VALUE nor GAE", rescaler);
    A3cArgs a{V, ld_v, logits, ld, actions, rewards, game_over, T, rows, n_actions, discount, gae_lambda, rescaler,
              estimate_state_value_using_gae != 0, beta_entropy, v_loss_weight, targets_out, advantages_out, dV, ld_dv,
              dlogits, ld_dlogits, scalars, status};
    RLX_LAUNCH((a3c_window_loss_kernel), 1, kThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
