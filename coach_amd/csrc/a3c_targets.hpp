// The value targets and advantages of one Actor-Critic update window (ActorCriticAgent.learn_from_batch,
// agents/actor_critic_agent.py:108-125, 138-165) and the V head's row term (heads/head.py:170-181), shared by
// rlx_a3c_window_loss and rlx_a3c_continuous_window_loss (a3c.hip): one definition, so the discrete and the continuous
// window give the same bits for the same V, rewards and flag.  tests/a3c_ref.py is the numpy restatement; it states
// every fp32 / fp64 rounding point named here.  Needs -ffp-contract=off in the file that includes it.
#pragma once
#include "policy_head.hpp"

namespace rlx {

struct A3cWindow {
    const float *V;                 // [rows] at stride ld_v
    long long ld_v;
    const float *rewards;           // [T]
    const unsigned char *game_over; // the last transition's flag
    int T, rows;
    double discount, gae_lambda;
    int rescaler, estimate_gae;
    float v_weight;
    double *targets, *advantages;   // [T] out (in with RLX_A3C_TARGETS_GIVEN)
    float *dV;                      // [rows] at stride ld_dv
    long long ld_dv;
    int *status;
};

// Fills targets / advantages [T] (or leaves them, RLX_A3C_TARGETS_GIVEN): thread t writes entries t, t + 256, ...,
// the rows it owns in the heads' pass behind this.  r_s / v_s / x_s: kPgThreads doubles of LDS each, a chunk of the
// window: the recurrence's inputs, overwritten by its results (T-independent).  Every thread of the workgroup calls it
// (barriers inside).  false: the bootstrap row is missing, the status bit is set and nothing was read or written.
__device__ __forceinline__ bool a3c_window_targets(const A3cWindow &a, double *r_s, double *v_s, double *x_s) {
    constexpr int kThreads = kPgThreads;
    const int t = threadIdx.x, T = a.T;
    // RLX_A3C_TARGETS_GIVEN: targets / advantages already hold the window's values and nothing is bootstrapped
    const bool given = a.rescaler == RLX_A3C_TARGETS_GIVEN;
    const bool terminal = given || *a.game_over != 0;
    if (!terminal && a.rows <= T) {         // the bootstrap row is missing: nothing is read or written
        if (t == 0) atomicOr(a.status, RLX_A3C_STATUS_NO_BOOTSTRAP_ROW);
        return false;
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
    return true;
}

// The V head on row b of the window (b < T, a row the calling thread owns): adds its loss term onto val, writes dV_b
// -> the row's advantage, rounded to fp32 once (the policy head's placeholder)
__device__ __forceinline__ float a3c_value_row(const A3cWindow &a, int b, float fT, float &val) {
    // the fp32 casts of the heads' placeholders
    const float tgt = (float)a.targets[b], adv = (float)a.advantages[b];
    const float dv = a.V[(size_t)b * a.ld_v] - tgt;
    val += a.v_weight * (dv * dv);
    a.dV[(size_t)b * a.ld_dv] = (a.v_weight * (2.f * dv)) / fT;
    return adv;
}

// thread 0, after tree_sum of the three partials: the window's four scalars
__device__ __forceinline__ void a3c_write_scalars(float val_sum, float pol_sum, float ent_sum, float fT, float beta,
                                                  float *scalars) {
    const float value_loss = val_sum / fT, policy_loss = -(pol_sum / fT), mean_h = ent_sum / fT;
    scalars[0] = value_loss + (policy_loss - beta * mean_h);
    scalars[1] = value_loss;
    scalars[2] = policy_loss;
    scalars[3] = mean_h;
}

// Host: the checks of the window's own arguments, shared by the two entry points.
inline int check_a3c_window(const char *fn, const A3cWindow &a, const float *scalars) {
    RLX_REQUIRE(a.V && a.targets && a.advantages && a.dV && scalars && a.status &&
                    (a.rescaler == RLX_A3C_TARGETS_GIVEN || (a.rewards && a.game_over)),
                "%s: null pointer", fn);
    RLX_REQUIRE(a.T >= 1 && (a.rows == a.T || a.rows == a.T + 1), "%s: unsupported sizes (1 <= T=%d, rows=%d is T or T + 1)",
                fn, a.T, a.rows);
    RLX_REQUIRE(a.ld_v >= 1 && a.ld_dv >= 1, "%s: leading dimension < 1 for V", fn);
    RLX_REQUIRE(a.rescaler == RLX_A3C_A_VALUE || a.rescaler == RLX_A3C_GAE || a.rescaler == RLX_A3C_TARGETS_GIVEN,
                "%s: the policy gradient rescaler %d is neither A_VALUE nor GAE", fn, a.rescaler);
    return RLX_OK;
}

}  // namespace rlx
