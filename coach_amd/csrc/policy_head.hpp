// The row arithmetic of the discrete PolicyHead (architectures/tensorflow_components/heads/policy_head.py:75-100), shared
// by rlx_pg_head_loss (policy_gradient.hip) and rlx_a3c_window_loss (a3c.hip): one definition, so the two launches give
// the same bits for the same logits, action and advantage.  tests/pg_ref.py (head_rows, head_loss) is the restatement.
// Needs -ffp-contract=off (no fused multiply-add) in the file that includes it.
#pragma once
#include "distributional_head.hpp"

namespace rlx {

constexpr int kPgThreads = 256;
constexpr int kPgMaxActions = kDistMaxActions;
constexpr float kPgEps = 1.1920928955078125e-07f;   // np.finfo(np.float32).eps (rl_coach/utils.py: eps)

// The project's ONE softmax over a row of action logits (as csrc/c51.hip defines it), fp32: mx = max z,
// e_j = (float)exp((double)(z_j - mx)), s = sum e_j in index order, p_j = e_j / s.  Shared by pg_row below and by the
// classification head and BCQ's imitation selector (imitation.hip), so a network's predict and the selector's
// familiarity are the same bits.  mx and s are handed back for log p_j = (z_j - mx) - log s.
__device__ __forceinline__ void softmax_row(const float *x, int A, float *p, float &mx_out, float &s_out) {
    float mx = x[0];
    for (int j = 1; j < A; ++j) mx = fmaxf(mx, x[j]);
    float s = 0.f;
    for (int j = 0; j < A; ++j) {
        p[j] = (float)exp((double)(x[j] - mx));
        s += p[j];
    }
    for (int j = 0; j < A; ++j) p[j] = p[j] / s;
    mx_out = mx;
    s_out = s;
}

// p = softmax_row(z), q = p + eps, S = sum q (index order), log pi = log q - log S with
// log x = (float)log((double)x), H = -sum (q / S) * log pi.  All fp32.
struct PgRow {
    float p[kPgMaxActions], q[kPgMaxActions], lp[kPgMaxActions];
    float S, H;
};

__device__ __forceinline__ void pg_row(const float *x, int A, PgRow &r) {
    float mx, s;
    softmax_row(x, A, r.p, mx, s);
    float S = 0.f;
    for (int j = 0; j < A; ++j) {
        r.q[j] = r.p[j] + kPgEps;
        S += r.q[j];
    }
    const float logS = (float)log((double)S);
    float h = 0.f;
    for (int j = 0; j < A; ++j) {
        r.lp[j] = (float)log((double)r.q[j]) - logS;
        h += (r.q[j] / S) * r.lp[j];
    }
    r.S = S;
    r.H = -h;
}

// One valid row of a window of T rows (fT = (float)T): adds log pi(act) * adv onto pol and H onto ent, writes dz[0 .. A).
// g_k = dL/dp_k of this row's terms -(1/T) log pi_a adv - beta (1/T) H:
//   dlog pi_a/dp_k = [k == a]/q_a - 1/S,   dH/dp_k = -(log pi_k + H)/S;   dz_j = p_j (g_j - sum_k g_k p_k)
__device__ __forceinline__ void pg_row_loss_grad(const float *x, int A, int act, float adv, float beta, float fT,
                                                 float *dz, float &pol, float &ent) {
    PgRow r;
    pg_row(x, A, r);
    pol += r.lp[act] * adv;
    ent += r.H;
    const float cp = adv / fT, ce = beta / fT;
    float g[kPgMaxActions];
    float dot = 0.f;
    for (int k = 0; k < A; ++k) {
        const float dlog = (k == act ? 1.f / r.q[k] : 0.f) - 1.f / r.S;
        g[k] = ce * ((r.lp[k] + r.H) / r.S) - cp * dlog;
        dot += g[k] * r.p[k];
    }
    for (int j = 0; j < A; ++j) dz[j] = r.p[j] * (g[j] - dot);
}

}  // namespace rlx
