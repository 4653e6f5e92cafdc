// The row arithmetic of the ACER agent and its policy head (agents/acer_agent.py:129-141 and
// architectures/tensorflow_components/heads/acer_policy_head.py:47-113 of the reference) on top of the discrete policy row
// of policy_head.hpp, which is included and not restated.  tests/acer_ref.py is the restatement.
// Needs -ffp-contract=off (no fused multiply-add) in the file that includes it.
#pragma once
#include "policy_head.hpp"

namespace rlx {

// np.sum over a contiguous fp32 row of n <= 18 values as numpy's add.reduce runs it (pairwise_sum, n <= 128): a plain
// loop below 8 values, else eight interleaved accumulators over the multiples of 8, folded in pairs, the rest in order.
template <typename F>
__device__ __forceinline__ float np_sum_row(F elem, int n) {
    if (n < 8) {
        float s = 0.f;
        for (int j = 0; j < n; ++j) s += elem(j);
        return s;
    }
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = elem(j);
    int i = 8;
    for (; i < n - n % 8; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += elem(i + j);
    }
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += elem(i);
    return res;
}

struct AcerRowSums {
    float prob, bias, kl, ent;
};

// One valid row of a window of T rows (fT = (float)T).  x: the row's logits; Qp(k): the aliased Q values (the retrace
// value in the taken entry); avg, rho: the average policy's probabilities and the importance weights of the row.
// Adds the row's terms onto s and writes dz[0 .. A).  g_k = dL/dp_k of the row:
//   (beta / T) (log pi_k + H) / S - (coef / T) ([k == a] / q_a - 1 / S) - (w_k / q_k) / T
//   coef = (q_retrace - V) * min(c, rho_a),  w_k = ((Q'_k - V) * relu(1 - c / (rho_k + eps))) * p_k  (p_k: stop_gradient)
// then, when asked, the trust-region layer's `grad` on g, then dz_j = p_j (g_j - sum_k g_k p_k).
template <typename QF>
__device__ __forceinline__ void acer_row_loss_grad(const float *x, int A, int act, QF Qp, const float *avg,
                                                   const float *rho, float rho_a, float q_retrace, float V, float c,
                                                   float delta, float beta, bool trust, float fT, float *dz,
                                                   AcerRowSums &s) {
    PgRow r;
    pg_row(x, A, r);
    const float adv = q_retrace - V, trunc = fminf(c, rho_a);
    s.prob += (r.lp[act] * adv) * trunc;
    s.ent += r.H;
    const float cp = (adv * trunc) / fT, ce = beta / fT;
    float g[kPgMaxActions];
    float bias = 0.f, Sa = 0.f;
    for (int k = 0; k < A; ++k) {
        const float lq = (float)log((double)r.q[k]);                  // tf.log(policy_probs + eps): not normalised
        const float dq = Qp(k) - V;
        const float f = fmaxf(1.f - c / (rho[k] + kPgEps), 0.f);
        bias += ((lq * dq) * f) * r.p[k];
        const float w = (dq * f) * r.p[k];
        const float dlog = (k == act ? 1.f / r.q[k] : 0.f) - 1.f / r.S;
        g[k] = ce * ((r.lp[k] + r.H) / r.S) - cp * dlog - (w / r.q[k]) / fT;
        Sa += avg[k] + kPgEps;
    }
    s.bias += bias;
    // KL(Categorical(avg + eps) || Categorical(p + eps)): logged only
    const float logSa = (float)log((double)Sa);
    float kl = 0.f;
    for (int k = 0; k < A; ++k) {
        const float qa = avg[k] + kPgEps;
        const float lpa = (float)log((double)qa) - logSa;
        kl += (qa / Sa) * (lpa - r.lp[k]);
    }
    s.kl += kl;
    if (trust) {                                                     // acer_policy_head.py:103-112 on g
        float num = 0.f, den = 0.f;
        for (int k = 0; k < A; ++k) {
            const float gp = (-g[k]) * fT, kk = -(avg[k] / r.q[k]);
            num += kk * gp;
            den += kk * kk;
        }
        const float adj = fmaxf((num - delta) / (den + kPgEps), 0.f);
        for (int k = 0; k < A; ++k) {
            const float gp = (-g[k]) * fT, kk = -(avg[k] / r.q[k]);
            g[k] = (-(gp - adj * kk)) / fT;
        }
    }
    float dot = 0.f;
    for (int k = 0; k < A; ++k) dot += g[k] * r.p[k];
    for (int j = 0; j < A; ++j) dz[j] = r.p[j] * (g[j] - dot);
}

}  // namespace rlx
