// PPO-penalty head (the reference's PPOAgent, agents/ppo_agent.py, with heads/ppo_head.py:52-98 built WITHOUT
// clip_likelihood_ratio_using_epsilon and WITH use_kl_regularization): the surrogate is unclipped and the loss carries
//
//     kl_coefficient * KL + high_kl_penalty_coefficient * max(0, KL - kl_cutoff)^2        (ppo_head.py:68-72)
//
// where KL = mean_b KL(old_b || new_b) is a BATCH mean.  The gradient of the squared hinge therefore multiplies every
// row's dKL_b/dz by a factor that depends on all rows,
//
//     c = kl_coefficient + 2 * high * max(0, KL - kl_cutoff),
//
// which is why this head is a launch of its own: one workgroup, one row per thread (batch <= 1024), in three phases.
//   A  per row: log pi(a), log pi_old(a), ratio, entropy, KL(old || new); the optional likelihood_ratio output.
//   B  the batch sums through the fixed LDS tree (rlx_losses::block_sum, no atomics), KL mean, the factor c.
//   C  the gradient rows: (-adv ratio / B) dlogp/dz + (c / B) dKL_b/dz - (beta / B) dH_b/dz, times grad_scale.
// kl_coefficient is a DEVICE scalar (ppo_head.py:42-45 keeps it in a tf.Variable): a captured graph survives
// rlx_ppo_kl_coefficient_update changing it between training phases.
//
// Discrete: phase A is rlx_losses::ppo_discrete_row itself, called with a clip range that cannot bind (kNoClip) and
// (with the KL terms) grad_scale 1, so the surrogate, entropy, KL and the dlogp / dH part of the gradient have ONE definition and one
// rounding; with use_kl_regularization = 0 the results are rlx_ppo_discrete_loss's bit for bit at that clip range.
// Continuous: the formulas of ppo_continuous_loss_kernel (csrc/losses.hip) are RESTATED here, not shared: that kernel's
// products are left to the optimiser's FMA contraction and this file's are not, so a shared function would not keep that
// kernel's bits; the two agree within the counted bounds of tests/ppo_kl_ref.py, not bit for bit.
//
// Contraction is switched off per function (#pragma clang fp contract(off), as ppo_discrete_row does), NOT with
// -ffp-contract=off for the file: the flag also changes how the compiler expands logf INSIDE ppo_discrete_row (the last
// addition of its extended-precision product is fused or not), and the discrete launch would lose its bit-identity with
// rlx_ppo_discrete_loss, which csrc/losses.hip builds without the flag.
//
// TensorFlow's op-level rounding is unpinned, as for the other heads (see losses.hip).
#include "losses_body.hpp"

namespace {
using namespace rlx_losses;

constexpr float kNoClip = 3.0e38f;                 // 1 -+ kNoClip = -+3e38: no finite ratio is clipped
constexpr int kMaxActions = 18, kMaxActionDim = 32;

inline int block_for(int batch) {
    int t = 64;
    while (t < batch && t < kMaxBlock) t <<= 1;
    return t;
}

// c and the total from the batch means (ppo_head.py:68-72, :95-97); every thread evaluates the same expressions
struct KlPenalty { float c, total; };
__device__ __forceinline__ KlPenalty kl_penalty(float surrogate, float entropy_term, float kl_mean, int use_kl,
                                                const float *__restrict__ kl_coefficient, float kl_cutoff, float high) {
#pragma clang fp contract(off)
    KlPenalty r;
    r.c = 0.f;
    r.total = surrogate;
    if (use_kl) {
        const float klc = kl_coefficient[0];
        const float h = fmaxf(0.f, kl_mean - kl_cutoff);
        r.c = klc + 2.f * high * h;
        r.total = (surrogate + klc * kl_mean) + high * (h * h);
    }
    r.total = r.total - entropy_term;
    return r;
}

__device__ __forceinline__ void write_scalars(float *__restrict__ scalars, float *__restrict__ accumulate, float sur,
                                              float ent, float kl, const KlPenalty &p) {
#pragma clang fp contract(off)
    if (scalars) {
        scalars[0] = sur;
        scalars[1] = ent;
        scalars[2] = kl;
        scalars[3] = p.total;
        scalars[4] = p.c;
    }
    if (accumulate) {                              // the epoch's running sums (ppo_agent.py:296-304), in launch order
        accumulate[0] += kl;
        accumulate[1] += ent;
        accumulate[2] += p.total;
        accumulate[3] += 1.f;
    }
}

__global__ void __launch_bounds__(kMaxBlock)
ppo_kl_discrete_kernel(const float *__restrict__ logits, long long ld, const int *__restrict__ actions,
                       const float *__restrict__ advantages, const float *__restrict__ old_probs, long long ld_old,
                       int batch, int n, float beta, float grad_scale, const float *__restrict__ kl_coefficient,
                       float kl_cutoff, float high, int use_kl, float *dlogits, long long ld_grad,
                       float *__restrict__ scalars, float *__restrict__ ratio_out, int *__restrict__ status,
                       float *__restrict__ accumulate) {
#pragma clang fp contract(off)
    __shared__ float red[kMaxBlock];
    const int b = threadIdx.x;                     // batch <= blockDim: one row per thread
    // ---- A
    float l_sur = 0.f, l_ent = 0.f, l_kl = 0.f;
    bool valid = false;
    if (b < batch) {
        PpoRowTerms t;
        // without the KL terms the row function's gradient IS the result: it scales by grad_scale itself, as in
        // rlx_ppo_discrete_loss (bit-identical for every grad_scale); with them it leaves the unscaled row for phase C
        valid = ppo_discrete_row(logits + (size_t)b * ld, old_probs + (size_t)b * ld_old, actions[b], n, advantages[b],
                                 kNoClip, beta, use_kl ? 1.f : grad_scale, batch,
                                 dlogits ? dlogits + (size_t)b * ld_grad : nullptr,
                                 ratio_out ? ratio_out + b : nullptr, nullptr, t);
        if (valid) {
            l_sur = t.sur;
            l_ent = t.ent;
            l_kl = t.kl;
        } else {
            atomicOr(status, 1);
            if (ratio_out) ratio_out[b] = 0.f;
        }
    }
    // ---- B
    const float sur = block_sum(l_sur, red);
    const float ent = block_sum(l_ent, red);
    const float kl = block_sum(l_kl, red);
    const float inv = 1.f / (float)batch;
    const float s_sur = -sur * inv, s_ent = ent * inv, s_kl = kl * inv;       // ppo_discrete_scalars' expressions
    const KlPenalty pen = kl_penalty(s_sur, beta * ent * inv, s_kl, use_kl, kl_coefficient, kl_cutoff, high);
    if (b == 0) write_scalars(scalars, accumulate, s_sur, s_ent, s_kl, pen);
    // ---- C (with the KL terms): the row holds d(surrogate - beta H)/dz at grad_scale 1 (phase A); add (c / B) (p_j - old_j / sum old)
    if (dlogits && b < batch) {
        float *g = dlogits + (size_t)b * ld_grad;
        if (!valid) {
            for (int j = 0; j < n; ++j) g[j] = 0.f;
        } else if (use_kl) {
            const float *z = logits + (size_t)b * ld, *po = old_probs + (size_t)b * ld_old;
            const float cb = pen.c / (float)batch;
            float mx = z[0];
            for (int j = 1; j < n; ++j) mx = fmaxf(mx, z[j]);
            float se = 0.f, so = 0.f;
            for (int j = 0; j < n; ++j) {
                se += expf(z[j] - mx);
                so += po[j];
            }
            // p_j as rlx_softmax forms it (the probabilities predict() hands out): an old policy that IS this softmax,
            // with sum 1, gives a KL gradient of exactly 0
            for (int j = 0; j < n; ++j) g[j] = grad_scale * (g[j] + cb * (expf(z[j] - mx) / se - po[j] / so));
        }
    }
}

// Continuous head: MultivariateNormalDiag(mean, exp(log_std) + eps) against (old_mean, old_std + eps), eps =
// finfo(float32).eps (ppo_head.py:118-144).  The entropy is the same for every row.
__global__ void __launch_bounds__(kMaxBlock)
ppo_kl_continuous_kernel(const float *__restrict__ mean, long long ld, const float *__restrict__ log_std,
                         const float *__restrict__ actions, const float *__restrict__ advantages,
                         const float *__restrict__ old_mean, const float *__restrict__ old_std, long long ld_old,
                         int batch, int A, float beta, float grad_scale, const float *__restrict__ kl_coefficient,
                         float kl_cutoff, float high, int use_kl, float *__restrict__ dmean, long long ld_grad,
                         float *__restrict__ dlog_std, float *__restrict__ scalars, float *__restrict__ ratio_out,
                         float *__restrict__ accumulate) {
#pragma clang fp contract(off)
    __shared__ float red[kMaxBlock];
    constexpr float kEps = 1.1920928955078125e-07f, kHalfLog2Pi = 0.91893853320467274178f;
    const int b = threadIdx.x;
    const float *mu = mean + (size_t)b * ld, *x = actions + (size_t)b * A;
    const float *mo = old_mean + (size_t)b * ld_old, *so = old_std + (size_t)b * ld_old;
    // ---- A
    float ent = 0.f;
    for (int a = 0; a < A; ++a) ent += 0.5f + kHalfLog2Pi + logf(expf(log_std[a]) + kEps);
    float l_sur = 0.f, l_kl = 0.f, g_logp = 0.f;
    if (b < batch) {
        float logp = 0.f, logp_old = 0.f, kl = 0.f;
        for (int a = 0; a < A; ++a) {
            const float sd = expf(log_std[a]) + kEps, sdo = so[a] + kEps;
            const float z = (x[a] - mu[a]) / sd, zo = (x[a] - mo[a]) / sdo;
            logp += -0.5f * z * z - logf(sd) - kHalfLog2Pi;
            logp_old += -0.5f * zo * zo - logf(sdo) - kHalfLog2Pi;
            const float dm = mo[a] - mu[a];
            kl += logf(sd / sdo) + (sdo * sdo + dm * dm) / (2.f * sd * sd) - 0.5f;
        }
        const float ratio = expf(logp - logp_old);                 // (:78)
        const float adv = advantages[b];
        l_sur = ratio * adv;                                        // (:88)
        l_kl = kl;
        g_logp = -adv * ratio / (float)batch;
        if (ratio_out) ratio_out[b] = ratio;
    }
    // ---- B
    const float sur = block_sum(l_sur, red);
    const float kls = block_sum(l_kl, red);
    const float inv = 1.f / (float)batch;
    const float s_sur = -sur * inv, s_kl = kls * inv;
    const KlPenalty pen = kl_penalty(s_sur, beta * ent, s_kl, use_kl, kl_coefficient, kl_cutoff, high);
    if (b == 0) write_scalars(scalars, accumulate, s_sur, ent, s_kl, pen);
    // ---- C
    const float cb = pen.c / (float)batch;
    if (dmean && b < batch) {
        for (int a = 0; a < A; ++a) {
            const float sd = expf(log_std[a]) + kEps;
            float g = g_logp * (x[a] - mu[a]) / (sd * sd);          // d logp / d mu = (x - mu) / sd^2
            if (use_kl) g = g + cb * (-(mo[a] - mu[a]) / (sd * sd));
            dmean[(size_t)b * ld_grad + a] = grad_scale * g;
        }
    }
    if (dlog_std) {
        // one fixed-order workgroup sum per action dimension (reproducible, no atomics), as ppo_continuous_loss_kernel
        for (int a = 0; a < A; ++a) {
            const float e = expf(log_std[a]);
            const float sd = e + kEps;
            float part = 0.f;
            if (b < batch) {
                const float d = x[a] - mu[a];
                part = g_logp * (d * d / (sd * sd * sd) - 1.f / sd) * e;
                if (use_kl) {
                    const float sdo = so[a] + kEps, dm = mo[a] - mu[a];
                    part = part + cb * ((1.f - (sdo * sdo + dm * dm) / (sd * sd)) * e / sd);
                }
            }
            const float tot = block_sum(part, red);
            if (b == 0) dlog_std[a] = grad_scale * (tot - beta * e / sd);
        }
    }
}

// update_kl_coefficient (ppo_agent.py:329-353) on the fp32 variable.  The reference compares the fp32 mean of the last
// epoch's KL fetches with the python floats 1.3 * kl_target and 0.7 * kl_target and multiplies / divides the fp32
// coefficient by the python float 1.5: under NEP 50 the python floats are weak, so the comparisons are fp32 against the
// products ROUNDED to fp32, and the new coefficient is the fp32 product / quotient.  The thresholds arrive rounded.
__global__ void ppo_kl_coefficient_kernel(const float *__restrict__ epoch_sums, float hi, float lo,
                                          float *__restrict__ kl_coefficient, float *__restrict__ kl_mean_out) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!(epoch_sums[3] > 0.f)) {                                  // no minibatch was accumulated: nothing to adapt to
        if (kl_mean_out) kl_mean_out[0] = 0.f;
        return;
    }
    const float kl = epoch_sums[0] / epoch_sums[3];                // np.mean(loss['fetch_result'], 0)[0]  (:304)
    float c = kl_coefficient[0];
    if (kl > hi)
        c = c * 1.5f;                                              // (:339-341)
    else if (kl < lo)
        c = c / 1.5f;                                              // (:342-344)
    kl_coefficient[0] = c;
    if (kl_mean_out) kl_mean_out[0] = kl;
}

}  // namespace

extern "C" {

int rlx_ppo_kl_discrete_loss(const float *logits, long long ld, const int *actions, const float *advantages,
                             const float *old_probs, long long ld_old, int batch, int n_actions, float beta_entropy,
                             float grad_scale, const float *kl_coefficient, float kl_cutoff,
                             float high_kl_penalty_coefficient, int use_kl_regularization, float *dlogits,
                             long long ld_grad, float *scalars, float *likelihood_ratio, int *status, float *accumulate,
                             void *stream) {
    RLX_REQUIRE(logits && actions && advantages && old_probs && status, "rlx_ppo_kl_discrete_loss: null pointer");
    RLX_REQUIRE(!use_kl_regularization || kl_coefficient, "rlx_ppo_kl_discrete_loss: kl_coefficient is null");
    RLX_REQUIRE(batch > 0 && batch <= kMaxBlock && n_actions >= 1 && n_actions <= kMaxActions && ld >= n_actions &&
                    ld_old >= n_actions,
                "rlx_ppo_kl_discrete_loss: bad shape (minibatch must be <= %d rows, 1 <= actions <= %d)", kMaxBlock,
                kMaxActions);
    RLX_REQUIRE(!dlogits || ld_grad >= n_actions, "rlx_ppo_kl_discrete_loss: bad gradient pitch");
    RLX_LAUNCH((ppo_kl_discrete_kernel), 1, block_for(batch), 0, rlx::as_stream(stream), logits, ld, actions,
               advantages, old_probs, ld_old, batch, n_actions, beta_entropy, grad_scale, kl_coefficient, kl_cutoff,
               high_kl_penalty_coefficient, use_kl_regularization, dlogits, ld_grad, scalars, likelihood_ratio, status,
               accumulate);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_ppo_kl_continuous_loss(const float *mean, long long ld, const float *log_std, const float *actions,
                               const float *advantages, const float *old_mean, const float *old_std, long long ld_old,
                               int batch, int action_dim, float beta_entropy, float grad_scale,
                               const float *kl_coefficient, float kl_cutoff, float high_kl_penalty_coefficient,
                               int use_kl_regularization, float *dmean, long long ld_grad, float *dlog_std,
                               float *scalars, float *likelihood_ratio, float *accumulate, void *stream) {
    RLX_REQUIRE(mean && log_std && actions && advantages && old_mean && old_std,
                "rlx_ppo_kl_continuous_loss: null pointer");
    RLX_REQUIRE(!use_kl_regularization || kl_coefficient, "rlx_ppo_kl_continuous_loss: kl_coefficient is null");
    RLX_REQUIRE(batch > 0 && batch <= kMaxBlock && action_dim >= 1 && action_dim <= kMaxActionDim &&
                    ld >= action_dim && ld_old >= action_dim,
                "rlx_ppo_kl_continuous_loss: bad shape (minibatch must be <= %d rows, 1 <= action_dim <= %d)",
                kMaxBlock, kMaxActionDim);
    RLX_REQUIRE(!dmean || ld_grad >= action_dim, "rlx_ppo_kl_continuous_loss: bad gradient pitch");
    RLX_LAUNCH((ppo_kl_continuous_kernel), 1, block_for(batch), 0, rlx::as_stream(stream), mean, ld, log_std, actions,
               advantages, old_mean, old_std, ld_old, batch, action_dim, beta_entropy, grad_scale, kl_coefficient,
               kl_cutoff, high_kl_penalty_coefficient, use_kl_regularization, dmean, ld_grad, dlog_std, scalars,
               likelihood_ratio, accumulate);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_ppo_kl_coefficient_update(const float *epoch_sums, double target_kl, float *kl_coefficient, float *kl_mean_out,
                                  void *stream) {
    RLX_REQUIRE(epoch_sums && kl_coefficient, "rlx_ppo_kl_coefficient_update: null pointer");
    RLX_REQUIRE(target_kl > 0.0, "rlx_ppo_kl_coefficient_update: target_kl must be positive");
    // 1.3 * kl_target and 0.7 * kl_target are products of python floats (fp64), which the comparison rounds to fp32;
    // target_kl is a double because float(1.3 * 0.01) is not float(1.3 * float(0.01))
    const float hi = (float)(1.3 * target_kl), lo = (float)(0.7 * target_kl);
    RLX_LAUNCH((ppo_kl_coefficient_kernel), 1, 64, 0, rlx::as_stream(stream), epoch_sums, hi, lo, kl_coefficient,
               kl_mean_out);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
