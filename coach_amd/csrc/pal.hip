// Persistent Advantage Learning (PAL) and Mixed Monte Carlo (MMC) on gfx950: the mixed TD targets, the Q head's loss
// on them and its gradient in one launch.
//
// Replaces, in the reference (paths under rl_coach/):
//   * PALAgent.learn_from_batch              agents/pal_agent.py:70-111 (Double-DQN target, the advantage-learning
//                                            correction in its plain or persistent form, the Monte Carlo mix)
//   * MixedMonteCarloAgent.learn_from_batch  agents/mmc_agent.py:57-83 (Double-DQN target mixed with the Monte Carlo return)
//   * the QHead's loss and tf.gradients of it heads/q_head.py, heads/head.py:172-181 (mean squared error, or Huber)
//
// TD_targets equals Q_online(s) except at the taken action, so — as in dqn_head_loss_kernel (targets.hip), whose few
// lines of row arithmetic are restated here — loss and gradient live at [b, a_b] only.  The arithmetic, rounding for
// rounding, is tests/pal_ref.py's (its module text states where the reference rounds to fp32): the one-step target in
// fp64, PAL's correction in fp32 on the stored fp32 target, PAL's mix as an fp32 product plus an fp64 product, MMC's
// whole expression in fp64.  Compiled with -ffp-contract=off.
//
// One workgroup (batch <= 1024), one row per thread, the batch mean by the fixed-order LDS tree of dqn_head_loss_kernel
// over blockDim leaves.  Latency-bound, a few hundred bytes: the point is that no Q value leaves the device between
// the network passes.
#include "rlx_common.hpp"

namespace {

struct MixedTargetArgs {
    const float *q; long long ld_q;
    const float *q_cur;                  // target network on s, leading dimension ld_q; null: MMC
    const float *q_next, *q_sel; long long ld_next;
    const int *actions;
    const float *rewards;
    const unsigned char *dones;
    const double *total_returns;
    double discount, rate;
    float alpha32, keep32;               // (float)alpha, (float)(1.0 - rate): converted on the host, as the reference does
    int persistent, batch, n_actions, huber;
    float grad_scale;
    float *dq; long long ld_dq;
    float *td_targets; long long ld_t;
    float *loss;
    int *status;
};

__global__ void __launch_bounds__(1024) mixed_target_head_loss_kernel(const MixedTargetArgs a) {
    __shared__ float red[1024];
    const int i = threadIdx.x, A = a.n_actions;
    float term = 0.f;
    if (i < a.batch) {
        const float *qs = a.q_sel + (size_t)i * a.ld_next;
        const float *qn = a.q_next + (size_t)i * a.ld_next;
        int best = 0;
        float bv = qs[0], vn = qn[0];
        for (int k = 1; k < A; ++k) {
            rlx::np_argmax_step(qs[k], k, bv, best);              // np.argmax: first maximum, first NaN
            vn = fmaxf(vn, qn[k]);                                // np.max of the target's values on s'
        }
        const int act = a.actions[i];
        if (act < 0 || act >= A) {
            atomicOr(a.status, 1);
        } else {
            const float qsel = qn[best];
            const double y = (double)a.rewards[i] + (1.0 - (a.dones[i] ? 1.0 : 0.0)) * a.discount * (double)qsel;
            const double mc = a.total_returns[i];
            float t;
            if (a.q_cur) {                                                            // pal_agent.py:92-106
                const float *qc = a.q_cur + (size_t)i * a.ld_q;
                float vc = qc[0];
                for (int k = 1; k < A; ++k) vc = fmaxf(vc, qc[k]);
                float adv = vc - qc[act];
                if (a.persistent) adv = fminf(adv, vn - qsel);
                t = (float)y;
                t = t - a.alpha32 * adv;
                t = (float)((double)(a.keep32 * t) + a.rate * mc);
            } else {                                                                  // mmc_agent.py:73-78
                t = (float)((1.0 - a.rate) * y + a.rate * mc);
            }
            const float qa = a.q[(size_t)i * a.ld_q + act];
            const float e = qa - t;
            float l, g;
            if (!a.huber) { l = e * e; g = 2.f * e; }
            else { const float ae = fabsf(e); l = ae <= 1.f ? 0.5f * e * e : ae - 0.5f; g = fminf(fmaxf(e, -1.f), 1.f); }
            term = l;
            for (int k = 0; k < A; ++k) {
                a.dq[(size_t)i * a.ld_dq + k] = k == act ? a.grad_scale * g / (float)a.batch : 0.f;
                if (a.td_targets) a.td_targets[(size_t)i * a.ld_t + k] = k == act ? t : a.q[(size_t)i * a.ld_q + k];
            }
        }
    }
    red[i] = term;
    __syncthreads();
    for (int d = blockDim.x >> 1; d > 0; d >>= 1) {
        if (i < d) red[i] += red[i + d];
        __syncthreads();
    }
    if (i == 0 && a.loss) a.loss[0] = red[0] / (float)a.batch;
}

}  // namespace

extern "C" {

int rlx_mixed_target_head_loss(const float *q_online, long long ld_q, const float *q_target_cur,
                               const float *q_next_target, const float *q_next_selector, long long ld_next,
                               const int *actions, const float *rewards, const unsigned char *game_overs,
                               const double *total_returns, double discount, double pal_alpha, int persistent,
                               double mixing_rate, int batch, int n_actions, int huber, float grad_scale, float *dq,
                               long long ld_dq, float *td_targets, long long ld_targets, float *loss_scalar, int *status,
                               void *stream) {
    RLX_REQUIRE(q_online && q_next_target && q_next_selector && actions && rewards && game_overs && total_returns && dq &&
                    status,
                "rlx_mixed_target_head_loss: null pointer");
    RLX_REQUIRE(batch > 0 && batch <= 1024 && n_actions > 0,
                "rlx_mixed_target_head_loss: bad sizes (batch=%d <= 1024, actions=%d)", batch, n_actions);
    RLX_REQUIRE(ld_q >= n_actions && ld_next >= n_actions && ld_dq >= n_actions && (!td_targets || ld_targets >= n_actions),
                "rlx_mixed_target_head_loss: leading dimension < actions (%d)", n_actions);
    MixedTargetArgs a;
    a.q = q_online; a.ld_q = ld_q; a.q_cur = q_target_cur;
    a.q_next = q_next_target; a.q_sel = q_next_selector; a.ld_next = ld_next;
    a.actions = actions; a.rewards = rewards; a.dones = game_overs; a.total_returns = total_returns;
    a.discount = discount; a.rate = mixing_rate;
    a.alpha32 = (float)pal_alpha; a.keep32 = (float)(1.0 - mixing_rate);
    a.persistent = persistent; a.batch = batch; a.n_actions = n_actions; a.huber = huber; a.grad_scale = grad_scale;
    a.dq = dq; a.ld_dq = ld_dq; a.td_targets = td_targets; a.ld_t = ld_targets;
    a.loss = loss_scalar; a.status = status;
    int threads = 64;
    while (threads < batch) threads <<= 1;
    RLX_LAUNCH((mixed_target_head_loss_kernel), 1, threads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
