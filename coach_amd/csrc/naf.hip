// Normalized Advantage Functions on gfx950: the quadratic-advantage head, its loss and its gradient.
//
// Replaces, in the reference (paths under rl_coach/):
//   * NAFHead._build_module                  architectures/tensorflow_components/heads/naf_head.py:45-86 (mu = mu_unscaled *
//                                            output_scale, the packed l_vector -> lower-triangular L with an exponentiated
//                                            diagonal, P = L L^T, A = -1/2 (u - mu)^T P (u - mu), Q = V + A)
//   * NAFAgent.learn_from_batch              agents/naf_agent.py:83-90 (fp64 TD targets on the target network's V(s'))
//   * the head's loss and tf.gradients of it heads/head.py:143-186 (mean squared error, or Huber with delta 1)
//
// The arithmetic, operation for operation, is tests/naf_ref.py's (its module text states the order): y = L^T d is
// formed instead of P, every sum runs in ascending index order, fp32 throughout except the fp64 TD target, which is
// rounded where rlx_dqn_head_loss rounds it.  Compiled with -ffp-contract=off.
//
// Mapping: one wave per batch row, four rows per 256-thread workgroup; lane c owns column c of L (contiguous in
// l_vector), d_c, mu_c and y_c.  The row's l_vector (at most 528 floats), d, y and the diagonal live in LDS.
#include "rlx_common.hpp"

namespace {

constexpr int kNafThreads = 256;
constexpr int kNafWave = 64;
constexpr int kNafRows = kNafThreads / kNafWave;   // rows of a workgroup: one per wave
constexpr int kNafMaxA = 32;
constexpr int kNafMaxL = kNafMaxA * (kNafMaxA + 1) / 2;
constexpr int kNafMaxBatch = 256;

struct NafRowIn {
    const float *v; long long ld_v;
    const float *mu_unscaled; long long ld_mu;
    const float *l_vector; long long ld_l;
    const float *output_scale;
    const float *actions; long long ld_act;      // null: u = mu
    int batch, A;
};

struct NafRowLds {
    float l[kNafMaxL];
    float d[kNafMaxA], y[kNafMaxA], diag[kNafMaxA];
};

// First index of column c in the packed vector: sum_{k<c} (A - k).
__device__ __forceinline__ int col_start(int c, int A) { return c * A - (c * (c - 1)) / 2; }

// The row's forward pass up to y = L^T d, by the row's wave; every thread of the workgroup calls it (barriers inside).
// Returns mu_c in lane c < A of a live row.
__device__ __forceinline__ float naf_row_forward(const NafRowIn &in, NafRowLds &s, int b, int ln, bool live) {
    const int A = in.A, NL = A * (A + 1) / 2;
    float mu = 0.f;
    if (live) {
        const float *lrow = in.l_vector + (size_t)b * in.ld_l;
        for (int i = ln; i < NL; i += kNafWave) s.l[i] = lrow[i];
        if (ln < A) {
            mu = in.mu_unscaled[(size_t)b * in.ld_mu + ln] * in.output_scale[ln];
            s.d[ln] = in.actions ? in.actions[(size_t)b * in.ld_act + ln] - mu : 0.f;
        }
    }
    __syncthreads();
    if (live && ln < A) {
        const int ic = col_start(ln, A);
        const float dg = expf(s.l[ic]);
        s.diag[ln] = dg;
        float acc = dg * s.d[ln];
        for (int r = ln + 1; r < A; ++r) acc += s.l[ic + r - ln] * s.d[r];
        s.y[ln] = acc;
    }
    __syncthreads();
    return mu;
}

// Adv = -0.5 * sum_c y_c^2, in column order (one lane).
__device__ __forceinline__ float naf_advantage(const NafRowLds &s, int A) {
    float ss = s.y[0] * s.y[0];
    for (int c = 1; c < A; ++c) ss += s.y[c] * s.y[c];
    return -0.5f * ss;
}

struct NafLossArgs {
    NafRowIn in;
    const float *v_next; long long ld_vnext;
    const float *rewards;
    const unsigned char *dones;
    double discount;
    int huber;
    float grad_scale;
    float *dv; long long ld_dv;
    float *dmu; long long ld_dmu;
    float *dl; long long ld_dl;
    float *partials;             // [batch] workspace
    unsigned int *ticket;        // one zero-initialised word, left at zero
    float *loss;
    float *td_targets, *q_out, *adv_out;   // [batch] or null
};

__global__ void __launch_bounds__(kNafThreads) naf_head_loss_kernel(const NafLossArgs a) {
    __shared__ NafRowLds rows[kNafRows];
    __shared__ float g_s[kNafRows], term_s[kNafRows];
    __shared__ float red[kNafMaxBatch];
    __shared__ bool last_s;
    const int t = threadIdx.x, w = t / kNafWave, ln = t % kNafWave;
    const int A = a.in.A, B = a.in.batch, b = blockIdx.x * kNafRows + w;
    const bool live = b < B;
    NafRowLds &s = rows[w];
    const float mu_scale = (live && ln < A) ? a.in.output_scale[ln] : 0.f;
    naf_row_forward(a.in, s, b, ln, live);
    if (live && ln == 0) {
        const float adv = naf_advantage(s, A);
        const float q = a.in.v[(size_t)b * a.in.ld_v] + adv;
        const double vn = (double)a.v_next[(size_t)b * a.ld_vnext];
        const double y = (double)a.rewards[b] + (1.0 - (a.dones[b] ? 1.0 : 0.0)) * a.discount * vn;   // naf_agent.py:89-90
        const float y32 = (float)y;
        const float e = q - y32;
        float l, d;
        if (!a.huber) { l = e * e; d = 2.f * e; }
        else { const float ae = fabsf(e); l = ae <= 1.f ? 0.5f * e * e : ae - 0.5f; d = fminf(fmaxf(e, -1.f), 1.f); }
        const float g = a.grad_scale * d / (float)B;
        g_s[w] = g;
        term_s[w] = l;
        a.dv[(size_t)b * a.ld_dv] = g;
        if (a.td_targets) a.td_targets[b] = y32;
        if (a.q_out) a.q_out[b] = q;
        if (a.adv_out) a.adv_out[b] = adv;
    }
    __syncthreads();
    if (live && ln < A) {
        const float g = g_s[w];
        // (L y)_c = sum_{k <= c} L[c][k] y_k: row c of L crosses the packed columns
        float acc = 0.f;
        int ik = 0;
        for (int k = 0; k <= ln; ++k) {
            const float lck = k == ln ? s.diag[ln] : s.l[ik + ln - k];
            const float p = lck * s.y[k];
            acc = k == 0 ? p : acc + p;
            ik += A - k;
        }
        a.dmu[(size_t)b * a.ld_dmu + ln] = (g * acc) * mu_scale;
        const int ic = col_start(ln, A);
        const float tc = (-g) * s.y[ln];
        float *dlr = a.dl + (size_t)b * a.ld_dl + ic;
        dlr[0] = (tc * s.d[ln]) * s.diag[ln];
        for (int r = ln + 1; r < A; ++r) dlr[r - ln] = tc * s.d[r];
    }
    // The batch sum: wave 0 publishes its workgroup's row terms and draws a ticket; the workgroup that draws the last
    // one sums partials[0 .. batch) in a fixed tree (rlx::ticketed_batch_sum's protocol with several rows per
    // workgroup: every access to partials and ticket is an agent-scope atomic, the release is wave 0's).
    if (t < kNafRows && blockIdx.x * kNafRows + t < B)
        __hip_atomic_store(&a.partials[blockIdx.x * kNafRows + t], term_s[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 0) {
        const unsigned int old = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last_s = old == gridDim.x - 1;
        if (last_s) __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last_s) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    red[t] = t < B ? __hip_atomic_load(&a.partials[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    __syncthreads();
    for (int d = kNafMaxBatch >> 1; d > 0; d >>= 1) {
        if (t < d) red[t] += red[t + d];
        __syncthreads();
    }
    if (t == 0) a.loss[0] = red[0] / (float)B;
}

__global__ void __launch_bounds__(kNafThreads) naf_head_forward_kernel(const NafRowIn in, float *__restrict__ mu_out,
                                                                       float *__restrict__ q_out,
                                                                       float *__restrict__ adv_out,
                                                                       float *__restrict__ l_out) {
    __shared__ NafRowLds rows[kNafRows];
    const int t = threadIdx.x, w = t / kNafWave, ln = t % kNafWave;
    const int A = in.A, b = blockIdx.x * kNafRows + w;
    const bool live = b < in.batch;
    NafRowLds &s = rows[w];
    const float mu = naf_row_forward(in, s, b, ln, live);
    if (!live) return;
    if (ln < A && mu_out) mu_out[(size_t)b * A + ln] = mu;
    if (ln == 0) {
        const float adv = naf_advantage(s, A);
        if (adv_out) adv_out[b] = adv;
        if (q_out) q_out[b] = in.v[(size_t)b * in.ld_v] + adv;
    }
    if (l_out) {
        float *lo = l_out + (size_t)b * A * A;
        for (int i = ln; i < A * A; i += kNafWave) {
            const int r = i / A, c = i % A;
            lo[i] = r < c ? 0.f : (r == c ? s.diag[c] : s.l[col_start(c, A) + r - c]);
        }
    }
}

int check_row_inputs(const char *fn, const NafRowIn &in) {
    RLX_REQUIRE(in.v && in.mu_unscaled && in.l_vector && in.output_scale, "%s: null pointer", fn);
    RLX_REQUIRE(in.A >= 1 && in.A <= kNafMaxA, "%s: unsupported action dimension %d (1 <= A <= %d)", fn, in.A, kNafMaxA);
    const long long nl = (long long)in.A * (in.A + 1) / 2;
    RLX_REQUIRE(in.ld_v >= 1 && in.ld_mu >= in.A && in.ld_l >= nl && (!in.actions || in.ld_act >= in.A),
                "%s: leading dimension smaller than the row", fn);
    return RLX_OK;
}

}  // namespace

extern "C" {

int rlx_naf_head_loss(const float *v, long long ld_v, const float *mu_unscaled, long long ld_mu, const float *l_vector,
                      long long ld_l, const float *output_scale, const float *actions, long long ld_act,
                      const float *v_next, long long ld_vnext, const float *rewards, const unsigned char *game_overs,
                      double discount, int batch, int action_dim, int huber, float grad_scale, float *dv,
                      long long ld_dv, float *dmu_unscaled, long long ld_dmu, float *dl_vector, long long ld_dl,
                      float *partials, unsigned int *ticket, float *loss_scalar, float *td_targets_out, float *q_out,
                      float *adv_out, void *stream) {
    NafLossArgs a;
    a.in = NafRowIn{v, ld_v, mu_unscaled, ld_mu, l_vector, ld_l, output_scale, actions, ld_act, batch, action_dim};
    RLX_REQUIRE(actions && v_next && rewards && game_overs && dv && dmu_unscaled && dl_vector && partials && ticket &&
                    loss_scalar,
                "rlx_naf_head_loss: null pointer");
    RLX_REQUIRE(batch >= 1 && batch <= kNafMaxBatch, "rlx_naf_head_loss: unsupported batch %d (1 <= batch <= %d)", batch,
                kNafMaxBatch);
    if (int rc = check_row_inputs("rlx_naf_head_loss", a.in)) return rc;
    const long long nl = (long long)action_dim * (action_dim + 1) / 2;
    RLX_REQUIRE(ld_vnext >= 1 && ld_dv >= 1 && ld_dmu >= action_dim && ld_dl >= nl,
                "rlx_naf_head_loss: leading dimension smaller than the row");
    a.v_next = v_next; a.ld_vnext = ld_vnext; a.rewards = rewards; a.dones = game_overs; a.discount = discount;
    a.huber = huber; a.grad_scale = grad_scale;
    a.dv = dv; a.ld_dv = ld_dv; a.dmu = dmu_unscaled; a.ld_dmu = ld_dmu; a.dl = dl_vector; a.ld_dl = ld_dl;
    a.partials = partials; a.ticket = ticket; a.loss = loss_scalar;
    a.td_targets = td_targets_out; a.q_out = q_out; a.adv_out = adv_out;
    const int grid = (batch + kNafRows - 1) / kNafRows;
    RLX_LAUNCH((naf_head_loss_kernel), grid, kNafThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_naf_head_forward(const float *v, long long ld_v, const float *mu_unscaled, long long ld_mu,
                         const float *l_vector, long long ld_l, const float *output_scale, const float *actions,
                         long long ld_act, int batch, int action_dim, float *mu_out, float *q_out, float *adv_out,
                         float *l_out, void *stream) {
    const NafRowIn in{v, ld_v, mu_unscaled, ld_mu, l_vector, ld_l, output_scale, actions, ld_act, batch, action_dim};
    RLX_REQUIRE(batch >= 1 && batch <= 65536, "rlx_naf_head_forward: unsupported batch %d", batch);
    RLX_REQUIRE(mu_out || q_out || adv_out || l_out, "rlx_naf_head_forward: no output");
    if (int rc = check_row_inputs("rlx_naf_head_forward", in)) return rc;
    const int grid = (batch + kNafRows - 1) / kNafRows;
    RLX_LAUNCH((naf_head_forward_kernel), grid, kNafThreads, 0, rlx::as_stream(stream), in, mu_out, q_out, adv_out, l_out);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
