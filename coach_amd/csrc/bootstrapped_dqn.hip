// Bootstrapped DQN on gfx950: the K-head masked loss + gradient and the ensemble acting reductions (selected head / vote,
// and UCB's mean + lambda * std).
//
// Replaces, in the reference (paths under rl_coach/):
//   * BootstrappedDQNAgent.learn_from_batch   agents/bootstrapped_dqn_agent.py:57-86  (per head and row: Double-DQN target
//                                             action on the online network's s' values, fp64 TD target, only where the
//                                             transition's mask has the head's bit)
//   * the K QHead losses and their sum        architectures/tensorflow_components/heads/q_head.py, head.py:172-181
//   * Bootstrapped.get_action                 exploration_policies/bootstrapped.py:72-85 (selected head in TRAIN, majority
//                                             vote otherwise) + EGreedy.get_action, e_greedy.py:84-101
//   * UCB.get_action                          exploration_policies/ucb.py:76-86 (mean + lamb * std over the heads in TRAIN,
//                                             the mean otherwise) + EGreedy.get_action
//
// Q is the head layer's output [rows][K*A]: column h*A + a is action a of head h.  The arithmetic of one (row, head) is
// that of dqn_head_loss_kernel (targets.hip) for that head alone with a selector and no importance weights — the same
// fp64 target, the same fp32 rounding points, and each head's batch sum goes through the same tree — so with every mask
// bit set head h's slice of dQ and head_losses[h] are rlx_dqn_head_loss's on columns [h*A, (h+1)*A), bit for bit.
// Compiled with -ffp-contract=off.
#include "rlx_common.hpp"

namespace {

constexpr int kBootThreads = 256;      // four waves; wave 0 holds the heads (lane h = head h)
constexpr int kBootMaxHeads = 32;
constexpr int kBootMaxActions = 18;
constexpr int kBootMaxBatch = 256;
// the [K][A] tile of a row in LDS with an odd pitch: lane h reads word h*pitch + a, and ds_read_b32 banks are word % 32
// over a 32-lane group — an odd pitch puts the 32 heads on 32 different banks
constexpr int kBootMaxPitch = kBootMaxActions | 1;
constexpr int kBootTile = kBootMaxHeads * kBootMaxPitch;

__device__ __forceinline__ int tile_pitch(int n_actions) { return n_actions | 1; }

struct BootLossArgs {
    const float *q; long long ld_q;                  // online(s)
    const float *q_next, *q_sel; long long ld_next;  // target(s'), online(s')
    const int *actions;
    const float *rewards;
    const unsigned char *dones;
    const unsigned int *masks;
    double discount;
    int n_heads, n_actions, batch, huber;
    float grad_scale;
    float *dq; long long ld_dq;
    float *partials;             // [K][batch] workspace
    unsigned int *ticket;        // one zero-initialised word, left at zero
    float *loss;
    int *status;
    float *head_losses;          // [K] or null
    float *td_targets;           // [batch][K] or null
    int *target_actions;         // [batch][K] or null
    int tree;                    // threads of rlx_dqn_head_loss's block at this batch: its tree has this many leaves
};

// One workgroup per batch row.  All threads stage the row's three [K*A] vectors with coalesced loads; lane h of wave 0
// does head h; all threads write the row of dQ; the workgroup that draws the last ticket sums every head's row terms in
// rlx_dqn_head_loss's tree and adds the K head losses in head order.
__global__ void __launch_bounds__(kBootThreads) bootstrapped_dqn_head_loss_kernel(const BootLossArgs a) {
    __shared__ float q_s[kBootTile], qn_s[kBootTile], qs_s[kBootTile];
    __shared__ float g_s[kBootMaxHeads];
    __shared__ float red[kBootMaxHeads * kBootMaxBatch];
    __shared__ bool last_s;
    const int b = blockIdx.x, t = threadIdx.x, K = a.n_heads, A = a.n_actions, B = a.batch, P = tile_pitch(A);
    const float *qr = a.q + (size_t)b * a.ld_q;
    const float *nr = a.q_next + (size_t)b * a.ld_next, *sr = a.q_sel + (size_t)b * a.ld_next;
    for (int c = t; c < K * A; c += kBootThreads) {
        const int o = (c / A) * P + c % A;
        q_s[o] = qr[c];
        qn_s[o] = nr[c];
        qs_s[o] = sr[c];
    }
    const int act = a.actions[b];
    const bool valid = act >= 0 && act < A;
    if (t == 0 && !valid) atomicOr(a.status, 1);
    __syncthreads();
    if (t < K) {
        const int h = t;
        const float *qs = qs_s + h * P;
        int best = 0;
        float bv = qs[0];
        for (int k = 1; k < A; ++k)
            rlx::np_argmax_step(qs[k], k, bv, best);             // np.argmax: first maximum, first NaN
        float term = 0.f, g = 0.f, tdt = 0.f;
        if (valid) {
            const float qa = q_s[h * P + act];
            tdt = qa;                                            // a cleared bit: the target is the prediction itself
            if ((a.masks[b] >> h) & 1u) {
                const double qn = (double)qn_s[h * P + best];
                const double y = (double)a.rewards[b] + (1.0 - (a.dones[b] ? 1.0 : 0.0)) * a.discount * qn;   // :79-81
                const float y32 = (float)y;
                const float e = qa - y32;
                const float w = 1.f;
                float l, d;
                if (!a.huber) { l = e * e; d = 2.f * e; }
                else { const float ae = fabsf(e); l = ae <= 1.f ? 0.5f * e * e : ae - 0.5f; d = fminf(fmaxf(e, -1.f), 1.f); }
                term = w * l;
                g = a.grad_scale * w * d / (float)B;
                tdt = y32;
            }
        }
        g_s[h] = g;
        if (a.td_targets) a.td_targets[(size_t)b * K + h] = tdt;
        if (a.target_actions) a.target_actions[(size_t)b * K + h] = best;
        // the row's term of head h, for the workgroup that draws the last ticket (the release below is wave 0's)
        __hip_atomic_store(&a.partials[(size_t)h * B + b], term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    float *drow = a.dq + (size_t)b * a.ld_dq;
    for (int c = t; c < K * A; c += kBootThreads) drow[c] = (valid && c % A == act) ? g_s[c / A] : 0.f;
    if (t == 0) {
        const unsigned int old = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last_s = old == (unsigned int)(B - 1);
        if (last_s) __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last_s) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // K trees side by side: red[h][i], i < n leaves (rows beyond the batch are zeros, as in rlx_dqn_head_loss's block)
    const int n = a.tree;
    for (int c = t; c < K * n; c += kBootThreads) {
        const int h = c / n, i = c % n;
        red[c] = i < B ? __hip_atomic_load(&a.partials[(size_t)h * B + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    }
    __syncthreads();
    for (int d = n >> 1; d > 0; d >>= 1) {
        for (int c = t; c < K * d; c += kBootThreads) {
            const int h = c / d, i = c % d;
            red[h * n + i] += red[h * n + i + d];
        }
        __syncthreads();
    }
    if (t == 0) {
        float total = 0.f;
        for (int h = 0; h < K; ++h) {
            const float lh = red[h * n] / (float)B;
            if (a.head_losses) a.head_losses[h] = lh;
            total += lh;                                         // the total loss: the heads' losses, added in head order
        }
        a.loss[0] = total;
    }
}

// EGreedy.get_action (e_greedy.py:84-101) on one env's action values v[0 .. A), by one lane: the random action when the
// env explores, else the argmax of the tie-break draws over the entries close to the maximum.
__device__ __forceinline__ int egreedy_choice(const float *v, int A, double explore_u, int random_act,
                                              const double *tie, double epsilon) {
    if (explore_u < epsilon) return random_act;                  // e_greedy.py:88
    float mx = v[0];
    for (int k = 1; k < A; ++k) mx = (v[k] > mx || v[k] != v[k]) ? v[k] : mx;   // egreedy_kernel's np.max
    const float tol = 1e-8f + 1e-5f * fabsf(mx);                 // egreedy_kernel's isclose (explore.hip)
    const bool mx_finite = fabsf(mx) <= 3.402823466e+38f;
    int best = 0;
    double bv = -1.0;
    for (int k = 0; k < A; ++k) {
        const bool close = (mx_finite && fabsf(v[k] - mx) <= tol) || v[k] == mx;
        const double d = close ? tie[k] : 0.0;
        if (d > bv) { bv = d; best = k; }
    }
    return best;
}

// One wave per env.  The env's [K*A] row is staged into the padded tile; TRAIN: the values are the selected head's;
// otherwise lane h votes for head h's first maximum, the counts' first maximum wins (np.bincount + np.argmax: the
// lowest action index on a tie) and the values are its one-hot vector.  Lane 0 then makes rlx_egreedy's choice on the
// values (fp32 isclose; a one-hot vector has one entry close to its maximum, so the tie draw decides nothing there).
__global__ void __launch_bounds__(64) bootstrapped_egreedy_kernel(const float *__restrict__ q, long long ld, int n_heads,
                                                                  const int *__restrict__ selected_head, int vote,
                                                                  const double *__restrict__ explore_u,
                                                                  const int *__restrict__ random_act,
                                                                  const double *__restrict__ tie_rand, double epsilon,
                                                                  int n_env, int n_actions, float *__restrict__ values_out,
                                                                  int *__restrict__ actions) {
    __shared__ float q_s[kBootTile];
    __shared__ float v_s[kBootMaxActions];
    __shared__ int votes[kBootMaxHeads];
    const int e = blockIdx.x, t = threadIdx.x, K = n_heads, A = n_actions, P = tile_pitch(A);
    const float *qe = q + (size_t)e * ld;
    for (int c = t; c < K * A; c += 64) q_s[(c / A) * P + c % A] = qe[c];
    __syncthreads();
    if (vote) {
        if (t < K) {
            const float *r = q_s + t * P;
            int best = 0;
            float bv = r[0];
            for (int k = 1; k < A; ++k)
                if (r[k] > bv) { bv = r[k]; best = k; }
            votes[t] = best;
        }
        __syncthreads();
        if (t == 0) {
            int top = 0, top_n = -1;
            for (int k = 0; k < A; ++k) {
                int n = 0;
                for (int h = 0; h < K; ++h) n += votes[h] == k ? 1 : 0;
                if (n > top_n) { top_n = n; top = k; }
            }
            for (int k = 0; k < A; ++k) v_s[k] = k == top ? 1.f : 0.f;
        }
    } else {
        int h = selected_head[e];
        h = h < 0 ? 0 : (h >= K ? K - 1 : h);                    // (stays inside the row whatever the word holds)
        if (t < A) v_s[t] = q_s[h * P + t];
    }
    __syncthreads();
    if (values_out && t < A) values_out[(size_t)e * A + t] = v_s[t];
    if (t != 0) return;
    actions[e] = egreedy_choice(v_s, A, explore_u[e], random_act[e], tie_rand + (size_t)e * A, epsilon);
}

// One wave per env, lane a = action a.  UCB.get_action (exploration_policies/ucb.py:76-86): the values are the heads' mean
// plus lamb times their (population) standard deviation while training, the mean alone otherwise; lane 0 then makes
// rlx_egreedy's choice on them.  The sums run over the heads in head order, in fp32, one rounding per operation (the
// file is compiled without FMA contraction) -- the order numpy's mean / std over axis 0 take (tests/ucb_ref.py).
__global__ void __launch_bounds__(64) ucb_egreedy_kernel(const float *__restrict__ q, long long ld, int n_heads, float lamb,
                                                         int use_std, const double *__restrict__ explore_u,
                                                         const int *__restrict__ random_act,
                                                         const double *__restrict__ tie_rand, double epsilon, int n_env,
                                                         int n_actions, float *__restrict__ values_out,
                                                         float *__restrict__ std_out, int *__restrict__ actions) {
    __shared__ float q_s[kBootTile];
    __shared__ float v_s[kBootMaxActions];
    const int e = blockIdx.x, t = threadIdx.x, K = n_heads, A = n_actions, P = tile_pitch(A);
    const float *qe = q + (size_t)e * ld;
    for (int c = t; c < K * A; c += 64) q_s[(c / A) * P + c % A] = qe[c];
    __syncthreads();
    if (t < A) {
        const float kf = (float)K;
        float s = q_s[t];
        for (int h = 1; h < K; ++h) s += q_s[h * P + t];
        const float mean = s / kf;
        float v = mean;
        if (use_std) {
            float d = q_s[t] - mean;
            float acc = d * d;
            for (int h = 1; h < K; ++h) {
                d = q_s[h * P + t] - mean;
                acc += d * d;
            }
            const float sd = sqrtf(acc / kf);
            v = mean + lamb * sd;
            if (std_out) std_out[(size_t)e * A + t] = sd;
        }
        v_s[t] = v;
        values_out[(size_t)e * A + t] = v;
    }
    __syncthreads();
    if (t != 0) return;
    actions[e] = egreedy_choice(v_s, A, explore_u[e], random_act[e], tie_rand + (size_t)e * A, epsilon);
}

}  // namespace

extern "C" {

int rlx_bootstrapped_dqn_head_loss(const float *q_online, long long ld_q, const float *q_next_target,
                                   const float *q_next_online, long long ld_next, const int *actions,
                                   const float *rewards, const unsigned char *game_overs, const uint32_t *masks,
                                   double discount, int batch, int n_heads, int n_actions, int huber, float grad_scale,
                                   float *dq, long long ld_dq, float *partials, unsigned int *ticket, float *loss_scalar,
                                   int *status, float *head_losses, float *td_targets, int *target_actions,
                                   void *stream) {
    RLX_REQUIRE(q_online && q_next_target && q_next_online && actions && rewards && game_overs && masks && dq &&
                    partials && ticket && loss_scalar && status,
                "rlx_bootstrapped_dqn_head_loss: null pointer");
    RLX_REQUIRE(n_heads >= 1 && n_heads <= kBootMaxHeads && n_actions >= 1 && n_actions <= kBootMaxActions &&
                    batch >= 1 && batch <= kBootMaxBatch,
                "rlx_bootstrapped_dqn_head_loss: unsupported sizes (heads=%d <= 32, actions=%d <= 18, batch=%d <= 256)",
                n_heads, n_actions, batch);
    const long long row = (long long)n_heads * n_actions;
    RLX_REQUIRE(ld_q >= row && ld_next >= row && ld_dq >= row, "rlx_bootstrapped_dqn_head_loss: leading dimension < K*A");
    BootLossArgs a;
    a.q = q_online; a.ld_q = ld_q; a.q_next = q_next_target; a.q_sel = q_next_online; a.ld_next = ld_next;
    a.actions = actions; a.rewards = rewards; a.dones = game_overs; a.masks = masks; a.discount = discount;
    a.n_heads = n_heads; a.n_actions = n_actions; a.batch = batch; a.huber = huber; a.grad_scale = grad_scale;
    a.dq = dq; a.ld_dq = ld_dq; a.partials = partials; a.ticket = ticket; a.loss = loss_scalar; a.status = status;
    a.head_losses = head_losses; a.td_targets = td_targets; a.target_actions = target_actions;
    a.tree = 64;
    while (a.tree < batch) a.tree <<= 1;
    RLX_LAUNCH((bootstrapped_dqn_head_loss_kernel), batch, kBootThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_bootstrapped_egreedy(const float *q_values, long long ld, int n_heads, const int *selected_head, int vote,
                             const double *explore_uniforms, const int *random_actions,
                             const double *tie_break_uniforms, double epsilon, int n_env, int n_actions,
                             float *values_out, int *actions, void *stream) {
    RLX_REQUIRE(q_values && explore_uniforms && random_actions && tie_break_uniforms && actions && (vote || selected_head),
                "rlx_bootstrapped_egreedy: null pointer");
    RLX_REQUIRE(n_env > 0 && n_heads >= 1 && n_heads <= kBootMaxHeads && n_actions >= 1 && n_actions <= kBootMaxActions &&
                    ld >= (long long)n_heads * n_actions,
                "rlx_bootstrapped_egreedy: bad shape (heads=%d <= 32, actions=%d <= 18)", n_heads, n_actions);
    RLX_LAUNCH((bootstrapped_egreedy_kernel), n_env, 64, 0, rlx::as_stream(stream), q_values, ld, n_heads, selected_head,
               vote, explore_uniforms, random_actions, tie_break_uniforms, epsilon, n_env, n_actions, values_out, actions);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_ucb_egreedy(const float *q_values, long long ld, int n_heads, float lamb, int use_std,
                    const double *explore_uniforms, const int *random_actions, const double *tie_break_uniforms,
                    double epsilon, int n_env, int n_actions, float *values_out, float *std_out, int *actions,
                    void *stream) {
    RLX_REQUIRE(q_values && explore_uniforms && random_actions && tie_break_uniforms && values_out && actions,
                "rlx_ucb_egreedy: null pointer");
    RLX_REQUIRE(n_env > 0 && n_heads >= 1 && n_heads <= kBootMaxHeads && n_actions >= 1 && n_actions <= kBootMaxActions &&
                    ld >= (long long)n_heads * n_actions,
                "rlx_ucb_egreedy: bad shape (heads=%d <= 32, actions=%d <= 18)", n_heads, n_actions);
    RLX_LAUNCH((ucb_egreedy_kernel), n_env, 64, 0, rlx::as_stream(stream), q_values, ld, n_heads, lamb, use_std,
               explore_uniforms, random_actions, tie_break_uniforms, epsilon, n_env, n_actions, values_out, std_out,
               actions);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
