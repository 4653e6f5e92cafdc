// Imitation learning on gfx950: the softmax classifier's head loss, and the action mask DDQN-BCQ takes from such a
// classifier (its "imitation model").
//
// Replaces, in the reference (paths under rl_coach/):
//   * ClassificationHead between the forward and the backward pass   architectures/tensorflow_components/heads/classification_head.py
//     (tf.nn.softmax as the output, softmax_cross_entropy_with_logits as the loss, summed by general_network.py:360)
//   * DDQNBCQAgent.select_actions, NNImitationModelParameters branch, up to its argmax   agents/ddqn_bcq_agent.py:115-133
//
// Both are latency-bound row kernels over at most 1024 rows of at most 18 actions: ONE workgroup, one row per thread
// (as rlx_dqn_head_loss and rlx_bcq_masked_selector), so every sum has a fixed order and nothing is handed between
// workgroups.  The softmax is policy_head.hpp's softmax_row — the project's one definition — and the selector's row
// tail is bcq_selector_tail.hpp's.  tests/imitation_ref.py is the numpy restatement; it states every fp32 rounding
// point named here.  Compiled with -ffp-contract=off.
#include "bcq_selector_tail.hpp"
#include "policy_head.hpp"

namespace {

constexpr int kMaxRows = 1024;
constexpr int kMaxActions = rlx::kPgMaxActions;
static_assert(kMaxActions == rlx::kBcqSelectorMaxActions && kMaxRows == rlx::kBcqSelectorMaxBatch, "one set of limits");

// np.argmax: the first maximum
__device__ __forceinline__ int first_argmax(const float *v, int A) {
    int best = 0;
    float bv = v[0];
    for (int k = 1; k < A; ++k)
        if (v[k] > bv) { bv = v[k]; best = k; }
    return best;
}

struct ClsArgs {
    const float *logits; long long ld;
    const int *actions;                     // [rows], or null
    const float *labels; long long ld_l;    // [rows][ld_l], or null
    float grad_scale;
    int rows, A;
    float *dlogits; long long ld_d;
    float *probs; long long ld_p;           // optional
    float *row_loss;                        // optional [rows]
    float *scalars;                         // [2]: sum of the rows' losses, number of correct rows
    int *status;
};

// Thread b owns row b.  Per row, fp32: p = softmax_row(z); log p_j = (z_j - mx) - (float)log((double)s);
// actions mode: loss = -log p_a, dz_j = (p_j - [j == a]) * grad_scale; labels mode: loss = -(sum_j l_j * log p_j) in
// index order from 0.f, dz_j = (p_j - l_j) * grad_scale.  The batch sum: the rows' losses (0.f beyond the batch and
// for a row without a term) through the tree of the launch's blockDim threads.
__global__ void __launch_bounds__(kMaxRows) classification_head_loss_kernel(const ClsArgs a) {
    __shared__ float loss_s[kMaxRows];
    __shared__ int hit_s[kMaxRows];
    const int b = threadIdx.x, A = a.A;
    float loss = 0.f;
    int hit = 0;
    if (b < a.rows) {
        const float *x = a.logits + (size_t)b * a.ld;
        float *d = a.dlogits + (size_t)b * a.ld_d;
        float p[kMaxActions], mx, s;
        rlx::softmax_row(x, A, p, mx, s);
        const float logs = (float)log((double)s);
        if (a.probs) {
            float *po = a.probs + (size_t)b * a.ld_p;
            for (int j = 0; j < A; ++j) po[j] = p[j];
        }
        if (a.actions) {
            const int act = a.actions[b];
            if (act >= 0 && act < A) {
                loss = -((x[act] - mx) - logs);
                for (int j = 0; j < A; ++j) d[j] = (p[j] - (j == act ? 1.f : 0.f)) * a.grad_scale;
                hit = first_argmax(p, A) == act;
            } else {                        // no term, zero gradient, not counted
                atomicOr(a.status, 1);
                for (int j = 0; j < A; ++j) d[j] = 0.f;
            }
        } else {
            const float *l = a.labels + (size_t)b * a.ld_l;
            float acc = 0.f;
            for (int j = 0; j < A; ++j) {
                acc += l[j] * ((x[j] - mx) - logs);
                d[j] = (p[j] - l[j]) * a.grad_scale;
            }
            loss = -acc;
            hit = first_argmax(p, A) == first_argmax(l, A);
        }
        if (a.row_loss) a.row_loss[b] = loss;
    }
    loss_s[b] = loss;
    hit_s[b] = hit;
    __syncthreads();
    for (int t = blockDim.x >> 1; t > 0; t >>= 1) {
        if (b < t) {
            loss_s[b] += loss_s[b + t];
            hit_s[b] += hit_s[b + t];
        }
        __syncthreads();
    }
    if (b == 0) {
        a.scalars[0] = loss_s[0];
        a.scalars[1] = (float)hit_s[0];
    }
}

struct ImSelArgs {
    const float *q; long long ld_q;
    const float *im; long long ld_i;        // the imitation model's output on s': logits, or probabilities
    float threshold;
    int probs_in;
    int batch, n_actions;
    uint32_t seed, rank;
    const long long *event;
    float *sel; long long ld_sel;
    float *fam; long long ld_f;             // optional
    int *zero_rows;
};

__global__ void __launch_bounds__(kMaxRows) bcq_imitation_selector_kernel(const ImSelArgs a) {
    __shared__ int red[rlx::kBcqSelectorMaxBatch];
    const int b = threadIdx.x, A = a.n_actions;
    int zero = 0;
    if (b < a.batch) {
        const float *q = a.q + (size_t)b * a.ld_q, *x = a.im + (size_t)b * a.ld_i;
        float *s = a.sel + (size_t)b * a.ld_sel;
        float f[kMaxActions];
        if (a.probs_in) {
            for (int k = 0; k < A; ++k) f[k] = x[k];
        } else {
            float mx, sum;
            rlx::softmax_row(x, A, f, mx, sum);
        }
        if (a.fam) {
            float *fo = a.fam + (size_t)b * a.ld_f;
            for (int k = 0; k < A; ++k) fo[k] = f[k];
        }
        // ddqn_bcq_agent.py:117-118, :129: an fp32 comparison (a NaN familiarity is not masked); the row's maximum is
        // -inf when every action is masked (or its own Q value is -inf already)
        zero = 1;
        for (int k = 0; k < A; ++k) {
            const float v = f[k] < a.threshold ? -INFINITY : q[k];
            if (!(v == -INFINITY)) zero = 0;
            s[k] = v;
        }
        if (zero) rlx::bcq_zero_row_draws(s, b, A, a.seed, a.rank, a.event);
    }
    rlx::bcq_zero_row_count(zero, a.zero_rows, red);
}

}  // namespace

extern "C" {

int rlx_classification_head_loss(const float *logits, long long ld, const int *actions, const float *labels,
                                 long long ld_labels, float grad_scale, int rows, int n_actions, float *dlogits,
                                 long long ld_dlogits, float *probs_out, long long ld_probs, float *row_loss_out,
                                 float *scalars, int *status, void *stream) {
    RLX_REQUIRE(logits && dlogits && scalars && status, "rlx_classification_head_loss: null pointer");
    RLX_REQUIRE((actions != nullptr) != (labels != nullptr),
                "rlx_classification_head_loss: exactly one of actions and labels is given (got %s)",
                actions ? "both" : "neither");
    RLX_REQUIRE(rows >= 1 && rows <= kMaxRows && n_actions >= 1 && n_actions <= kMaxActions,
                "rlx_classification_head_loss: bad sizes (1 <= rows=%d <= 1024, 1 <= actions=%d <= 18)", rows, n_actions);
    RLX_REQUIRE(ld >= n_actions && ld_dlogits >= n_actions && (!labels || ld_labels >= n_actions) &&
                    (!probs_out || ld_probs >= n_actions),
                "rlx_classification_head_loss: leading dimension < actions (%d)", n_actions);
    ClsArgs a;
    a.logits = logits; a.ld = ld; a.actions = actions; a.labels = labels; a.ld_l = ld_labels; a.grad_scale = grad_scale;
    a.rows = rows; a.A = n_actions; a.dlogits = dlogits; a.ld_d = ld_dlogits; a.probs = probs_out; a.ld_p = ld_probs;
    a.row_loss = row_loss_out; a.scalars = scalars; a.status = status;
    RLX_LAUNCH((classification_head_loss_kernel), 1, rlx::bcq_selector_threads(rows), 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_bcq_imitation_selector(const float *q_next_online, long long ld_q, const float *imitation, long long ld_i,
                               float threshold, int flags, int batch, int n_actions, unsigned int seed,
                               unsigned int rank, const long long *event, float *sel_out, long long ld_sel,
                               float *familiarity_out, long long ld_f, int *zero_rows_out, void *stream) {
    RLX_REQUIRE(q_next_online && imitation && event && sel_out, "rlx_bcq_imitation_selector: null pointer");
    RLX_REQUIRE((flags & ~RLX_IMITATION_INPUT_PROBS) == 0, "rlx_bcq_imitation_selector: unknown flags %d", flags);
    RLX_REQUIRE(batch > 0 && batch <= kMaxRows && n_actions > 0 && n_actions <= kMaxActions,
                "rlx_bcq_imitation_selector: bad sizes (batch=%d <= 1024, actions=%d <= 18)", batch, n_actions);
    RLX_REQUIRE(ld_q >= n_actions && ld_i >= n_actions && ld_sel >= n_actions && (!familiarity_out || ld_f >= n_actions),
                "rlx_bcq_imitation_selector: leading dimension < actions (%d)", n_actions);
    ImSelArgs a;
    a.q = q_next_online; a.ld_q = ld_q; a.im = imitation; a.ld_i = ld_i; a.threshold = threshold;
    a.probs_in = (flags & RLX_IMITATION_INPUT_PROBS) ? 1 : 0;
    a.batch = batch; a.n_actions = n_actions; a.seed = seed; a.rank = rank; a.event = event;
    a.sel = sel_out; a.ld_sel = ld_sel; a.fam = familiarity_out; a.ld_f = ld_f; a.zero_rows = zero_rows_out;
    RLX_LAUNCH((bcq_imitation_selector_kernel), 1, rlx::bcq_selector_threads(batch), 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
