// Batch-constrained Q-learning (the DDQN-BCQ agent of Batch RL) on gfx950: the exact nearest-neighbour distances behind
// its action mask, and the masked Double-DQN selector.
//
// Replaces, in the reference (paths under rl_coach/):
//   * AnnoyDictionary._get_k_nearest_neighbors_indices(keys, 1)   memories/non_episodic/differentiable_neural_dictionary.py
//     as DDQNBCQAgent uses it (agents/ddqn_bcq_agent.py:109-111, :212-214): per action, the Euclidean distance from each
//     embedded state to its nearest stored embedding.  The reference searches an approximate Annoy forest on the host,
//     one query at a time; here the search is exact and one pass over the keys.
//   * DDQNBCQAgent.select_actions up to its argmax                 agents/ddqn_bcq_agent.py:107-133
//
// rlx_nn_min_distance.  The arithmetic is fixed so that numpy restates it bit for bit (tests/bcq_ref.py): per (query,
// key) pair acc = 0; for w = 0 .. width-1 in this order t = q[w] - k[w], acc = acc + t * t, every operation rounded to
// fp32 on its own (this file is compiled with -ffp-contract=off); a set's value is the minimum of acc over its keys —
// exact in any order — and then one correctly rounded square root.  Never |q|^2 + |k|^2 - 2 q.k: that form cancels
// near zero, and a query that IS one of the keys (the usual case: the keys are the dataset's states) must give 0.
//
// One workgroup of 256 threads (wave64 x 4) per (key chunk of kKeyChunk keys, tile of kQueryTile queries, set).  The
// width is walked in tiles of kWidthTile floats: the workgroup brings the query tile and the key tile into LDS with
// 16-byte global loads (scalar loads where a base or a leading dimension is not 16-byte aligned, zeros beyond the
// width: (0 - 0)^2 added to a non-negative acc changes nothing), and every lane keeps a 4 x 4 register block of
// (query, key) accumulators, so that one 16-byte LDS read feeds four pairs.  LDS rows are padded by four floats: the
// 32 key rows a half-wave reads then fall on distinct banks.  The accumulators stay in registers across width tiles,
// which keeps the order of the additions.  The block's minima are reduced over the 32 lanes that share a query by
// shuffles and combined across key chunks by an integer atomicMin on the bit pattern of the squared distance (never
// negative, so the unsigned order is the float order: deterministic).  Two small launches frame it: +inf into
// dist_out[i][s] before, the square root after.  An empty set keeps +inf.
//
// rlx_bcq_masked_selector.  One workgroup, one row per thread (batch <= 1024, as rlx_dqn_head_loss).  Its row tail (the
// draws of a row that keeps no action, the count of such rows) is bcq_selector_tail.hpp's, shared with imitation.hip.
#include "bcq_selector_tail.hpp"

namespace {

constexpr int kKeyChunk = RLX_NN_KEY_CHUNK;     // keys of one workgroup
constexpr int kQueryTile = 32;                  // queries of one workgroup
constexpr int kWidthTile = 32;                  // floats of the width per LDS fill
constexpr int kRow = kWidthTile + 4;            // padded LDS row, in floats (a multiple of 4: rows stay 16-byte aligned)
constexpr int kThreads = 256;
static_assert(kKeyChunk == 128 && kQueryTile == 32 && kThreads == 256, "the lane -> (4 queries, 4 keys) map below");

constexpr unsigned kInfBits = 0x7f800000u;

struct NnArgs {
    const float *q; long long ld_q; int n_queries, width;
    const float *k; long long ld_k; long long n_keys;
    const int *set_offsets; int n_sets;
    float *out; long long ld_out;
    int vec_q, vec_k;                            // 16-byte global loads are legal on the operand
};

// floats [w0 + 4 c, w0 + 4 c + 4) of row `row` of `base` (zeros beyond the width or where the row does not exist)
__device__ __forceinline__ float4 load4(const float *base, long long ld, long long row, bool row_ok, int w, int width,
                                        int vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!row_ok) return v;
    const float *p = base + (size_t)row * (size_t)ld + w;
    if (vec && w + 3 < width) return *reinterpret_cast<const float4 *>(p);
    if (w < width) v.x = p[0];
    if (w + 1 < width) v.y = p[1];
    if (w + 2 < width) v.z = p[2];
    if (w + 3 < width) v.w = p[3];
    return v;
}

__global__ void __launch_bounds__(kThreads) nn_fill_inf_kernel(float *out, long long ld_out, int n_queries, int n_sets) {
    const long long n = (long long)n_queries * n_sets;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        reinterpret_cast<unsigned *>(out)[(size_t)(i / n_sets) * (size_t)ld_out + (size_t)(i % n_sets)] = kInfBits;
}

__global__ void __launch_bounds__(kThreads) nn_sqrt_kernel(float *out, long long ld_out, int n_queries, int n_sets) {
    const long long n = (long long)n_queries * n_sets;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float *p = out + (size_t)(i / n_sets) * (size_t)ld_out + (size_t)(i % n_sets);
        // the correctly rounded fp32 root: llvm.sqrt.f64 is correctly rounded and 53 >= 2 * 24 + 2 bits make the second
        // rounding innocuous (the fp32 square-root instruction alone is good to 1 ulp only)
        *p = (float)__builtin_sqrt((double)*p);
    }
}

__global__ void __launch_bounds__(kThreads) nn_min_distance_kernel(const NnArgs a) {
    __shared__ __attribute__((aligned(16))) float Qs[kQueryTile * kRow];
    __shared__ __attribute__((aligned(16))) float Ks[kKeyChunk * kRow];
    const int tid = threadIdx.x, set = blockIdx.z;
    long long beg = a.set_offsets[set], end = a.set_offsets[set + 1];
    if (beg < 0) beg = 0;
    if (end > a.n_keys) end = a.n_keys;                       // a bad offset table cannot make the launch read past the keys
    const long long key0 = beg + (long long)blockIdx.x * kKeyChunk;
    if (key0 >= end) return;                                  // uniform over the workgroup: before any barrier
    const int q0 = blockIdx.y * kQueryTile;
    const int tk = tid & 31, tq = tid >> 5;                   // keys tk + 32 j, queries 4 tq + i
    const int lrow = tid >> 3, lcol = (tid & 7) * 4;          // the fills: row lrow (+ 32 r), floats lcol .. lcol + 3

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    for (int w0 = 0; w0 < a.width; w0 += kWidthTile) {
        const float4 qv = load4(a.q, a.ld_q, q0 + lrow, q0 + lrow < a.n_queries, w0 + lcol, a.width, a.vec_q);
        float4 kv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
            kv[r] = load4(a.k, a.ld_k, key0 + lrow + 32 * r, key0 + lrow + 32 * r < end, w0 + lcol, a.width, a.vec_k);
        __syncthreads();                                      // the previous tile's reads are done
        *reinterpret_cast<float4 *>(&Qs[lrow * kRow + lcol]) = qv;
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<float4 *>(&Ks[(lrow + 32 * r) * kRow + lcol]) = kv[r];
        __syncthreads();
#pragma unroll 2
        for (int c = 0; c < kWidthTile; c += 4) {
            float4 qr[4], kr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) qr[i] = *reinterpret_cast<const float4 *>(&Qs[(4 * tq + i) * kRow + c]);
#pragma unroll
            for (int j = 0; j < 4; ++j) kr[j] = *reinterpret_cast<const float4 *>(&Ks[(tk + 32 * j) * kRow + c]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {                 // w in order: x, y, z, w of the pair's own accumulator
                    float t = qr[i].x - kr[j].x;
                    float s = acc[i][j] + t * t;
                    t = qr[i].y - kr[j].y;
                    s = s + t * t;
                    t = qr[i].z - kr[j].z;
                    s = s + t * t;
                    t = qr[i].w - kr[j].w;
                    acc[i][j] = s + t * t;
                }
        }
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned m = kInfBits;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (key0 + tk + 32 * j < end) m = min(m, __float_as_uint(acc[i][j]));
#pragma unroll
        for (int d = 16; d > 0; d >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, d));   // stays inside the 32 lanes of tq
        const int qi = q0 + 4 * tq + i;
        if (tk == 0 && qi < a.n_queries)
            atomicMin(reinterpret_cast<unsigned *>(a.out) + (size_t)qi * (size_t)a.ld_out + set, m);
    }
}

struct SelArgs {
    const float *q; long long ld_q;
    const float *fam; long long ld_f;
    double threshold;
    int batch, n_actions;
    uint32_t seed, rank;
    const long long *event;
    float *sel; long long ld_sel;
    int *zero_rows;
};

__global__ void __launch_bounds__(1024) bcq_masked_selector_kernel(const SelArgs a) {
    __shared__ int red[rlx::kBcqSelectorMaxBatch];
    const int b = threadIdx.x, A = a.n_actions;
    int zero = 0;
    if (b < a.batch) {
        const float *q = a.q + (size_t)b * a.ld_q, *f = a.fam + (size_t)b * a.ld_f;
        float *s = a.sel + (size_t)b * a.ld_sel;
        // ddqn_bcq_agent.py:129: the row's maximum is -inf — every action masked (or its own Q value -inf already)
        zero = 1;
        for (int k = 0; k < A; ++k) {
            const float v = (double)f[k] > a.threshold ? -INFINITY : q[k];
            if (!(v == -INFINITY)) zero = 0;
            s[k] = v;
        }
        if (zero) rlx::bcq_zero_row_draws(s, b, A, a.seed, a.rank, a.event);      // bcq_selector_tail.hpp
    }
    rlx::bcq_zero_row_count(zero, a.zero_rows, red);
}

// The reward model's targets (agents/value_optimization_agent.py:173-180): the prediction with the taken action's
// entry replaced by the reward; status bit 1: an action outside [0, n_actions) (the row stays the prediction).
__global__ void __launch_bounds__(kThreads) reward_model_targets_kernel(const float *pred, long long ld_p, const int *actions,
                                                                      const float *rewards, int batch, int n_actions,
                                                                      float *targets, long long ld_t, int *status) {
    const long long n = (long long)batch * n_actions;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / n_actions), k = (int)(i % n_actions), act = actions[b];
        if (k == 0 && (act < 0 || act >= n_actions)) atomicOr(status, 1);
        targets[(size_t)b * ld_t + k] = k == act ? rewards[b] : pred[(size_t)b * ld_p + k];
    }
}

}  // namespace

extern "C" {

int rlx_nn_min_distance(const float *queries, long long ld_q, int n_queries, int width, const float *keys,
                        long long ld_k, long long n_keys, const int *set_offsets, int n_sets, float *dist_out,
                        long long ld_out, void *stream) {
    RLX_REQUIRE(queries && set_offsets && dist_out && (keys || n_keys == 0), "rlx_nn_min_distance: null pointer");
    RLX_REQUIRE(width >= 1 && width <= 512, "rlx_nn_min_distance: width %d outside [1, 512]", width);
    RLX_REQUIRE(n_sets >= 1 && n_sets <= 18, "rlx_nn_min_distance: n_sets %d outside [1, 18]", n_sets);
    RLX_REQUIRE(n_queries >= 1 && n_keys >= 0 && n_keys <= 0x7fffffffLL,
                "rlx_nn_min_distance: bad sizes (queries=%d, keys=%lld)", n_queries, n_keys);
    RLX_REQUIRE(ld_q >= width && ld_k >= width, "rlx_nn_min_distance: leading dimension < width (%d)", width);
    RLX_REQUIRE(ld_out >= n_sets, "rlx_nn_min_distance: ld_out < n_sets (%d)", n_sets);
    hipStream_t s = rlx::as_stream(stream);
    const int small = rlx::grid_for((long long)n_queries * n_sets, kThreads);
    RLX_LAUNCH((nn_fill_inf_kernel), small, kThreads, 0, s, dist_out, ld_out, n_queries, n_sets);
    RLX_LAUNCH_CHECK();
    if (n_keys > 0) {
        NnArgs a;
        a.q = queries; a.ld_q = ld_q; a.n_queries = n_queries; a.width = width;
        a.k = keys; a.ld_k = ld_k; a.n_keys = n_keys;
        a.set_offsets = set_offsets; a.n_sets = n_sets;
        a.out = dist_out; a.ld_out = ld_out;
        a.vec_q = ((uintptr_t)queries % 16 == 0 && ld_q % 4 == 0) ? 1 : 0;
        a.vec_k = ((uintptr_t)keys % 16 == 0 && ld_k % 4 == 0) ? 1 : 0;
        const long long chunks = (n_keys + kKeyChunk - 1) / kKeyChunk;      // no set holds more than all the keys
        const int tiles = (n_queries + kQueryTile - 1) / kQueryTile;
        RLX_REQUIRE(tiles <= 65535, "rlx_nn_min_distance: more than %d queries", 65535 * kQueryTile);
        RLX_LAUNCH((nn_min_distance_kernel), dim3((unsigned)chunks, (unsigned)tiles, (unsigned)n_sets), kThreads, 0, s, a);
        RLX_LAUNCH_CHECK();
    }
    RLX_LAUNCH((nn_sqrt_kernel), small, kThreads, 0, s, dist_out, ld_out, n_queries, n_sets);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_bcq_masked_selector(const float *q_next_online, long long ld_q, const float *familiarity, long long ld_f,
                            double threshold, int batch, int n_actions, unsigned int seed, unsigned int rank,
                            const long long *event, float *sel_out, long long ld_sel, int *zero_rows_out, void *stream) {
    RLX_REQUIRE(q_next_online && familiarity && event && sel_out, "rlx_bcq_masked_selector: null pointer");
    RLX_REQUIRE(batch > 0 && batch <= 1024 && n_actions > 0 && n_actions <= 18,
                "rlx_bcq_masked_selector: bad sizes (batch=%d <= 1024, actions=%d <= 18)", batch, n_actions);
    RLX_REQUIRE(ld_q >= n_actions && ld_f >= n_actions && ld_sel >= n_actions,
                "rlx_bcq_masked_selector: leading dimension < actions (%d)", n_actions);
    SelArgs a;
    a.q = q_next_online; a.ld_q = ld_q; a.fam = familiarity; a.ld_f = ld_f; a.threshold = threshold;
    a.batch = batch; a.n_actions = n_actions; a.seed = seed; a.rank = rank; a.event = event;
    a.sel = sel_out; a.ld_sel = ld_sel; a.zero_rows = zero_rows_out;
    RLX_LAUNCH((bcq_masked_selector_kernel), 1, rlx::bcq_selector_threads(batch), 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_reward_model_targets(const float *prediction, long long ld_p, const int *actions, const float *rewards, int batch,
                             int n_actions, float *targets, long long ld_t, int *status, void *stream) {
    RLX_REQUIRE(prediction && actions && rewards && targets && status, "rlx_reward_model_targets: null pointer");
    RLX_REQUIRE(batch > 0 && n_actions > 0, "rlx_reward_model_targets: bad sizes (batch=%d, actions=%d)", batch, n_actions);
    RLX_REQUIRE(ld_p >= n_actions && ld_t >= n_actions, "rlx_reward_model_targets: leading dimension < actions (%d)",
                n_actions);
    RLX_LAUNCH((reward_model_targets_kernel), rlx::grid_for((long long)batch * n_actions, kThreads), kThreads, 0,
               rlx::as_stream(stream), prediction, ld_p, actions, rewards, batch, n_actions, targets, ld_t, status);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
