// The Wolpertinger agent ("Deep Reinforcement Learning in Large Discrete Action Spaces", Dulac-Arnold et al. 2015) on
// gfx950: the exact, ordered k-nearest-neighbour lookup of the actor's proto-action among the discrete actions'
// embeddings, the critic's candidate rows, the choice among them, and the discrete -> box conversion of a batch.
//
// Replaces, in the reference (paths under rl_coach/):
//   * AnnoyDictionary.query as WolpertingerAgent.choose_action uses it      agents/wolpertinger_agent.py:92-100,
//     memories/non_episodic/differentiable_neural_dictionary.py: an approximate Annoy forest on the host, one query at a
//     time; here the search is exact, ordered and one pass over the keys for a whole tile of queries.
//   * np.tile(observation, (k, 1)) / nn_action_embeddings[0]                agents/wolpertinger_agent.py:103-105
//   * int(indices[0][np.argmax(q_values)]) and BoxDiscretization.filter     agents/wolpertinger_agent.py:106-107,
//                                                                           filters/action/partial_discrete_action_space_map.py
//   * the per-row filter loop of WolpertingerAgent.learn_from_batch         agents/wolpertinger_agent.py:77-83
//
// rlx_knn_topk.  The squared distance is rlx_nn_min_distance's (csrc/bcq.hip), word for word: acc = 0; for w = 0 ..
// width-1 in this order t = q[w] - key[w], acc = acc + t * t, every operation rounded to fp32 on its own (this file is
// compiled with -ffp-contract=off); never |q|^2 + |k|^2 - 2 q.k.  Every (query, key) pair becomes ONE 64-bit word,
// (bit pattern of acc) << 32 | key index, a NaN's bit pattern replaced by 0xffffffff: acc is never negative, so the
// unsigned order of the words is ascending (distance, index) with NaN behind +inf — equal distances go to the lower
// index, and no word occurs twice.  The k smallest words are the answer; minima of integers are exact in any order, so
// nothing depends on the order in which workgroups run, and there are no atomics.
//
// One workgroup of 256 threads (wave64 x 4) covers ONE chunk of kKeyChunk = 2048 keys (eight per thread) and a tile of
// kQueryTile = 16 queries, which it walks one after the other: the thread's eight words, then k rounds of "the
// workgroup's minimum" (every wave's minimum — the thread's own, then six shuffle steps — through four words of LDS, one
// barrier per round); the owner of a round's winner retires that word and only its wave works out a new minimum, thread r
// keeps round r's winner in a register and the k winners are stored together after the last round.  The chunk's list of k words (padded with ~0 when the
// chunk has fewer than k keys) goes to the caller's scratch.  With width <= 4 the thread's keys stay in registers for
// the whole tile (one 16-byte load brings four keys of a width-1, ld-1 table; a 16-byte row load where base and leading
// dimension allow; scalar loads otherwise); wider keys are re-read per query in 16-byte (or scalar) steps from L2.
// Merge passes follow while more than one list per query is left: one workgroup takes up to 2048 / k consecutive lists
// (2048 words, eight per thread) and selects their k smallest the same way.  The last pass — the search itself when the
// keys fit one chunk — writes idx_out / dist2_out (a NaN distance as the quiet NaN 0x7fc00000) instead of a list.
// A call is 1 + ceil(log_{2048 / k}(chunks)) launches: 1 up to 2048 keys, 2 up to 2048 * (2048 / k), 3 for the preset's
// 10^6 keys only when k > 4.  No allocation, no synchronisation: capturable.
//
// rlx_wolpertinger_candidates is a launch of its own (the proto-actions' neighbours are known only after the last merge
// pass, and the observation rows are wider than that pass's output); rlx_wolpertinger_select one thread per env;
// rlx_discrete_to_box one thread per output word.
#include "rlx_common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kSlots = 8;                         // words of one thread
constexpr int kKeyChunk = RLX_KNN_KEY_CHUNK;      // keys of one search workgroup = words of one merge workgroup
constexpr int kQueryTile = 16;                    // queries of one search workgroup
constexpr int kMaxWidth = 64;
constexpr int kMaxK = 64;
static_assert(kKeyChunk == kThreads * kSlots, "eight words per thread");

typedef unsigned long long u64;
constexpr u64 kNone = ~0ull;                      // no word: above every (distance, index) word (index < 2^31 - 1)

__device__ __forceinline__ u64 make_word(float acc, long long key) {
    const unsigned bits = acc != acc ? 0xffffffffu : __float_as_uint(acc);
    return ((u64)bits << 32) | (u64)(unsigned)key;
}

struct TopkOut {
    u64 *lists;                                   // [n_queries][lists_out][k], or null: the final pass
    long long lists_out;
    int *idx; float *dist2;                       // [n_queries][k] (dist2 optional)
    int k;
};

// the minimum of the wave's 64 * kSlots words, in every lane of the wave
__device__ __forceinline__ u64 wave_min(const u64 (&w)[kSlots]) {
    u64 m = w[0];
#pragma unroll
    for (int s = 1; s < kSlots; ++s) m = w[s] < m ? w[s] : m;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const u64 other = __shfl_xor(m, d);
        m = other < m ? other : m;
    }
    return m;
}

// The k smallest of the workgroup's kThreads * kSlots words, ascending, to list `list` of query `q` (or to idx / dist2).
// Every thread of the workgroup calls it; `red` is 2 x 4 words of LDS.
__device__ __forceinline__ void select_k(u64 (&w)[kSlots], u64 (*red)[4], const TopkOut &o, int q, long long list) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    u64 wm = wave_min(w);            // kept across rounds: only the wave that held a round's winner has a new minimum
    u64 mine = kNone;                // round tid's winner: thread r < k keeps round r's, and stores it after the last round
    for (int r = 0; r < o.k; ++r) {
        if (lane == 0) red[r & 1][wave] = wm;
        __syncthreads();             // round r + 1 writes the other half; round r + 2 comes after the next barrier
        u64 best = red[r & 1][0];
#pragma unroll
        for (int v = 1; v < kThreads / 64; ++v) best = red[r & 1][v] < best ? red[r & 1][v] : best;
        if (tid == r) mine = best;   // (the k winners go out together below: one coalesced store per list)
        if (wm == best && best != kNone) {        // uniform over the wave; words are unique: one wave, one owner
#pragma unroll
            for (int s = 0; s < kSlots; ++s)
                if (w[s] == best) w[s] = kNone;
            wm = wave_min(w);
        }
    }
    if (tid < o.k) {
        if (o.lists) {
            o.lists[((size_t)q * (size_t)o.lists_out + (size_t)list) * (size_t)o.k + tid] = mine;
        } else {
            const unsigned hi = (unsigned)(mine >> 32);
            o.idx[(size_t)q * o.k + tid] = (int)(unsigned)mine;
            if (o.dist2) reinterpret_cast<unsigned *>(o.dist2)[(size_t)q * o.k + tid] = hi == 0xffffffffu ? 0x7fc00000u : hi;
        }
    }
    __syncthreads();                 // the next query's first round writes red[0] again
}

struct SearchArgs {
    const float *q; long long ld_q; int n_queries, width;
    const float *k; long long ld_k; long long n_keys;
    int vec_q, vec_k, vec_keys4;     // 16-byte loads are legal along a row of q / of k; across four keys of a width-1 table
    TopkOut out;
};

// floats [w, w + 4) of row `row` of `base`, zeros beyond the width: (0 - 0)^2 added to a non-negative acc changes nothing
__device__ __forceinline__ float4 load4(const float *base, long long ld, long long row, int w, int width, int vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const float *p = base + (size_t)row * (size_t)ld + w;
    if (vec && w + 3 < width) return *reinterpret_cast<const float4 *>(p);
    if (w < width) v.x = p[0];
    if (w + 1 < width) v.y = p[1];
    if (w + 2 < width) v.z = p[2];
    if (w + 3 < width) v.w = p[3];
    return v;
}

__device__ __forceinline__ float dist4(float acc, const float4 &q, const float4 &k) {   // w in order: x, y, z, w
    float t = q.x - k.x;
    acc = acc + t * t;
    t = q.y - k.y;
    acc = acc + t * t;
    t = q.z - k.z;
    acc = acc + t * t;
    t = q.w - k.w;
    return acc + t * t;
}

__global__ void __launch_bounds__(kThreads) knn_search_kernel(const SearchArgs a) {
    __shared__ __attribute__((aligned(16))) float Qs[kQueryTile * kMaxWidth];
    __shared__ u64 red[2][4];
    const int tid = threadIdx.x;
    const long long chunk = blockIdx.x, key0 = chunk * kKeyChunk;
    const int q0 = blockIdx.y * kQueryTile;
    const int nq = min(kQueryTile, a.n_queries - q0);
    const int wpad = (a.width + 3) & ~3;

    static_assert(kQueryTile * kMaxWidth / 4 == kThreads, "one float4 of the query tile per thread");
    {
        const int qi = tid / (kMaxWidth / 4), w = (tid % (kMaxWidth / 4)) * 4;
        *reinterpret_cast<float4 *>(&Qs[qi * kMaxWidth + w]) =
            qi < nq ? load4(a.q, a.ld_q, q0 + qi, w, a.width, a.vec_q) : make_float4(0.f, 0.f, 0.f, 0.f);
    }

    // slot s of this thread: key index, or -1 past the table
    long long key[kSlots];
    const bool small = a.width <= 4;
    float4 kreg[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        const long long kk = a.vec_keys4 ? key0 + (long long)(s >> 2) * (kThreads * 4) + tid * 4 + (s & 3)
                                         : key0 + (long long)s * kThreads + tid;
        key[s] = kk < a.n_keys ? kk : -1;
        kreg[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (small) {
        if (a.vec_keys4) {           // width 1, ld 1: four keys per 16-byte load where all four exist
#pragma unroll
            for (int g = 0; g < kSlots / 4; ++g) {
                if (key[4 * g + 3] >= 0) {
                    const float4 v = *reinterpret_cast<const float4 *>(a.k + key[4 * g]);
                    kreg[4 * g].x = v.x; kreg[4 * g + 1].x = v.y; kreg[4 * g + 2].x = v.z; kreg[4 * g + 3].x = v.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (key[4 * g + j] >= 0) kreg[4 * g + j].x = a.k[key[4 * g + j]];
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < kSlots; ++s)
                if (key[s] >= 0) kreg[s] = load4(a.k, a.ld_k, key[s], 0, a.width, a.vec_k);
        }
    }
    __syncthreads();

    for (int qi = 0; qi < nq; ++qi) {             // nq is uniform over the workgroup: select_k's barriers are taken by all
        const float *qrow = &Qs[qi * kMaxWidth];
        u64 w[kSlots];
        if (small) {
            const float4 qv = *reinterpret_cast<const float4 *>(qrow);
#pragma unroll
            for (int s = 0; s < kSlots; ++s) w[s] = key[s] >= 0 ? make_word(dist4(0.f, qv, kreg[s]), key[s]) : kNone;
        } else {
#pragma unroll
            for (int s = 0; s < kSlots; ++s) {
                w[s] = kNone;
                if (key[s] >= 0) {
                    float acc = 0.f;
                    for (int c = 0; c < wpad; c += 4)
                        acc = dist4(acc, *reinterpret_cast<const float4 *>(qrow + c),
                                    load4(a.k, a.ld_k, key[s], c, a.width, a.vec_k));
                    w[s] = make_word(acc, key[s]);
                }
            }
        }
        select_k(w, red, a.out, q0 + qi, chunk);
    }
}

struct MergeArgs {
    const u64 *in; long long lists_in;            // [n_queries][lists_in][k]
    int fan;                                      // lists of one workgroup: fan * k <= kKeyChunk
    TopkOut out;
};

__global__ void __launch_bounds__(kThreads) knn_merge_kernel(const MergeArgs a) {
    __shared__ u64 red[2][4];
    const int tid = threadIdx.x, q = blockIdx.y;
    const long long group = blockIdx.x, first = group * a.fan;
    const long long lists = min((long long)a.fan, a.lists_in - first);
    const long long words = lists * a.out.k;      // <= kKeyChunk
    const u64 *src = a.in + ((size_t)q * (size_t)a.lists_in + (size_t)first) * (size_t)a.out.k;
    u64 w[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        const long long i = (long long)s * kThreads + tid;
        w[s] = i < words ? src[i] : kNone;
    }
    select_k(w, red, a.out, q, group);
}

// critic inputs: row e * k + j <- (env e's observation, keys[idx[e][j]]); an index outside the table gives a zero key
__global__ void __launch_bounds__(kThreads) wolpertinger_candidates_kernel(
        const int *idx, const float *keys, long long ld_k, long long n_keys, int width, const float *obs, long long ld_obs,
        int obs_dim, int n_env, int k, float *obs_out, long long ld_oo, float *act_out, long long ld_ao) {
    const int per = obs_dim + width;
    const long long n = (long long)n_env * k * per;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / per;
        const int c = (int)(i % per), e = (int)(row / k);
        if (c < obs_dim) {
            obs_out[(size_t)row * ld_oo + c] = obs[(size_t)e * ld_obs + c];
        } else {
            const long long key = idx[row];
            act_out[(size_t)row * ld_ao + (c - obs_dim)] =
                (key >= 0 && key < n_keys) ? keys[(size_t)key * ld_k + (c - obs_dim)] : 0.f;
        }
    }
}

__global__ void __launch_bounds__(kThreads) wolpertinger_select_kernel(
        const float *q, long long q_stride, const int *idx, int n_env, int k, const float *table, long long ld_t,
        long long n_actions, int action_dim, int *action_out, float *env_action_out, long long ld_e) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    const float *qe = q + (size_t)e * k * (size_t)q_stride;
    float bv = qe[0];
    int best = 0;
    for (int j = 1; j < k; ++j) rlx::np_argmax_step(qe[(size_t)j * q_stride], j, bv, best);
    const int act = idx[(size_t)e * k + best];
    action_out[e] = act;
    const bool ok = act >= 0 && act < n_actions;
    for (int d = 0; d < action_dim; ++d)
        env_action_out[(size_t)e * ld_e + d] = ok ? table[(size_t)act * ld_t + d] : 0.f;
}

// status bit 1: an action outside [0, n_actions) (its row is zero)
__global__ void __launch_bounds__(kThreads) discrete_to_box_kernel(const int *actions, int batch, const float *table,
                                                                  long long ld_t, long long n_actions, int action_dim,
                                                                  float *out, long long ld_out, int *status) {
    const long long n = (long long)batch * action_dim;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / action_dim), d = (int)(i % action_dim), act = actions[b];
        const bool ok = act >= 0 && act < n_actions;
        if (!ok && d == 0) atomicOr(status, 1);
        out[(size_t)b * ld_out + d] = ok ? table[(size_t)act * ld_t + d] : 0.f;
    }
}

// lists left after one merge pass over `lists` lists of k words
inline long long merged_lists(long long lists, int k) {
    const int fan = kKeyChunk / k;
    return (lists + fan - 1) / fan;
}

int check_topk_sizes(const char *who, int n_queries, long long n_keys, int k) {
    RLX_REQUIRE(k >= 1 && k <= kMaxK, "%s: k %d outside [1, %d]", who, k, kMaxK);
    RLX_REQUIRE(n_keys >= k && n_keys <= 0x7fffffffLL, "%s: n_keys %lld outside [k = %d, 2^31 - 1]", who, n_keys, k);
    RLX_REQUIRE(n_queries >= 1 && n_queries <= 65535, "%s: n_queries %d outside [1, 65535]", who, n_queries);
    return RLX_OK;
}

}  // namespace

extern "C" {

int rlx_knn_topk_scratch_bytes(int n_queries, long long n_keys, int k, long long *bytes_out) {
    RLX_REQUIRE(bytes_out, "rlx_knn_topk_scratch_bytes: null pointer");
    if (int rc = check_topk_sizes("rlx_knn_topk_scratch_bytes", n_queries, n_keys, k)) return rc;
    const long long chunks = (n_keys + kKeyChunk - 1) / kKeyChunk;
    // the search's lists and the first merge pass's; later passes alternate between the two
    const long long words = chunks > 1 ? (chunks + merged_lists(chunks, k)) * k * (long long)n_queries : 0;
    *bytes_out = words * (long long)sizeof(u64);
    return RLX_OK;
}

int rlx_knn_topk(const float *queries, long long ld_q, int n_queries, int width, const float *keys, long long ld_k,
                 long long n_keys, int k, int *idx_out, float *dist2_out, void *scratch, long long scratch_bytes,
                 void *stream) {
    RLX_REQUIRE(queries && keys && idx_out, "rlx_knn_topk: null pointer");
    RLX_REQUIRE(width >= 1 && width <= kMaxWidth, "rlx_knn_topk: width %d outside [1, %d]", width, kMaxWidth);
    if (int rc = check_topk_sizes("rlx_knn_topk", n_queries, n_keys, k)) return rc;
    RLX_REQUIRE(ld_q >= width && ld_k >= width, "rlx_knn_topk: leading dimension < width (%d)", width);
    long long need = 0;
    if (int rc = rlx_knn_topk_scratch_bytes(n_queries, n_keys, k, &need)) return rc;
    RLX_REQUIRE(need == 0 || (scratch && scratch_bytes >= need && (uintptr_t)scratch % 8 == 0),
                "rlx_knn_topk: scratch of %lld bytes (8-byte aligned) needed, %lld given", need, scratch_bytes);
    hipStream_t s = rlx::as_stream(stream);
    const long long chunks = (n_keys + kKeyChunk - 1) / kKeyChunk;
    const int tiles = (n_queries + kQueryTile - 1) / kQueryTile;
    u64 *buf[2] = {static_cast<u64 *>(scratch), static_cast<u64 *>(scratch) + chunks * k * (long long)n_queries};

    SearchArgs a;
    a.q = queries; a.ld_q = ld_q; a.n_queries = n_queries; a.width = width;
    a.k = keys; a.ld_k = ld_k; a.n_keys = n_keys;
    a.vec_q = ((uintptr_t)queries % 16 == 0 && ld_q % 4 == 0) ? 1 : 0;
    a.vec_k = ((uintptr_t)keys % 16 == 0 && ld_k % 4 == 0) ? 1 : 0;
    a.vec_keys4 = (width == 1 && ld_k == 1 && (uintptr_t)keys % 16 == 0) ? 1 : 0;
    a.out.k = k; a.out.idx = idx_out; a.out.dist2 = dist2_out;
    a.out.lists = chunks > 1 ? buf[0] : nullptr;
    a.out.lists_out = chunks;
    RLX_LAUNCH((knn_search_kernel), dim3((unsigned)chunks, (unsigned)tiles), kThreads, 0, s, a);
    RLX_LAUNCH_CHECK();

    long long lists = chunks;
    for (int pass = 0; lists > 1; ++pass) {
        MergeArgs m;
        m.in = buf[pass & 1]; m.lists_in = lists; m.fan = kKeyChunk / k;
        const long long left = merged_lists(lists, k);
        m.out = a.out;
        m.out.lists = left > 1 ? buf[(pass + 1) & 1] : nullptr;
        m.out.lists_out = left;
        RLX_LAUNCH((knn_merge_kernel), dim3((unsigned)left, (unsigned)n_queries), kThreads, 0, s, m);
        RLX_LAUNCH_CHECK();
        lists = left;
    }
    return RLX_OK;
}

int rlx_wolpertinger_candidates(const int *idx, const float *keys, long long ld_k, long long n_keys, int width,
                                const float *observations, long long ld_obs, int obs_dim, int n_env, int k,
                                float *obs_out, long long ld_obs_out, float *action_out, long long ld_action_out,
                                void *stream) {
    RLX_REQUIRE(idx && keys && observations && obs_out && action_out, "rlx_wolpertinger_candidates: null pointer");
    RLX_REQUIRE(n_env >= 1 && k >= 1 && k <= kMaxK && width >= 1 && width <= kMaxWidth && obs_dim >= 1 && n_keys >= 1,
                "rlx_wolpertinger_candidates: bad sizes (envs=%d, k=%d <= %d, width=%d <= %d, obs=%d, keys=%lld)", n_env, k,
                kMaxK, width, kMaxWidth, obs_dim, n_keys);
    RLX_REQUIRE(ld_k >= width && ld_action_out >= width && ld_obs >= obs_dim && ld_obs_out >= obs_dim,
                "rlx_wolpertinger_candidates: leading dimension < row (width=%d, obs=%d)", width, obs_dim);
    RLX_LAUNCH((wolpertinger_candidates_kernel), rlx::grid_for((long long)n_env * k * (obs_dim + width), kThreads), kThreads,
               0, rlx::as_stream(stream), idx, keys, ld_k, n_keys, width, observations, ld_obs, obs_dim, n_env, k, obs_out,
               ld_obs_out, action_out, ld_action_out);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_wolpertinger_select(const float *q, long long q_stride, const int *idx, int n_env, int k,
                            const float *target_actions, long long ld_t, long long n_actions, int action_dim,
                            int *action_out, float *env_action_out, long long ld_env, void *stream) {
    RLX_REQUIRE(q && idx && target_actions && action_out && env_action_out, "rlx_wolpertinger_select: null pointer");
    RLX_REQUIRE(n_env >= 1 && k >= 1 && k <= kMaxK && action_dim >= 1 && n_actions >= 1 && q_stride >= 1,
                "rlx_wolpertinger_select: bad sizes (envs=%d, k=%d <= %d, action_dim=%d, actions=%lld, q_stride=%lld)",
                n_env, k, kMaxK, action_dim, n_actions, q_stride);
    RLX_REQUIRE(ld_t >= action_dim && ld_env >= action_dim, "rlx_wolpertinger_select: leading dimension < action_dim (%d)",
                action_dim);
    RLX_LAUNCH((wolpertinger_select_kernel), rlx::grid_for(n_env, kThreads), kThreads, 0, rlx::as_stream(stream), q,
               q_stride, idx, n_env, k, target_actions, ld_t, n_actions, action_dim, action_out, env_action_out, ld_env);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_discrete_to_box(const int *actions, int batch, const float *target_actions, long long ld_t, long long n_actions,
                        int action_dim, float *out, long long ld_out, int *status, void *stream) {
    RLX_REQUIRE(actions && target_actions && out && status, "rlx_discrete_to_box: null pointer");
    RLX_REQUIRE(batch >= 1 && action_dim >= 1 && n_actions >= 1, "rlx_discrete_to_box: bad sizes (batch=%d, action_dim=%d, "
                "actions=%lld)", batch, action_dim, n_actions);
    RLX_REQUIRE(ld_t >= action_dim && ld_out >= action_dim, "rlx_discrete_to_box: leading dimension < action_dim (%d)",
                action_dim);
    RLX_LAUNCH((discrete_to_box_kernel), rlx::grid_for((long long)batch * action_dim, kThreads), kThreads, 0,
               rlx::as_stream(stream), actions, batch, target_actions, ld_t, n_actions, action_dim, out, ld_out, status);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
