// Neural Episodic Control's differentiable neural dictionary (Pritzel et al. 2017) on gfx950: the exact wide-key
// k-nearest-neighbour lookup over one table per action, the dictionary Q head forward and backward, and the episode-end
// writes with LRU eviction.
//
// Replaces, in the reference (paths under rl_coach/):
//   * AnnoyDictionary.query / QDND.query           memories/non_episodic/differentiable_neural_dictionary.py:105-127, 213-229
//     (an approximate Annoy forest on the host, one query at a time; here exact and ordered)
//   * DNDQHead._q_value                            architectures/tensorflow_components/heads/dnd_q_head.py:67-83
//   * the Q head's loss as NECAgent.learn_from_batch feeds it (agents/nec_agent.py:137-150) and tf.gradients through it
//   * AnnoyDictionary.add with override_existing_keys and a rebuild at the end of every call          :60-102
//
// Storage (device, the caller's): keys [A][cap][ld_k] fp32, values [A][cap] fp32, stamps [A][cap] int64, size [A] int32,
// one int64 clock.
//
// rlx_dnd_lookup.  The squared distance and the (distance bits << 32 | index) selection are rlx_knn_topk's
// (csrc/knn_select.hpp): acc = 0; for w ascending t = q[w] - key[w], acc = acc + t * t, each operation rounded to fp32 on
// its own (-ffp-contract=off).  What is new is how the pairs are formed at widths up to 512 floats.  One workgroup of 256
// threads covers a tile of 16 queries and a chunk of 2048 keys of ONE action (grid: chunks x tiles x A); a workgroup none
// of whose queries asks for its action leaves at once.  A thread OWNS keys: key (sub-chunk s, thread t) for s = 0 .. 7,
// and holds 16 accumulators per key, one per query of the tile — 128 distances in registers when the chunk is done.
// The query tile sits in LDS ([16][W] floats: 32 KB at W = 512, 1 KB at W = 16) and is read as same-address broadcasts.
// Keys arrive in slabs of 256 keys x 16 floats through LDS: each thread fetches four 16-byte pieces (four lanes cover the
// 64 contiguous bytes of one key row's slab), one slab ahead in registers, and the slab is stored with a row stride of 20
// floats, so that the 16-byte reads of thread t at word 20 t + 4 c fall on distinct bank groups (20 t mod 64 takes 16
// values, all multiples of 4).  That transposition through LDS is what lets "thread owns key" coexist with row-major
// keys.  One slab step reads 1 + 16 float4 from LDS for 128 VALU operations (64 subtract-multiply-add triples), and w
// ascends inside every accumulator.  Every key byte is fetched from memory once per query tile.  No matrix instruction:
// fp32 MFMA has no peak advantage over fp32 VALU on this part, and (q - k)^2 summed in order is not bilinear.
// Then, per query of the tile that asked for this action: eight words, select_k.  With more than one chunk the lists go
// to scratch and the merge passes of knn_select.hpp follow; the chunk count comes from the host's bound max_keys, the
// tables' real sizes are read on the device.  1 + ceil(log_{2048 / k}(chunks)) launches, no allocation, no
// synchronisation: capturable.
//
// rlx_dnd_head_forward: one wave per (row, list); the k gathered key rows are read once, 16 bytes per lane and step.
// rlx_dnd_head_loss_backward: one workgroup per row, no atomics.  rlx_dnd_add: one workgroup per action.
#include "knn_select.hpp"
#include "rlx_device.hpp"

namespace {

using namespace rlx::knn;

constexpr int kMaxWidth = 512;
constexpr int kSlabFloats = 16;                   // floats of one key row in a slab
constexpr int kSlabStride4 = kSlabFloats / 4 + 1; // float4 per slab row: 20 floats
constexpr int kSub = kThreads;                    // keys of one slab = one per thread
constexpr int kStampIndexBits = 22;               // rlx_dnd_add's eviction word: stamp << 22 | index

struct DndSearchArgs {
    const float *q; long long ld_q; int n_queries, width;
    const float *keys; long long ld_k, cap;       // table a starts at keys + a * cap * ld_k
    const int *size;                              // [A]
    const int *actions;                           // [n_queries] or null (every query: -1)
    int A, n_lists, min_keys; long long max_keys;
    int *flags;                                   // [n_queries][n_lists]
    TopkOut out;
};

__global__ void __launch_bounds__(kThreads) dnd_search_kernel(const DndSearchArgs a) {
    extern __shared__ float4 Qs[];                // [kQueryTile][width / 4]
    __shared__ float4 slab[kSub * kSlabStride4];
    __shared__ u64 red[2][4];
    const int tid = threadIdx.x, act = blockIdx.z;
    const long long chunk = blockIdx.x, key0 = chunk * kKeyChunk;
    const int q0 = blockIdx.y * kQueryTile;
    const int nq = min(kQueryTile, a.n_queries - q0);
    const int w4 = a.width / 4;
    const bool all = a.n_lists == a.A;           // a list per table (A = 1: the two forms are one)
    const long long n_keys = min((long long)max(a.size[act], 0), a.max_keys);
    const bool enough = n_keys >= a.min_keys;

    // which queries of the tile ask for this table; chunk 0 says which (query, list) pairs get no list
    unsigned mask = 0;
    for (int qi = 0; qi < nq; ++qi) {
        const int aq = a.actions ? a.actions[q0 + qi] : -1;
        const bool match = aq == act || (aq == -1 && all);
        if (match && enough) mask |= 1u << qi;
        if (chunk == 0 && tid == 0) {
            if (all) a.flags[(size_t)(q0 + qi) * a.n_lists + act] = match && enough ? 0 : 1;
            else if (match) a.flags[q0 + qi] = enough ? 0 : 1;
            else if (act == 0 && (aq < 0 || aq >= a.A)) a.flags[q0 + qi] = 1;      // no such table
        }
    }
    if (!mask) return;
    const int slot = all ? act : 0;
    TopkOut out = a.out;
    out.skip = nullptr;                           // only rows that get a list come this far; the merge passes read the flags
    if (key0 >= n_keys) {                         // (only with several chunks) nothing here: lists of "no word"
        for (int qi = 0; qi < nq; ++qi)
            if ((mask >> qi & 1) && tid < a.out.k)
                a.out.lists[(((size_t)(q0 + qi) * a.n_lists + slot) * (size_t)a.out.lists_out + (size_t)chunk) * a.out.k + tid] = kNone;
        return;
    }

    for (int i = tid; i < kQueryTile * w4; i += kThreads) {
        const int qi = i / w4, c = i % w4;
        Qs[i] = qi < nq ? *reinterpret_cast<const float4 *>(a.q + (size_t)(q0 + qi) * a.ld_q + 4 * c)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
    }

    const float *table = a.keys + (size_t)act * (size_t)a.cap * (size_t)a.ld_k;
    const int slabs = a.width / kSlabFloats;
    float dist[kSlots][kQueryTile];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
#pragma unroll
        for (int qi = 0; qi < kQueryTile; ++qi) dist[s][qi] = 0.f;
        const long long sub0 = key0 + (long long)s * kSub;
        if (sub0 >= n_keys) continue;             // uniform
        // piece j of this thread: row (j * 256 + tid) / 4 of the slab, floats 4 * ((j * 256 + tid) % 4) ..
        float4 pre[4];
        auto fetch = [&](int sl) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = j * kThreads + tid;
                const long long key = sub0 + (e >> 2);
                pre[j] = key < n_keys ? *reinterpret_cast<const float4 *>(table + (size_t)key * (size_t)a.ld_k +
                                                                         sl * kSlabFloats + 4 * (e & 3))
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        fetch(0);
        for (int sl = 0; sl < slabs; ++sl) {
            __syncthreads();                      // the last slab's reads are over (first time: the query tile is there)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = j * kThreads + tid;
                slab[(e >> 2) * kSlabStride4 + (e & 3)] = pre[j];
            }
            __syncthreads();
            if (sl + 1 < slabs) fetch(sl + 1);    // in flight under the products below
#pragma unroll
            for (int c = 0; c < kSlabFloats / 4; ++c) {
                const float4 kv = slab[tid * kSlabStride4 + c];
                const float4 *qc = Qs + sl * (kSlabFloats / 4) + c;
#pragma unroll
                for (int qi = 0; qi < kQueryTile; ++qi) dist[s][qi] = dist4(dist[s][qi], qc[qi * w4], kv);
            }
        }
    }

#pragma unroll
    for (int qi = 0; qi < kQueryTile; ++qi) {
        if (!(mask >> qi & 1)) continue;          // uniform over the workgroup: select_k's barriers are taken by all
        u64 w[kSlots];
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const long long key = key0 + (long long)s * kSub + tid;
            w[s] = key < n_keys ? make_word(dist[s][qi], key) : kNone;
        }
        select_k(w, red, out, (long long)(q0 + qi) * a.n_lists + slot, chunk);
    }
}

__global__ void dnd_clock_advance_kernel(long long *clock, long long by) { *clock += by; }

struct DndHeadArgs {
    const float *e; long long ld_e; int rows, width;
    const float *keys; long long ld_k, cap;
    const float *values; unsigned long long *stamps;
    const int *idx, *flags, *actions;             // idx [rows][n_lists][k], flags [rows][n_lists], actions [rows] (n_lists 1)
    int A, n_lists, k; float delta;
    const long long *clock;
    float *q; long long ld_qout;                  // [rows][n_lists]
    float *d, *sumw;                              // [rows][n_lists][k], [rows][n_lists] (optional, together)
};

// table of (row, list) — or -1
__device__ __forceinline__ int dnd_table(const int *actions, int A, int n_lists, int row, int list) {
    if (n_lists == A) return list;
    const int aq = actions[row];
    return aq >= 0 && aq < A ? aq : -1;
}

__global__ void __launch_bounds__(kThreads) dnd_head_forward_kernel(const DndHeadArgs a) {
    const int lane = threadIdx.x & 63;
    const long long pair = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (pair >= (long long)a.rows * a.n_lists) return;                  // uniform over the wave
    const int row = (int)(pair / a.n_lists), list = (int)(pair % a.n_lists);
    const int table = dnd_table(a.actions, a.A, a.n_lists, row, list);
    float *qout = a.q + (size_t)row * a.ld_qout + list;
    if (table < 0 || a.flags[pair]) {                                   // no list: QDND.query's zeros
        if (lane == 0) {
            *qout = 0.f;
            if (a.sumw) a.sumw[pair] = 0.f;
        }
        if (a.d && lane < a.k) a.d[pair * a.k + lane] = 0.f;
        return;
    }
    const float *keys = a.keys + (size_t)table * (size_t)a.cap * (size_t)a.ld_k;
    const float *erow = a.e + (size_t)row * a.ld_e;
    const int w4 = a.width / 4;
    float4 ev[kMaxWidth / 256];
#pragma unroll
    for (int p = 0; p < kMaxWidth / 256; ++p)
        ev[p] = lane + 64 * p < w4 ? *reinterpret_cast<const float4 *>(erow + 4 * (lane + 64 * p)) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int mine = lane < a.k ? (int)min((long long)max(a.idx[pair * a.k + lane], 0), a.cap - 1) : 0;
    float dj = 1.f;
    for (int j = 0; j < a.k; ++j) {
        const float *krow = keys + (size_t)__shfl(mine, j) * (size_t)a.ld_k;
        float part = 0.f;
#pragma unroll
        for (int p = 0; p < kMaxWidth / 256; ++p)
            if (lane + 64 * p < w4) part = dist4(part, *reinterpret_cast<const float4 *>(krow + 4 * (lane + 64 * p)), ev[p]);
        const float sum = rlx::wave_sum(part) + a.delta;
        if (lane == j) dj = sum;
    }
    const bool live = lane < a.k;
    const float wj = live ? 1.f / dj : 0.f;
    const float vj = live ? a.values[(size_t)table * a.cap + mine] : 0.f;
    const float sw = rlx::wave_sum(wj), num = rlx::wave_sum(vj * wj);
    if (lane == 0) {
        *qout = num / sw;
        if (a.sumw) a.sumw[pair] = sw;
    }
    if (live) {
        if (a.d) a.d[pair * a.k + lane] = dj;
        atomicMax(a.stamps + (size_t)table * a.cap + mine, (unsigned long long)(*a.clock + row));   // "later wins"
    }
}

struct DndBwdArgs {
    const float *e; long long ld_e; int rows, width;
    const float *keys; long long ld_k, cap;
    const float *values;
    const int *idx, *flags, *actions;             // idx [rows][k], flags [rows]
    const float *d, *sumw, *q;                    // [rows][k], [rows], [rows] (ld_qin apart)
    long long ld_qin;
    const float *targets;                         // [rows]
    int A, k; float grad_scale;
    float *de; long long ld_de;
    float *loss;                                  // scalars[0] (optional)
};

__global__ void __launch_bounds__(kThreads) dnd_head_loss_backward_kernel(const DndBwdArgs a) {
    __shared__ float coef[kMaxK];
    __shared__ int nbr[kMaxK];
    __shared__ float red[kThreads];
    const int tid = threadIdx.x, row = blockIdx.x, B = a.rows;
    if (row == 0 && a.loss) {                     // (uniform) the Q head's loss: sum_b (Q_b - R_b)^2 / B
        float term = 0.f;
        for (int b = tid; b < B; b += kThreads) { // a flagged row counts with the Q = 0 the forward pass gave it
            const float err = a.q[(size_t)b * a.ld_qin] - a.targets[b];
            term = term + err * err;
        }
        rlx::tree_sum(kThreads, red, term);
        if (tid == 0) a.loss[0] = red[0] / (float)B;
        __syncthreads();
    }
    const int table = dnd_table(a.actions, a.A, 1, row, 0);
    const int w4 = a.width / 4;
    float *de = a.de + (size_t)row * a.ld_de;
    if (table < 0 || a.flags[row]) {
        if (tid < w4) *reinterpret_cast<float4 *>(de + 4 * tid) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float qb = a.q[(size_t)row * a.ld_qin];
    const float g = a.grad_scale * 2.f * (qb - a.targets[row]) / (float)B;
    if (tid < a.k) {
        // dQ/dd_j = -(v_j - Q) / (S d_j^2), dd_j/de = -2 (key_j - e)
        const int j = (int)min((long long)max(a.idx[(size_t)row * a.k + tid], 0), a.cap - 1);
        const float dj = a.d[(size_t)row * a.k + tid];
        nbr[tid] = j;
        coef[tid] = g * 2.f * (a.values[(size_t)table * a.cap + j] - qb) / (a.sumw[row] * dj * dj);
    }
    __syncthreads();
    if (tid >= w4) return;
    const float *keys = a.keys + (size_t)table * (size_t)a.cap * (size_t)a.ld_k;
    const float4 ev = *reinterpret_cast<const float4 *>(a.e + (size_t)row * a.ld_e + 4 * tid);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < a.k; ++j) {               // neighbour order: fixed
        const float4 kv = *reinterpret_cast<const float4 *>(keys + (size_t)nbr[j] * (size_t)a.ld_k + 4 * tid);
        const float c = coef[j];
        acc.x += c * (kv.x - ev.x);
        acc.y += c * (kv.y - ev.y);
        acc.z += c * (kv.z - ev.z);
        acc.w += c * (kv.w - ev.w);
    }
    *reinterpret_cast<float4 *>(de + 4 * tid) = acc;
}

struct DndAddArgs {
    const float *e; long long ld_e; int T, width;
    const int *actions; const float *returns;     // [T]
    const int *nn_idx; const float *nn_dist2; const int *nn_flags;      // [T]: rlx_dnd_lookup, k = 1, the row's own action
    float *keys; long long ld_k, cap;
    float *values; long long *stamps; int *size;
    const long long *clock;
    float threshold, shift;
    int *slot_of, *evicted;                       // scratch: [T], [A][T]
    int *status;
};

// exclusive rank of this thread's `pred` among the workgroup's threads (thread order), and their count
__device__ __forceinline__ int block_rank(bool pred, int *wave_count, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(pred);
    __syncthreads();                              // wave_count is free again
    if (lane == 0) wave_count[wave] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int v = 0; v < kThreads / 64; ++v) {
        if (v < wave) before += wave_count[v];
        total += wave_count[v];
    }
    return before;
}

__global__ void __launch_bounds__(kThreads) dnd_add_kernel(const DndAddArgs a) {
    __shared__ int wave_count[kThreads / 64];
    __shared__ long long red[kThreads];
    const int tid = threadIdx.x, act = blockIdx.x;
    const long long cap = a.cap, clock = *a.clock;
    const int size_old = min((long long)max(a.size[act], 0), cap);
    float *values = a.values + (size_t)act * cap;
    long long *stamps = a.stamps + (size_t)act * cap;
    auto matched = [&](int t) { return !a.nn_flags[t] && sqrtf(a.nn_dist2[t]) <= a.threshold; };
    if (clock >> (62 - kStampIndexBits)) {        // (uniform) an eviction word would overflow: the whole call is dropped
        if (tid == 0) atomicOr(a.status, 2);
        return;
    }
    if (act == 0)                                 // a row that names no table is written nowhere
        for (int t = tid; t < a.T; t += kThreads)
            if (a.actions[t] < 0 || a.actions[t] >= (int)gridDim.x) atomicOr(a.status, 1);

    // 1. keys that are a stored entry: the value shifts in episode order (one thread: the order shows), the entry is stamped
    if (tid == 0) {
        for (int t = 0; t < a.T; ++t)
            if (a.actions[t] == act && matched(t)) {
                const int j = (int)min((long long)max(a.nn_idx[t], 0), cap - 1);
                values[j] += a.shift * (a.returns[t] - values[j]);
                stamps[j] = clock;
            }
    }
    // 2. every other key of this action, ranked in episode order
    int n_new = 0;
    for (int t0 = 0; t0 < a.T; t0 += kThreads) {
        const int t = t0 + tid;
        const bool isnew = t < a.T && a.actions[t] == act && !matched(t);
        int total;
        const int r = n_new + block_rank(isnew, wave_count, total);
        if (isnew) a.slot_of[t] = r;              // its rank for now
        else if (t < a.T && a.actions[t] == act) a.slot_of[t] = -1;
        n_new += total;
    }
    const int room = (int)min((long long)n_new, cap - size_old), m = n_new - room;
    __threadfence_block();
    __syncthreads();                              // step 1's stamps and step 2's ranks are visible to the workgroup

    // 3. a full table: the m smallest (stamp << 22 | index) words among the entries from before the call.  R = the m-th
    // smallest word, bit by bit from the top: R takes a bit when fewer than m words lie below R with that bit set.
    int *evicted = a.evicted + (size_t)act * a.T;
    if (m > 0) {
        u64 R = 0;
        const int top = kStampIndexBits + 64 - __clzll(clock | 1);
        for (int bit = top; bit >= 0; --bit) {
            const u64 trial = R | (1ull << bit);
            long long below = 0;
            for (int i = tid; i < size_old; i += kThreads)
                below += (((u64)stamps[i] << kStampIndexBits) | (u64)i) < trial ? 1 : 0;
            __syncthreads();                      // red is free again
            rlx::tree_sum(kThreads, red, below);
            if (red[0] < m) R = trial;
        }
        // the evicted slots in index order
        int found = 0;
        for (int i0 = 0; i0 < size_old; i0 += kThreads) {
            const int i = i0 + tid;
            const bool out = i < size_old && (((u64)stamps[i] << kStampIndexBits) | (u64)i) <= R;
            int total;
            const int r = found + block_rank(out, wave_count, total);
            if (out) evicted[r] = i;
            found += total;
        }
        __threadfence_block();
        __syncthreads();
    }

    // 4. rank r takes slot size_old + r while there is room, evicted slot r - room afterwards
    for (int t = tid; t < a.T; t += kThreads)
        if (a.actions[t] == act && a.slot_of[t] >= 0) {
            const int r = a.slot_of[t], slot = r < room ? size_old + r : evicted[r - room];
            a.slot_of[t] = slot;
            values[slot] = a.returns[t];
            stamps[slot] = clock;
        }
    __threadfence_block();
    __syncthreads();
    const int w4 = a.width / 4;
    float *keys = a.keys + (size_t)act * (size_t)cap * (size_t)a.ld_k;
    for (long long i = tid; i < (long long)a.T * w4; i += kThreads) {
        const int t = (int)(i / w4), c = (int)(i % w4);
        if (a.actions[t] != act || a.slot_of[t] < 0) continue;
        *reinterpret_cast<float4 *>(keys + (size_t)a.slot_of[t] * (size_t)a.ld_k + 4 * c) =
            *reinterpret_cast<const float4 *>(a.e + (size_t)t * a.ld_e + 4 * c);
    }
    if (tid == 0) a.size[act] = size_old + room;
}

int check_rows(const char *who, const char *what, const void *p, long long ld, int width) {
    RLX_REQUIRE((uintptr_t)p % 16 == 0 && ld >= width && ld % 4 == 0,
                "%s: %s must be 16-byte aligned with a leading dimension >= width (%d) that is a multiple of 4 (got %lld)",
                who, what, width, ld);
    return RLX_OK;
}

int check_lookup_sizes(const char *who, int n_queries, int n_lists, int A, long long max_keys, int width, int k) {
    RLX_REQUIRE(width >= 16 && width <= kMaxWidth && width % 16 == 0, "%s: width %d is not a multiple of 16 in [16, %d]", who,
                width, kMaxWidth);
    RLX_REQUIRE(k >= 1 && k <= kMaxK, "%s: k %d outside [1, %d]", who, k, kMaxK);
    RLX_REQUIRE(A >= 1 && A <= 65535 && (n_lists == 1 || n_lists == A), "%s: n_lists %d is neither 1 nor A = %d (A in [1, 65535])",
                who, n_lists, A);
    RLX_REQUIRE(n_queries >= 1 && (long long)n_queries * n_lists <= 65535, "%s: n_queries * n_lists = %lld outside [1, 65535]",
                who, (long long)n_queries * n_lists);
    RLX_REQUIRE(max_keys >= 1 && max_keys <= 0x7fffffffLL, "%s: max_keys %lld outside [1, 2^31 - 1]", who, max_keys);
    return RLX_OK;
}

}  // namespace

extern "C" {

int rlx_dnd_lookup_scratch_bytes(int n_queries, int n_lists, long long max_keys, int k, long long *bytes_out) {
    RLX_REQUIRE(bytes_out, "rlx_dnd_lookup_scratch_bytes: null pointer");
    if (int rc = check_lookup_sizes("rlx_dnd_lookup_scratch_bytes", n_queries, n_lists, n_lists, max_keys, 16, k)) return rc;
    const long long chunks = (max_keys + kKeyChunk - 1) / kKeyChunk;
    *bytes_out = scratch_words((long long)n_queries * n_lists, chunks, k) * (long long)sizeof(u64);
    return RLX_OK;
}

int rlx_dnd_lookup(const float *queries, long long ld_q, int n_queries, int width, const float *keys, long long ld_k,
                   long long cap, const int *size, int A, long long max_keys, const int *actions, int n_lists, int k,
                   int min_keys, int *idx_out, float *dist2_out, int *flags_out, void *scratch, long long scratch_bytes,
                   void *stream) {
    RLX_REQUIRE(queries && keys && size && idx_out && flags_out, "rlx_dnd_lookup: null pointer");
    if (int rc = check_lookup_sizes("rlx_dnd_lookup", n_queries, n_lists, A, max_keys, width, k)) return rc;
    RLX_REQUIRE(max_keys <= cap, "rlx_dnd_lookup: max_keys %lld above cap %lld", max_keys, cap);
    RLX_REQUIRE(min_keys >= k, "rlx_dnd_lookup: min_keys %d below k = %d", min_keys, k);
    RLX_REQUIRE(actions || n_lists == A, "rlx_dnd_lookup: n_lists = 1 needs the queries' actions");
    if (int rc = check_rows("rlx_dnd_lookup", "queries", queries, ld_q, width)) return rc;
    if (int rc = check_rows("rlx_dnd_lookup", "keys", keys, ld_k, width)) return rc;
    long long need = 0;
    if (int rc = rlx_dnd_lookup_scratch_bytes(n_queries, n_lists, max_keys, k, &need)) return rc;
    RLX_REQUIRE(need == 0 || (scratch && scratch_bytes >= need && (uintptr_t)scratch % 8 == 0),
                "rlx_dnd_lookup: scratch of %lld bytes (8-byte aligned) needed, %lld given", need, scratch_bytes);
    hipStream_t s = rlx::as_stream(stream);
    const long long chunks = (max_keys + kKeyChunk - 1) / kKeyChunk, rows = (long long)n_queries * n_lists;
    const int tiles = (n_queries + kQueryTile - 1) / kQueryTile;
    u64 *const buf[2] = {static_cast<u64 *>(scratch), static_cast<u64 *>(scratch) + chunks * k * rows};

    DndSearchArgs a;
    a.q = queries; a.ld_q = ld_q; a.n_queries = n_queries; a.width = width;
    a.keys = keys; a.ld_k = ld_k; a.cap = cap; a.size = size; a.actions = actions;
    a.A = A; a.n_lists = n_lists; a.min_keys = min_keys; a.max_keys = max_keys; a.flags = flags_out;
    a.out.k = k; a.out.idx = idx_out; a.out.dist2 = dist2_out; a.out.skip = flags_out;
    a.out.lists = chunks > 1 ? buf[0] : nullptr;
    a.out.lists_out = chunks;
    RLX_LAUNCH((dnd_search_kernel), dim3((unsigned)chunks, (unsigned)tiles, (unsigned)A), kThreads,
               (unsigned)(kQueryTile * width * sizeof(float)), s, a);
    RLX_LAUNCH_CHECK();
    return run_merges(buf, chunks, rows, a.out, s);
}

int rlx_dnd_head_forward(const float *embedding, long long ld_e, int rows, int width, const float *keys, long long ld_k,
                         long long cap, const float *values, long long *stamps, int A, const int *idx, const int *flags,
                         const int *actions, int n_lists, int k, float l2_norm_added_delta, long long *clock, float *q_out,
                         long long ld_q, float *d_out, float *sumw_out, void *stream) {
    RLX_REQUIRE(embedding && keys && values && stamps && idx && flags && clock && q_out, "rlx_dnd_head_forward: null pointer");
    if (int rc = check_lookup_sizes("rlx_dnd_head_forward", rows, n_lists, A, cap, width, k)) return rc;
    RLX_REQUIRE(actions || n_lists == A, "rlx_dnd_head_forward: n_lists = 1 needs the rows' actions");
    RLX_REQUIRE(!d_out == !sumw_out, "rlx_dnd_head_forward: d_out and sumw_out go together");
    RLX_REQUIRE(ld_q >= n_lists, "rlx_dnd_head_forward: ld_q %lld below n_lists %d", ld_q, n_lists);
    if (int rc = check_rows("rlx_dnd_head_forward", "embedding", embedding, ld_e, width)) return rc;
    if (int rc = check_rows("rlx_dnd_head_forward", "keys", keys, ld_k, width)) return rc;
    hipStream_t s = rlx::as_stream(stream);
    DndHeadArgs a;
    a.e = embedding; a.ld_e = ld_e; a.rows = rows; a.width = width; a.keys = keys; a.ld_k = ld_k; a.cap = cap;
    a.values = values; a.stamps = reinterpret_cast<unsigned long long *>(stamps); a.idx = idx; a.flags = flags;
    a.actions = actions; a.A = A; a.n_lists = n_lists; a.k = k; a.delta = l2_norm_added_delta;
    a.clock = clock; a.q = q_out; a.ld_qout = ld_q; a.d = d_out; a.sumw = sumw_out;
    const long long pairs = (long long)rows * n_lists;
    RLX_LAUNCH((dnd_head_forward_kernel), dim3((unsigned)((pairs + 3) / 4)), kThreads, 0, s, a);
    RLX_LAUNCH_CHECK();
    RLX_LAUNCH((dnd_clock_advance_kernel), 1, 1, 0, s, clock, (long long)rows);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_dnd_head_loss_backward(const float *embedding, long long ld_e, int rows, int width, const float *keys,
                               long long ld_k, long long cap, const float *values, int A, const int *idx, const int *flags,
                               const int *actions, int k, const float *d, const float *sumw, const float *q, long long ld_q,
                               const float *targets, float grad_scale, float *de_out, long long ld_de, float *scalars,
                               void *stream) {
    RLX_REQUIRE(embedding && keys && values && idx && flags && actions && d && sumw && q && targets && de_out,
                "rlx_dnd_head_loss_backward: null pointer");
    if (int rc = check_lookup_sizes("rlx_dnd_head_loss_backward", rows, 1, A, cap, width, k)) return rc;
    RLX_REQUIRE(ld_q >= 1, "rlx_dnd_head_loss_backward: ld_q %lld below 1", ld_q);
    if (int rc = check_rows("rlx_dnd_head_loss_backward", "embedding", embedding, ld_e, width)) return rc;
    if (int rc = check_rows("rlx_dnd_head_loss_backward", "keys", keys, ld_k, width)) return rc;
    if (int rc = check_rows("rlx_dnd_head_loss_backward", "de_out", de_out, ld_de, width)) return rc;
    DndBwdArgs a;
    a.e = embedding; a.ld_e = ld_e; a.rows = rows; a.width = width; a.keys = keys; a.ld_k = ld_k; a.cap = cap;
    a.values = values; a.idx = idx; a.flags = flags; a.actions = actions; a.d = d; a.sumw = sumw; a.q = q; a.ld_qin = ld_q;
    a.targets = targets; a.A = A; a.k = k; a.grad_scale = grad_scale; a.de = de_out; a.ld_de = ld_de; a.loss = scalars;
    RLX_LAUNCH((dnd_head_loss_backward_kernel), dim3((unsigned)rows), kThreads, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_dnd_add(const float *embedding, long long ld_e, int T, int width, const int *actions, const float *returns,
                const int *nn_idx, const float *nn_dist2, const int *nn_flags, float *keys, long long ld_k, long long cap,
                float *values, long long *stamps, int *size, int A, long long *clock, float key_error_threshold,
                float new_value_shift_coefficient, int *slot_scratch, int *status, void *stream) {
    RLX_REQUIRE(embedding && actions && returns && nn_idx && nn_dist2 && nn_flags && keys && values && stamps && size &&
                clock && slot_scratch && status, "rlx_dnd_add: null pointer");
    RLX_REQUIRE(width >= 16 && width <= kMaxWidth && width % 16 == 0, "rlx_dnd_add: width %d is not a multiple of 16 in [16, %d]",
                width, kMaxWidth);
    RLX_REQUIRE(A >= 1 && A <= 65535, "rlx_dnd_add: A %d outside [1, 65535]", A);
    RLX_REQUIRE(cap >= 1 && cap <= (1LL << kStampIndexBits), "rlx_dnd_add: cap %lld outside [1, 2^%d]", cap, kStampIndexBits);
    RLX_REQUIRE(T >= 1 && T <= cap, "rlx_dnd_add: T %d outside [1, cap = %lld]", T, cap);
    if (int rc = check_rows("rlx_dnd_add", "embedding", embedding, ld_e, width)) return rc;
    if (int rc = check_rows("rlx_dnd_add", "keys", keys, ld_k, width)) return rc;
    hipStream_t s = rlx::as_stream(stream);
    DndAddArgs a;
    a.e = embedding; a.ld_e = ld_e; a.T = T; a.width = width; a.actions = actions; a.returns = returns;
    a.nn_idx = nn_idx; a.nn_dist2 = nn_dist2; a.nn_flags = nn_flags; a.keys = keys; a.ld_k = ld_k; a.cap = cap;
    a.values = values; a.stamps = stamps; a.size = size; a.clock = clock; a.threshold = key_error_threshold;
    a.shift = new_value_shift_coefficient; a.slot_of = slot_scratch; a.evicted = slot_scratch + T; a.status = status;
    RLX_LAUNCH((dnd_add_kernel), dim3((unsigned)A), kThreads, 0, s, a);
    RLX_LAUNCH_CHECK();
    RLX_LAUNCH((dnd_clock_advance_kernel), 1, 1, 0, s, clock, 1LL);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
