// The exact, ordered selection shared by the k-nearest-neighbour searches (wolpertinger.hip: rlx_knn_topk; dnd.hip:
// rlx_dnd_lookup).  One definition of: the 64-bit (distance bits, index) word, the squared distance's four steps, "k
// rounds of the workgroup's minimum", and the merge pass over lists of such words.
//
// Every (query, key) pair becomes ONE word, (bit pattern of acc) << 32 | key index, a NaN's bit pattern replaced by
// 0xffffffff: acc is never negative, so the unsigned order of the words is ascending (distance, index) with NaN behind
// +inf — equal distances go to the lower index, and no word occurs twice.  The k smallest words are the answer; minima
// of integers are exact in any order, so nothing depends on the order in which workgroups run, and there are no atomics.
//
// select_k: every wave's minimum — the thread's own, then six shuffle steps — through four words of LDS, one barrier per
// round; the owner of a round's winner retires that word and only its wave works out a new minimum; thread r keeps round
// r's winner in a register and the k winners are stored together after the last round.
// knn_merge_kernel: one workgroup takes up to kKeyChunk / k consecutive lists (kKeyChunk words, eight per thread) and
// selects their k smallest the same way; the last pass writes idx / dist2 (a NaN distance as the quiet NaN 0x7fc00000)
// instead of a list.
#pragma once
#include "rlx_common.hpp"

namespace rlx {
namespace knn {

constexpr int kThreads = 256;
constexpr int kSlots = 8;                         // words of one thread
constexpr int kKeyChunk = RLX_KNN_KEY_CHUNK;      // keys of one search workgroup = words of one merge workgroup
constexpr int kQueryTile = 16;                    // queries of one search workgroup
constexpr int kMaxK = 64;
static_assert(kKeyChunk == kThreads * kSlots, "eight words per thread");

typedef unsigned long long u64;
constexpr u64 kNone = ~0ull;                      // no word: above every (distance, index) word (index < 2^31 - 1)

__device__ __forceinline__ u64 make_word(float acc, long long key) {
    const unsigned bits = acc != acc ? 0xffffffffu : __float_as_uint(acc);
    return ((u64)bits << 32) | (u64)(unsigned)key;
}

struct TopkOut {
    u64 *lists;                                   // [rows][lists_out][k], or null: the final pass
    long long lists_out;
    int *idx; float *dist2;                       // [rows][k] (dist2 optional)
    const int *skip;                              // [rows] or null: a row whose entry is not 0 gets no idx / dist2
    int k;
};

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

// The k smallest of the workgroup's kThreads * kSlots words, ascending, to list `list` of row `q` (or to idx / dist2).
// Every thread of the workgroup calls it; `red` is 2 x 4 words of LDS.
__device__ __forceinline__ void select_k(u64 (&w)[kSlots], u64 (*red)[4], const TopkOut &o, long long q, long long list) {
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
        } else if (!(o.skip && o.skip[q])) {
            const unsigned hi = (unsigned)(mine >> 32);
            o.idx[(size_t)q * o.k + tid] = (int)(unsigned)mine;
            if (o.dist2) reinterpret_cast<unsigned *>(o.dist2)[(size_t)q * o.k + tid] = hi == 0xffffffffu ? 0x7fc00000u : hi;
        }
    }
    __syncthreads();                 // the next query's first round writes red[0] again
}

struct MergeArgs {
    const u64 *in; long long lists_in;            // [rows][lists_in][k]
    int fan;                                      // lists of one workgroup: fan * k <= kKeyChunk
    TopkOut out;
};

static __global__ void __launch_bounds__(kThreads) knn_merge_kernel(const MergeArgs a) {
    __shared__ u64 red[2][4];
    const int tid = threadIdx.x, q = blockIdx.y;
    if (a.out.skip && a.out.skip[q]) return;      // uniform: a row without a list (its words mean nothing)
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

// lists left after one merge pass over `lists` lists of k words
inline long long merged_lists(long long lists, int k) {
    const int fan = kKeyChunk / k;
    return (lists + fan - 1) / fan;
}

// words of scratch for `rows` rows over `chunks` chunks: the search's lists and the first merge pass's; later passes
// alternate between the two
inline long long scratch_words(long long rows, long long chunks, int k) {
    return chunks > 1 ? (chunks + merged_lists(chunks, k)) * k * rows : 0;
}

// the merge passes after a search that left `chunks` lists per row in buf[0]; `final` carries idx / dist2 / skip / k
inline int run_merges(u64 *const (&buf)[2], long long chunks, long long rows, const TopkOut &final, hipStream_t s) {
    long long lists = chunks;
    for (int pass = 0; lists > 1; ++pass) {
        MergeArgs m;
        m.in = buf[pass & 1]; m.lists_in = lists; m.fan = kKeyChunk / final.k;
        const long long left = merged_lists(lists, final.k);
        m.out = final;
        m.out.lists = left > 1 ? buf[(pass + 1) & 1] : nullptr;
        m.out.lists_out = left;
        RLX_LAUNCH((knn_merge_kernel), dim3((unsigned)left, (unsigned)rows), kThreads, 0, s, m);
        RLX_LAUNCH_CHECK();
        lists = left;
    }
    return RLX_OK;
}

}  // namespace knn
}  // namespace rlx
