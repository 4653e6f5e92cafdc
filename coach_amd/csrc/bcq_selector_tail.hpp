// The row tail of DDQN-BCQ's masked selectors (agents/ddqn_bcq_agent.py:126-131), shared by rlx_bcq_masked_selector
// (bcq.hip: the nearest-neighbour mask) and rlx_bcq_imitation_selector (imitation.hip: the imitation model's mask): one
// definition, so a row that keeps no action gets the same draws from either launch on the same (seed, rank, event).
// tests/bcq_ref.py (uniforms) is the restatement.
#pragma once
#include "philox.hpp"
#include "rlx_common.hpp"

namespace rlx {

constexpr int kBcqSelectorMaxBatch = 1024;      // one workgroup, one row per thread
constexpr int kBcqSelectorMaxActions = 18;

// A zero-confidence row b (its maximum is -inf: every action masked, or its own Q values -inf already) takes
// s[k] = u(b, k) instead: the top 24 bits of word 0 of Philox4x32-10 under the key (seed, rank) at the counter
// (event low word, event high word, b, k), times 2^-24 — [0, 1), exact in fp32.  event is read from device memory.
__device__ __forceinline__ void bcq_zero_row_draws(float *s, int b, int A, uint32_t seed, uint32_t rank,
                                                   const long long *event) {
    const unsigned long long ev = (unsigned long long)event[0];
    for (int k = 0; k < A; ++k) {
        const U4 r = philox4x32_10((uint32_t)ev, (uint32_t)(ev >> 32), (uint32_t)b, (uint32_t)k, seed, rank);
        s[k] = (float)(r.x >> 8) * 5.9604644775390625e-8f;
    }
}

// The number of zero-confidence rows of the workgroup into zero_rows[0] (optional).  Called by EVERY thread of the one
// workgroup with its row's flag (0 beyond the batch); zero_rows is uniform, so the barriers are taken by all or none.
// red: kBcqSelectorMaxBatch ints of LDS.
__device__ __forceinline__ void bcq_zero_row_count(int zero, int *zero_rows, int *red) {
    if (!zero_rows) return;
    const int b = threadIdx.x;
    red[b] = zero;
    __syncthreads();
    for (int d = blockDim.x >> 1; d > 0; d >>= 1) {
        if (b < d) red[b] += red[b + d];
        __syncthreads();
    }
    if (b == 0) zero_rows[0] = red[0];
}

// The workgroup of a selector launch: the smallest power of two >= batch, at least one wave.
inline int bcq_selector_threads(int batch) {
    int threads = 64;
    while (threads < batch) threads <<= 1;
    return threads;
}

}  // namespace rlx
