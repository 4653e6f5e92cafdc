// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the counter-based generator
// behind the synthetic environments (synth_env.hip) and the agents' device noise (noise.hip).  A pure function of
// (counter, key): the numpy restatements (oracle/synth_env.py, tests/noise_ref.py) produce the same words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rlx {

struct U4 {
    uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                            uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}

// Counter word 3 of the noise generators is the draw's high word ^ this tag (noise.hip's opening comment says why).
constexpr uint32_t kNoiseTag = 0x4E4F4953u;          // "NOIS"

// The 53-bit uniform of two output words: m = hi[31:5] lo[31:6], u = (m + 1) 2^-53 in (0, 1] -- exact in fp64.  The u1 of
// noise.hip's Box-Muller pair and the truncated-normal draw of explore_dist.hip (uniforms() of tests/noise_ref.py).
__device__ __forceinline__ double philox_unit(uint32_t hi, uint32_t lo) {
    const unsigned long long m = ((unsigned long long)(hi >> 5) << 26) | (lo >> 6);
    return (double)(m + 1ull) * 1.1102230246251565e-16;      // 2^-53
}

}  // namespace rlx
