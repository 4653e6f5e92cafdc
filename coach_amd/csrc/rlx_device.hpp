// Device primitives shared by the dense- and conv-layer kernels: the layer activations, the MFMA operand types and
// accumulator layout, the global -> LDS request.  One definition each; every kernel of the library that needs one takes
// it from here.
#pragma once
#include "rlx_common.hpp"

namespace rlx {

typedef float f32x4 __attribute__((ext_vector_type(4)));      // v_mfma_f32_16x16x4_f32 / 4x4x1 accumulator, 16-byte access
typedef float f32x16 __attribute__((ext_vector_type(16)));    // v_mfma_f32_32x32x2_f32 accumulator

__device__ __forceinline__ float relu(float v) {
    return v <= 0.f ? 0.f : v;       // np.maximum(v, 0): a NaN stays NaN (v > 0 ? v : 0 made it 0)
}

// kLeaky: RLX_ACT_LEAKY_RELU (slope 0.2) is served too -- dense_small.hip's launches alone; no other kernel's activation
// carries that branch.
template <bool kLeaky = false>
__device__ __forceinline__ float act_apply(float v, int act) {
    if (act == RLX_ACT_RELU) return relu(v);
    if (act == RLX_ACT_TANH) return tanhf(v);
    if (kLeaky && act == RLX_ACT_LEAKY_RELU) return v > 0.f ? v : 0.2f * v;
    return v;
}
// derivative of the activation expressed through its OUTPUT y
template <bool kLeaky = false>
__device__ __forceinline__ float act_deriv_out(float y, int kind) {
    if (kind == RLX_ACT_RELU) return y > 0.f ? 1.f : 0.f;
    if (kind == RLX_ACT_TANH) return 1.f - y * y;
    if (kLeaky && kind == RLX_ACT_LEAKY_RELU) return y > 0.f ? 1.f : 0.2f;
    return 1.f;
}

// row of a 32 x 32 MFMA accumulator tile that element r (0 .. 15) of lane (column = lane % 32, hi = lane / 32) holds
__device__ __forceinline__ int mfma_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// one 16-byte global -> LDS request per lane; lds_dst: wave-uniform LDS byte address of lane 0's 16 bytes
__device__ __forceinline__ void dma16(const float *gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_dst)
                 : "memory");
}

// ---- The two sums of the library.  Losses, gradient norms and batch statistics are pinned to references bit for bit
// (tests/*_ref.py), so the ORDER of their additions is part of the contract: neither atomics (order of arrival) nor a
// running sum, but the two fixed shapes below, one definition each.

// The 64 lanes of a wave: the xor butterfly, distances 32, 16, .. 1.  Every lane ends up with the sum; all 64 lanes
// must call it.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

namespace detail {
__device__ __forceinline__ void tree_store(int) {}
template <typename T, typename... Rest>
__device__ __forceinline__ void tree_store(int t, T *red, T v, Rest... rest) {
    red[t] = v;
    tree_store(t, rest...);
}
__device__ __forceinline__ void tree_add(int, int) {}
template <typename T, typename... Rest>
__device__ __forceinline__ void tree_add(int t, int d, T *red, T, Rest... rest) {
    red[t] += red[t + d];
    tree_add(t, d, rest...);
}
}  // namespace detail

// The workgroup: tree_sum(n, red, v) adds the values v of threads 0 .. n - 1 (n a power of two, at most the workgroup;
// a constant or blockDim.x) through the LDS array red as a halving tree: level d = n/2, n/4, .. 1 adds red[t + d]
// into red[t] for t < d, one barrier per level.  The sum is in red[0], visible to every thread, when it returns; it
// does not depend on the launch, and float or double alike round once per level and pair (tree_sum in tests/*_ref.py
// restates it).  tree_sum(n, red_a, a, red_b, b, ...) takes several sums through the same levels and barriers, each
// exactly the additions of its own tree_sum.  EVERY thread of the workgroup must call it (barriers inside), and every
// thread stores its v: red holds one entry per THREAD of the workgroup, also where n is smaller (no guard on the store:
// every caller's array is that wide, and the store stays what the hand-written copies had).  red is the caller's to
// reuse only after a barrier of its own.
template <typename... RedValuePairs>
__device__ __forceinline__ void tree_sum(int n, RedValuePairs... red_value_pairs) {
    const int t = threadIdx.x;
    detail::tree_store(t, red_value_pairs...);
    __syncthreads();
    for (int d = n >> 1; d > 0; d >>= 1) {
        if (t < d) detail::tree_add(t, d, red_value_pairs...);
        __syncthreads();
    }
}

}  // namespace rlx
