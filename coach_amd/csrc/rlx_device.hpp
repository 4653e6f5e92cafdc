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

}  // namespace rlx
