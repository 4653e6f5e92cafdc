// One workgroup's share of the register-held Adam + tf.global_norm step (adam_step_norm_kernel, optim.hip), in a header so
// that the same arithmetic can run as the block of an Adam launch, as one of a list of blocks (the late launch and the
// stand-alone early launch of rlx_adam_tf1_step_early / _late) and as a RIDER workgroup of another translation unit's
// launch (rlx_conv_dw_multi_adam, conv_dw_multi.hip).  The block is named by a VIRTUAL index vb of a virtual grid of
// `blocks` workgroups: element <-> (vb, thread, iteration) and every addition are those of the one-launch kernel, whose
// blockIdx.x / gridDim.x they replace, so any split of the virtual blocks over launches leaves w, m, v and the partial sums
// bit-identical.  The update's products and sums must not be contracted: a translation unit that is not compiled with
// -ffp-contract=off includes this header under `#pragma clang fp contract(off)`.
#pragma once
#include "rlx_common.hpp"

namespace rlx_adam {

constexpr int kBlock = 256;
constexpr int kNormIt = 4;       // float4 per array and thread held in registers

struct Coef {
    float alpha, omb1, omb2, eps, grad_scale, rate, one_minus_rate;
};

// state[0] = beta1_power, state[1] = beta2_power (see optim.hip)
__device__ __forceinline__ Coef coef(const float b1p, const float b2p, float lr, float beta1, float beta2, float eps,
                                     float grad_scale, float rate, float one_minus_rate) {
    Coef c;
    c.alpha = lr * sqrtf(1.f - b2p) / (1.f - b1p);
    c.omb1 = 1.f - beta1;
    c.omb2 = 1.f - beta2;
    c.eps = eps;
    c.grad_scale = grad_scale;
    c.rate = rate;
    c.one_minus_rate = one_minus_rate;
    return c;
}

// red: kBlock floats of LDS.  The block's sum of squares goes to sumsq_part[vb] BEFORE the first store of the update:
// EXCHANGE — by an agent-scope atomic exchange whose return value thread 0 hands back (the caller's ticket draw is made to
// depend on it: the partial is published without a fence, see adam_step_norm_kernel); otherwise by an agent-scope store that
// is complete, like every other store of the block, when the launch ends.  Every thread of the workgroup calls it; the last
// barrier inside lies in front of thread 0's read of red[0], so a caller may call it again for another block right away.
template <bool MIX, bool EXCHANGE>
__device__ __forceinline__ float block_step(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ m,
                                            float *__restrict__ v, const long long n, const Coef c, float *sumsq_part,
                                            float *__restrict__ target, const int vb, const int blocks, float *red) {
    const long long stride = (long long)blocks * kBlock;
    const long long n4 = n >> 2;
    const long long i0 = (long long)vb * kBlock + threadIdx.x;
    float4 gw[kNormIt], mw[kNormIt], vw[kNormIt], ww[kNormIt], tw[kNormIt];
#pragma unroll
    for (int it = 0; it < kNormIt; ++it) {
        const long long i = i0 + it * stride;
        if (i < n4) {
            gw[it] = reinterpret_cast<const float4 *>(g)[i];
            mw[it] = reinterpret_cast<float4 *>(m)[i];
            vw[it] = reinterpret_cast<float4 *>(v)[i];
            ww[it] = reinterpret_cast<float4 *>(w)[i];
            if (MIX) tw[it] = reinterpret_cast<float4 *>(target)[i];
        }
    }
    const long long it0 = (n4 << 2) + i0;            // the (at most 3) elements behind the last float4: one thread each
    const bool has_tail = it0 < n;
    const float gt = has_tail ? g[it0] : 0.f;
    float ss = 0.f;                                   // the additions of adam_step_kernel<true>, in its order
#pragma unroll
    for (int it = 0; it < kNormIt; ++it)
        if (i0 + it * stride < n4) {
            const float *gp = &gw[it].x;
#pragma unroll
            for (int k = 0; k < 4; ++k) ss += gp[k] * gp[k];
        }
    if (has_tail) ss += gt * gt;
    red[threadIdx.x] = ss;
    __syncthreads();
    for (int d = kBlock >> 1; d > 0; d >>= 1) {
        if (threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
        __syncthreads();
    }
    float old = 0.f;
    if (threadIdx.x == 0) {
        if (EXCHANGE) old = __hip_atomic_exchange(&sumsq_part[vb], red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_store(&sumsq_part[vb], red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int it = 0; it < kNormIt; ++it) {
        const long long i = i0 + it * stride;
        if (i < n4) {
            float *gp = &gw[it].x, *mp = &mw[it].x, *vp = &vw[it].x, *wp = &ww[it].x, *tp = &tw[it].x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float gr = gp[k] * c.grad_scale;
                mp[k] += (gr - mp[k]) * c.omb1;
                vp[k] += (gr * gr - vp[k]) * c.omb2;
                wp[k] -= (mp[k] * c.alpha) / (sqrtf(vp[k]) + c.eps);
                if (MIX) tp[k] = c.rate * wp[k] + c.one_minus_rate * tp[k];
            }
            reinterpret_cast<float4 *>(m)[i] = mw[it];
            reinterpret_cast<float4 *>(v)[i] = vw[it];
            reinterpret_cast<float4 *>(w)[i] = ww[it];
            if (MIX) reinterpret_cast<float4 *>(target)[i] = tw[it];
        }
    }
    if (has_tail) {
        const float gr = gt * c.grad_scale;
        m[it0] += (gr - m[it0]) * c.omb1;
        v[it0] += (gr * gr - v[it0]) * c.omb2;
        w[it0] -= (m[it0] * c.alpha) / (sqrtf(v[it0]) + c.eps);
        if (MIX) target[it0] = c.rate * w[it0] + c.one_minus_rate * target[it0];
    }
    return old;
}

// What a rider (or a workgroup of the stand-alone early launch) needs: the fields of rlx_adam_split_desc the device reads.
struct EarlyDev {
    float *w;
    const float *g;
    float *m, *v;
    long long n;
    float lr, beta1, beta2, eps, grad_scale;
    const float *state;
    float *sumsq_part;
    const int *early;
    int n_early, blocks;
};

// workgroup `r` of `R`: the early virtual blocks r, r + R, ...
__device__ __forceinline__ void early_blocks(const EarlyDev &e, const int r, const int R, float *red) {
    const Coef c = coef(e.state[0], e.state[1], e.lr, e.beta1, e.beta2, e.eps, e.grad_scale, 0.f, 0.f);
    for (int k = r; k < e.n_early; k += R)
        block_step<false, false>(e.w, e.g, e.m, e.v, e.n, c, e.sumsq_part, nullptr, e.early[k], e.blocks, red);
}

// host: a split descriptor checked and turned into what the early workgroups read
inline int early_dev(const rlx_adam_split_desc *d, EarlyDev *e, const char *who) {
    RLX_REQUIRE(d && d->weights && d->grads && d->m && d->v && d->state && d->partials, "%s: null pointer", who);
    RLX_REQUIRE(d->n > 0 && d->blocks >= 1 && (d->n >> 2) <= (long long)d->blocks * kBlock * kNormIt,
                "%s: %lld parameters do not fit %d register-held blocks", who, d->n, d->blocks);
    RLX_REQUIRE(d->n_early >= 0 && d->n_late >= 1 && d->n_early + d->n_late == d->blocks && d->late && (d->early || !d->n_early),
                "%s: the early and late lists must name every one of the %d blocks once (%d + %d), late not empty", who,
                d->blocks, d->n_early, d->n_late);
    RLX_REQUIRE((((uintptr_t)d->weights | (uintptr_t)d->grads | (uintptr_t)d->m | (uintptr_t)d->v) & 15) == 0,
                "%s: buffers must be 16-byte aligned", who);
    e->w = d->weights; e->g = d->grads; e->m = d->m; e->v = d->v; e->n = d->n;
    e->lr = d->learning_rate; e->beta1 = d->beta1; e->beta2 = d->beta2; e->eps = d->epsilon; e->grad_scale = d->grad_scale;
    e->state = d->state; e->sumsq_part = d->partials; e->early = d->early; e->n_early = d->n_early; e->blocks = d->blocks;
    return RLX_OK;
}

}  // namespace rlx_adam
