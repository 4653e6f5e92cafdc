// The stream merge of the Direct Future Prediction head (MeasurementsPredictionHead._build_module,
// architectures/tensorflow_components/heads/measurements_prediction_head.py:39-57), shared by the loss and the acting
// kernels of dfp.hip.
//
// E is the expectation stream's output [K], X the action stream's [A][K] (column a*K + k), K = steps * measurements.
// For every column k, all in fp32:
//   s    = 0.f, then plus X[a][k] for a = 0 .. A-1 in this order
//   mean = s / (float)A                              tf.reduce_mean(axis=1, keepdims=True)
//   y[a][k] = E[k] + (X[a][k] - mean)
// This is rlx_dueling_combine's order (targets.hip: the sum starts at 0.f, not at X[0][k]; the two differ only in the
// sign of a zero sum), so for K = 1 the result equals rlx_dueling_combine's bit for bit.
#pragma once
#include "rlx_common.hpp"

namespace rlx {

// One row.  Thread t of `threads` owns the columns k = t, t + threads, ...; y may be LDS or global.  No barrier inside:
// the caller synchronises before another thread reads y.
__device__ __forceinline__ void dfp_merge_row(const float *__restrict__ E, const float *__restrict__ X, int A, int K,
                                              float *y, int t, int threads) {
#pragma clang fp contract(off)
    for (int k = t; k < K; k += threads) {
        float s = 0.f;
        for (int a = 0; a < A; ++a) s += X[a * K + k];
        const float mean = s / (float)A;
        const float e = E[k];
        for (int a = 0; a < A; ++a) y[a * K + k] = e + (X[a * K + k] - mean);
    }
}

}  // namespace rlx
