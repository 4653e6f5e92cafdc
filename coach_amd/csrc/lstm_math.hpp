// The two gate functions of the LSTM cell (csrc/lstm.hip), one definition each.  The forward recurrence and the
// back-propagation through time both call these, so what the backward pass recomputes (tanh c_t) has the bits the
// forward pass multiplied by.
#pragma once
#include "rlx_common.hpp"

namespace rlx {

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float lstm_tanh(float x) { return tanhf(x); }

}  // namespace rlx
