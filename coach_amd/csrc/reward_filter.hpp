// The reward filters' arithmetic on one reward — RewardRescaleFilter.filter (filters/reward/reward_rescale_filter.py:37-39)
// then RewardClippingFilter.filter (reward_clipping_filter.py:41-49) — shared by rlx_reward_filter (filters.hip) and
// rlx_dataset_ingest (dataset.hip), so that a reward loaded from a file carries the bits the acting path would have
// stored.  fp64, the reference's operation order; both files are compiled with -ffp-contract=off.
// use_hi / use_lo: the clipping filter's truthiness quirk is resolved by the caller (a bound of 0 is not applied).
// The clip is Python's min(reward, high) / max(reward, low): the bound is taken only where the comparison holds, so a
// NaN reward stays NaN (fmin / fmax would return the bound and hide a broken environment behind a legal reward).
#pragma once
#include <hip/hip_runtime.h>

namespace rlx {

__device__ __forceinline__ float reward_filter_value(float in, double rescale, int use_hi, double hi, int use_lo,
                                                     double lo) {
    double r = (double)in * rescale;
    if (use_hi) r = hi < r ? hi : r;
    if (use_lo) r = lo > r ? lo : r;
    return (float)r;
}

}  // namespace rlx
