// Episode.update_discounted_rewards (core_types.py:771-801) for one transition of an episode, shared by
// rlx_episode_nstep_returns (returns.hip) and rlx_pg_episode_window (policy_gradient.hip).
//
// The reference adds current_discount * rewards[i:] for i = 1 .. n-1 onto a float64 copy of the rewards,
// current_discount growing by repeated multiplication: out[t] = ((r[t] + g1 r[t+1]) + g2 r[t+2]) + ...  with
// g_j = g_{j-1} * discount — the same order and the same products here, so the value is bit-identical to the reference's
// n_step_discounted_rewards.  Needs -ffp-contract=off (no fused multiply-add) in the file that includes it.
#pragma once

namespace rlx {

// rewards[row(k)] is the reward of step k of the episode (0 <= k < T); n = the number of steps summed (T for n_step -1).
template <typename Row>
__device__ __forceinline__ double episode_nstep_return(const float *__restrict__ rewards, int t, int T, int n,
                                                       double discount, Row row) {
    double acc = (double)rewards[row(t)];
    double g = discount;
    for (int j = 1; j < n; ++j) {
        if (t + j < T) acc += g * (double)rewards[row(t + j)];
        g *= discount;
    }
    return acc;
}

}  // namespace rlx
