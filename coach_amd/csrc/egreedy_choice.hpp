// The epsilon-greedy choice on fp64 action values, shared by the distributional agents' acting kernels
// (rlx_quantile_egreedy, rlx_categorical_egreedy): EGreedy.get_action, exploration_policies/e_greedy.py:84-101, with
// numpy's isclose in fp64: |q - max| <= 1e-8 + 1e-5 * |max| (:93-94).  Called by ONE lane per env.
#pragma once
#include <hip/hip_runtime.h>

namespace rlx {

__device__ __forceinline__ int egreedy_choice_f64(const double *q, int n_actions, double explore_u, int random_action,
                                                  const double *tie_rand, double epsilon) {
    if (explore_u < epsilon) return random_action;         // e_greedy.py:88
    double mx = q[0];
    for (int k = 1; k < n_actions; ++k) mx = fmax(mx, q[k]);
    const double tol = 1e-8 + 1e-5 * fabs(mx);
    int best = 0;
    double bv = -1.0;
    for (int k = 0; k < n_actions; ++k) {
        const double v = fabs(q[k] - mx) <= tol ? tie_rand[k] : 0.0;
        if (v > bv) { bv = v; best = k; }
    }
    return best;
}

}  // namespace rlx
