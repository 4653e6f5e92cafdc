// What the distributional DQN heads (qr_dqn.hip, c51.hip) share on the device: the first-maximum argmax that picks the
// target action, the check of the taken action, the deterministic batch sum of the loss kernels, the epsilon-greedy
// choice of the acting kernels; and on the host the size checks of the loss entry points.  Everything a head does with
// its atoms (means / softmax expectations, targets / projection, the loss itself) stays in its own file.
#pragma once
#include "rlx_common.hpp"

namespace rlx {

constexpr int kDistLossThreads = 256;   // a loss workgroup: one thread per atom (N <= 256); four waves of 64
constexpr int kDistMaxActions = 18;

// np.argmax over fp64 action values: the first maximum.
__device__ __forceinline__ int first_argmax_f64(const double *q, int n_actions) {
    int best = 0;
    double bv = q[0];
    for (int k = 1; k < n_actions; ++k)
        if (q[k] > bv) { bv = q[k]; best = k; }
    return best;
}

// Is the row's taken action one of the head's?  An action out of range raises status bit 0 (thread 0; the row then
// contributes a zero gradient).  Called by every thread of the workgroup.
__device__ __forceinline__ bool taken_action_valid(int act, int n_actions, int t, int *status) {
    const bool valid = act >= 0 && act < n_actions;
    if (t == 0 && !valid) atomicOr(status, 1);
    return valid;
}

// The batch sum of a loss kernel with one workgroup of THREADS threads per row (batch <= THREADS): thread 0 publishes
// its row's partial (row_partial is read in thread 0 only) and draws a ticket; the workgroup that draws the last one
// sums row_partials[0 .. batch) in a fixed tree, so the sum does not depend on the order of arrival.  Returns true in
// every thread of that workgroup, with the sum in red[0], and false in every thread of the others; the ticket is left
// at zero for the next launch.  Every thread of the workgroup must call it (barriers inside); red is THREADS floats of
// LDS and `last` one shared flag.
// This is the only hand-off between workgroups in these kernels: every access to row_partials and ticket is an
// agent-scope atomic, and their orders (and the fence) are part of the protocol, not a style.
template <int THREADS>
__device__ __forceinline__ bool ticketed_batch_sum(float row_partial, int b, int batch, float *row_partials,
                                                   unsigned int *ticket, float *red, bool *last, int t) {
    if (t == 0) {
        __hip_atomic_store(&row_partials[b], row_partial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned int old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        *last = old == (unsigned int)(batch - 1);
        if (*last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!*last) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    red[t] = t < batch ? __hip_atomic_load(&row_partials[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    __syncthreads();
    for (int d = THREADS >> 1; d > 0; d >>= 1) {
        if (t < d) red[t] += red[t + d];
        __syncthreads();
    }
    return true;
}

// The epsilon-greedy choice on fp64 action values of the acting kernels (rlx_quantile_egreedy,
// rlx_categorical_egreedy): EGreedy.get_action, exploration_policies/e_greedy.py:84-101, with numpy's isclose in fp64:
// |q - max| <= 1e-8 + 1e-5 * |max| (:93-94).  Called by ONE lane per env.
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

// Host: the size and leading-dimension checks of a loss entry point `fn` whose head needs at least min_atoms atoms
// (the three leading dimensions are those of the online output, the target output and the gradient).
inline int check_head_loss_shape(const char *fn, int min_atoms, int n_atoms, int n_actions, int batch,
                                 long long ld_online, long long ld_next, long long ld_grad) {
    RLX_REQUIRE(n_atoms >= min_atoms && n_atoms <= kDistLossThreads && n_actions >= 1 && n_actions <= kDistMaxActions &&
                    batch >= 1 && batch <= kDistLossThreads,
                "%s: unsupported sizes (%d <= atoms=%d <= 256, actions=%d <= 18, batch=%d <= 256)", fn, min_atoms,
                n_atoms, n_actions, batch);
    const long long row = (long long)n_atoms * n_actions;
    RLX_REQUIRE(ld_online >= row && ld_next >= row && ld_grad >= row, "%s: leading dimension < A*N", fn);
    return RLX_OK;
}

}  // namespace rlx
