"""numpy restatement of the Direct Future Prediction arithmetic of csrc/dfp.hip, operation by operation, so that the
kernels can be compared with it bit for bit; tests/test_dfp_ref.py pins it to the reference agent's recorded values
(tests/golden/dfp.npz, written by tests/golden/make_golden_dfp.py).

  future_measurements(meas, S, scale, last_step)   DFPAgent._update_measurements_targets (agents/dfp_agent.py:235-255)
  merge(E, X)                                      the MeasurementsPredictionHead's stream merge (csrc/dfp_merge.hpp)
  head_loss(E, X, actions, future, grad_scale)     learn_from_batch's targets + the head's loss and the gradients of the two
                                                   stream outputs, fp32 in the kernel's order
  total_loss64(E, X, actions, future)              the same loss in fp64 (for central differences)
  scores(E, X, goal, weights, S, M)                choose_action's fp64 action values (dfp_agent.py:175-186)
  egreedy(q, explore_u, random_actions, tie, eps)  EGreedy.get_action on fp64 values (the distributional agents' restatement)
  accumulated_reward_measurements(rewards)         use_accumulated_reward_as_measurement with the reference's one-step lag
"""
import numpy as np

from c51_ref import egreedy  # noqa: F401  (the same choice rlx_categorical_egreedy makes)

F32, F64 = np.float32, np.float64

# The cases tests/golden/dfp.npz records (tests/golden/make_golden_dfp.py reads them from here)
LENGTHS, STEPS, MEAS = (1, 2, 3, 5, 33, 40), (1, 3, 6), (1, 2)                 # episode lengths T, steps S, measurements M
SCALES = {"one": (1.0, 1.0), "half3": (0.5, 3.0)}                              # scale factors (the first M of them)
LEARN_CASES = ((1, 2, 1, 1), (5, 3, 6, 1), (64, 2, 6, 1), (7, 18, 3, 2))       # (B, A, S, M)
ACT_CASES = tuple((A, M, W) for A in (2, 6) for M in (1, 2) for W in (1, 3))   # with S = ACT_STEPS
ACT_ROWS, ACT_STEPS = 20, 6
GOALS = {1: [1.0], 2: [1.0, 0.7]}
WEIGHTS = {1: [1.0], 3: [0.5, 0.5, 1.0]}


def future_measurements(meas, S, scale, last_step=False):
    """meas: fp64 [T, M], the STATE's measurements of one episode -> fp32 [T, S, M].  off = i + 2^s; past the end: NaN, or
    (last_step) the LAST transition's state.  The difference and the product are fp64, rounded to fp32 once."""
    meas = np.asarray(meas, F64)
    T, M = meas.shape
    scale = np.asarray(scale, F64)
    out = np.empty((T, S, M), F32)
    for i in range(T):
        for s in range(S):
            off = i + 2 ** s
            if off >= T:
                if not last_step:
                    out[i, s] = np.nan
                    continue
                off = T - 1
            out[i, s] = (scale * (meas[off] - meas[i])).astype(F32)
    return out


def accumulated_reward_measurements(rewards):
    """rewards: one episode's shaped rewards r_1 .. r_T (fp32, as the replay holds them) -> fp64 [T + 1]: the measurement
    of the states s_0 .. s_T.  agent.py:920-925 injects total_shaped_reward_in_current_episode into the NEXT state before
    observe_transition (:958) adds the step's reward: s_t carries r_1 + ... + r_{t-1}, so s_0 and s_1 both carry 0.
    Entry t < T is transition t's STATE measurement."""
    out = np.zeros(len(rewards) + 1, F64)
    acc = F64(0.0)
    for t, r in enumerate(rewards):
        out[t + 1] = acc                 # injected first ...
        acc = acc + F64(F32(r))          # ... then the step's reward is added
    return out


def merge(E, X, dtype=F32):
    """E [B, K], X [B, A, K] -> y [B, A, K]: s = 0, then plus X[:, a] for a = 0 .. A-1 in this order; mean = s / A;
    y = E + (X - mean).  rlx_dueling_combine's order (for K = 1 the same bits)."""
    E, X = np.asarray(E, dtype), np.asarray(X, dtype)
    B, A, K = X.shape
    s = np.zeros((B, K), dtype)
    for a in range(A):
        s = s + X[:, a]
    mean = s / dtype(A)
    return E[:, None, :] + (X - mean[:, None, :])


def head_loss(E, X, actions, future, grad_scale=1.0, dtype=F32):
    """Everything rlx_dfp_head_loss computes, fp32 in its order -> dict(y, targets, loss, dE [B, K], dX [B, A, K], status).
    future: [B, K] (any float type; rounded to fp32 as the replay column holds it), may hold NaN.
    dtype=np.float64 evaluates the same expressions in fp64 from the fp32 inputs."""
    E, X, future = np.asarray(E, dtype), np.asarray(X, dtype), np.asarray(future).astype(F32).astype(dtype)
    B, A, K = X.shape
    future = future.reshape(B, K)
    y = merge(E, X, dtype)
    targets = y.copy()
    dE, dX = np.zeros((B, K), dtype), np.zeros((B, A, K), dtype)
    gs2, inv, status = dtype(grad_scale) * dtype(2.0), dtype(1.0) / dtype(A), 0
    total = dtype(0.0)
    for b in range(B):
        act = int(actions[b])
        row = dtype(0.0)
        if not 0 <= act < A:
            status |= 1
        else:
            for k in range(K):
                fm = future[b, k]
                if np.isnan(fm):
                    continue                                  # (the kernel adds 0.f here: the same sum)
                targets[b, act, k] = fm
                d = fm - y[b, act, k]
                row = row + d * d
                g = (gs2 * (y[b, act, k] - fm)) / dtype(B)
                dE[b, k] = g
                for a in range(A):
                    dX[b, a, k] = g * (dtype(1.0 if a == act else 0.0) - inv)
        total = total + row
    return dict(y=y, targets=targets, loss=dtype(total / dtype(B)), dE=dE, dX=dX, status=status)


def total_loss64(E, X, actions, future):
    """the head's loss, sum over (a, k) of the batch mean of (targets_nonan - y)^2, in fp64."""
    y = merge(np.asarray(E, F64), np.asarray(X, F64), F64)
    B = y.shape[0]
    taken = y[np.arange(B), np.asarray(actions)]
    fm = np.asarray(future, F64).reshape(taken.shape)
    d = np.where(np.isnan(fm), 0.0, fm - taken)
    return (d * d).sum() / B


def scores(E, X, goal, weights, S, M):
    """-> fp64 [n, A]: v[a] = sum_{j < W} (sum_{m < M} (double)y[a][(S - W + j)*M + m] * goal[m]) * weights[j], both sums
    from 0.0 in index order."""
    y = merge(E, X)
    n, A, K = y.shape
    assert K == S * M
    goal, weights = np.asarray(goal, F64), np.asarray(weights, F64)
    W = len(weights)
    v = np.zeros((n, A), F64)
    for j in range(W):
        f = np.zeros((n, A), F64)
        for m in range(M):
            f = f + y[:, :, (S - W + j) * M + m].astype(F64) * goal[m]
        v = v + f * weights[j]
    return v
