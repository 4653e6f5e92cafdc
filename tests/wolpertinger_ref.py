"""numpy restatement of the Wolpertinger agent's acting arithmetic and tables (csrc/wolpertinger.hip,
coach_amd/agents/wolpertinger_agent.py, coach_amd/filters/action.py), pinned to the reference's own code by
tests/golden/wolpertinger.npz (tests/test_wolpertinger_ref.py) and used as the bit-exact twin of the kernels
(tests/test_wolpertinger.py).

Reference (paths under rl_coach/): agents/wolpertinger_agent.py:72-128, filters/action/box_discretization.py:57-72,
memories/non_episodic/differentiable_neural_dictionary.py (AnnoyDictionary.query).  Annoy holds its items and takes its
queries as fp32; the search here is exact where Annoy's forest is approximate, and ordered by (squared distance, index).
"""
from itertools import product

import numpy as np

NAN_BITS = np.uint32(0x7fc00000)        # how the kernel reports a NaN distance


def knn_keys(num_actions, max_abs_range):
    """get_initialized_knn's keys (wolpertinger_agent.py:118-122): fp64 [n][len(max_abs_range)]"""
    return np.expand_dims((np.arange(num_actions) / (num_actions - 1) - 0.5) * 2, 1) * max_abs_range


def target_actions(low, high, bins, force_int_bins=False):
    """BoxDiscretization.get_unfiltered_action_space (box_discretization.py:57-70) -> [prod(bins)][len(low)], in the dtype
    numpy gives np.linspace(low[i], high[i], bins[i]): with the fp32 bounds gym gives a box, fp32 (and fp32 arithmetic)
    under numpy 2's promotion rules"""
    low, high = np.atleast_1d(low), np.atleast_1d(high)
    if isinstance(bins, (int, np.integer)):
        bins = np.ones(len(low)).astype(int) * bins
    dims = []
    for i in range(len(low)):
        d = np.linspace(low[i], high[i], bins[i])
        dims.append(d.astype(int) if force_int_bins else d)
    return np.array([list(a) for a in product(*dims)]).reshape(-1, len(low))


def squared_distances(queries, keys):
    """fp32 [n_queries][n_keys]: acc = 0; for w in order: t = q[w] - key[w]; acc = acc + t * t — each operation rounded
    to fp32 on its own (numpy's fp32 array arithmetic does exactly that)."""
    q, k = np.asarray(queries, dtype=np.float32), np.asarray(keys, dtype=np.float32)
    acc = np.zeros((q.shape[0], k.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for w in range(q.shape[1]):
            t = q[:, w:w + 1] - k[None, :, w]
            acc = acc + t * t
    return acc


def order_words(dist2):
    """the 64-bit words (distance bits << 32 | index) whose unsigned order is the result's order: a NaN's bits are
    0xffffffff, behind +inf"""
    bits = dist2.view(np.uint32).astype(np.uint64)
    bits = np.where(np.isnan(dist2), np.uint64(0xffffffff), bits)
    return (bits << np.uint64(32)) | np.arange(dist2.shape[1], dtype=np.uint64)[None, :]


def knn_topk(queries, keys, k):
    """-> (idx int32 [n_queries][k], dist2 fp32 [n_queries][k]) ascending in (squared distance, key index); equal
    distances go to the lower index; NaN distances come last, by index, reported as the quiet NaN 0x7fc00000."""
    d = squared_distances(queries, keys)
    order = np.argsort(order_words(d), axis=1, kind="stable")[:, :k]
    dist = np.take_along_axis(d, order, axis=1)
    bits = dist.view(np.uint32).copy()
    bits[np.isnan(dist)] = NAN_BITS
    return order.astype(np.int32), bits.view(np.float32)


def candidates(idx, keys, observations):
    """the critic's inputs (wolpertinger_agent.py:103-105): (np.tile'd observations [n_env * k][D], keys[idx] [n_env * k][W])"""
    idx = np.asarray(idx)
    n_env, k = idx.shape
    obs = np.repeat(np.asarray(observations, dtype=np.float32), k, axis=0)
    return obs, np.asarray(keys, dtype=np.float32)[idx.reshape(-1)]


def select(q, idx, table):
    """wolpertinger_agent.py:106-107 + the output filter: action[e] = idx[e][np.argmax(q[e])] (the first maximum; a NaN
    counts as the maximum), env_action[e] = table[action[e]]"""
    idx = np.asarray(idx)
    n_env, k = idx.shape
    best = np.argmax(np.asarray(q, dtype=np.float32).reshape(n_env, k), axis=1)
    action = idx[np.arange(n_env), best].astype(np.int32)
    return action, np.asarray(table, dtype=np.float32)[action]


def discrete_to_box(actions, table):
    """learn_from_batch's conversion (wolpertinger_agent.py:79-83) -> (fp32 [B][A], status): an action outside the table
    sets status bit 1 and leaves its row zero"""
    actions, table = np.asarray(actions), np.asarray(table, dtype=np.float32)
    ok = (actions >= 0) & (actions < len(table))
    out = np.zeros((len(actions), table.shape[1]), dtype=np.float32)
    out[ok] = table[actions[ok]]
    return out, int(not ok.all())
