"""csrc/wolpertinger.hip on the GPU against the numpy restatement (tests/wolpertinger_ref.py): every index and every fp32
word equal.  That is derived, not measured: per (query, key) pair the kernel performs the same fp32 operations in the
same order, the k smallest of the (distance bits, index) words are exact in any order, and the other three kernels only
move words."""
import ctypes

import numpy as np
import pytest

import wolpertinger_ref as R

pytestmark = pytest.mark.gpu
C = 2048                                                                      # RLX_KNN_KEY_CHUNK: keys of one workgroup


def _t(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _padded(x, ld, dev, offset=0):
    """[n, w] -> a device view [n, ld] (NaN beyond the row's w floats) that starts `offset` floats into its buffer"""
    import torch
    n, w = x.shape
    buf = np.full(offset + n * ld, np.nan, dtype=np.float32)
    buf[offset:offset + n * ld].reshape(n, ld)[:, :w] = x
    return torch.from_numpy(buf).to(dev)[offset:]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _scratch(rlx, dev, n_queries, n_keys, k):
    import torch
    nbytes = ctypes.c_longlong(-1)
    rlx.knn_topk_scratch_bytes(n_queries, n_keys, k, ctypes.byref(nbytes))
    assert nbytes.value >= 0 and nbytes.value % 8 == 0
    return torch.zeros(max(1, nbytes.value // 8), dtype=torch.int64, device=dev), nbytes.value


def _topk(rlx, dev, q, keys, k, ld_q=None, ld_k=None, offset=0, with_dist=True):
    import torch
    n, w = q.shape
    ld_q, ld_k = ld_q or w, ld_k or w
    idx = torch.full((n * k + 1,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((n * k + 1,), -7.0, dtype=torch.float32, device=dev)
    scratch, nbytes = _scratch(rlx, dev, n, len(keys), k)
    rlx.knn_topk(_padded(q, ld_q, dev, offset), ld_q, n, w, _padded(keys, ld_k, dev, offset), ld_k, len(keys), k, idx,
                 dist if with_dist else None, scratch, nbytes, 0)
    torch.cuda.synchronize()
    i, d = idx.cpu().numpy(), dist.cpu().numpy()
    assert i[-1] == -7 and d[-1] == -7.0                                      # nothing written past the lists
    return i[:-1].reshape(n, k), d[:-1].reshape(n, k)


def _check(rlx, dev, q, keys, k, **kw):
    want_i, want_d = R.knn_topk(q, keys, k)
    got_i, got_d = _topk(rlx, dev, q, keys, k, **kw)
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(bits(got_d), bits(want_d))
    return got_i, got_d


def _random(n_queries, n_keys, w, seed):
    rng = np.random.RandomState(seed)
    keys = rng.randn(n_keys, w).astype(np.float32)
    q = rng.randn(n_queries, w).astype(np.float32)
    q[0] = keys[rng.randint(n_keys)]                                          # a query that IS a key
    return q, keys


@pytest.mark.parametrize("n_keys", [1, 2, 5, C - 1, C, C + 1, 2 * C + 3])
def test_topk_key_counts_around_the_chunk(rlx, dev, n_keys):
    q, keys = _random(3, n_keys, 1, n_keys)
    i, d = _check(rlx, dev, q, keys, min(5, n_keys))
    assert d[0, 0] == 0.0


def test_topk_more_lists_than_one_merge_pass_takes(rlx, dev):
    """k = 64: a merge workgroup takes 2048 / 64 = 32 lists, 34 chunks leave two lists after the first pass"""
    q, keys = _random(2, 33 * C + 5, 1, 11)
    _check(rlx, dev, q, keys, 64)


def test_topk_the_preset_table(rlx, dev):
    """10^6 + 3 keys of width 1, as get_initialized_knn builds them: index arithmetic across 489 chunks"""
    n = 1000003
    keys = R.knn_keys(n, np.array([1.0], dtype=np.float32)).astype(np.float32)
    q = np.array([[0.3337], [-1.2], [float(keys[n - 7, 0])]], dtype=np.float32)
    i, d = _check(rlx, dev, q, keys, 5)
    assert i[1].tolist() == [0, 1, 2, 3, 4] and n - 7 in i[2].tolist() and d[2, 0] == 0.0


@pytest.mark.parametrize("k", [1, 2, 5, 64])
@pytest.mark.parametrize("n_keys", [300, 2 * C + 3])
def test_topk_k(rlx, dev, n_keys, k):
    q, keys = _random(3, n_keys, 3, 100 + k)
    _check(rlx, dev, q, keys, k)


@pytest.mark.parametrize("n_keys", [1, 5, 64])
def test_topk_k_equal_to_the_number_of_keys(rlx, dev, n_keys):
    q, keys = _random(3, n_keys, 2, 200 + n_keys)
    i, _ = _check(rlx, dev, q, keys, n_keys)
    assert sorted(i[1].tolist()) == list(range(n_keys))


@pytest.mark.parametrize("w", [1, 3, 4, 5, 33, 64])
@pytest.mark.parametrize("n_keys", [77, C + 1])
def test_topk_widths(rlx, dev, n_keys, w):
    q, keys = _random(3, n_keys, w, 300 + w)
    _check(rlx, dev, q, keys, 5)


@pytest.mark.parametrize("n_queries", [1, 3, 33])
def test_topk_query_counts(rlx, dev, n_queries):
    q, keys = _random(n_queries, C + 7, 4, 400 + n_queries)
    _check(rlx, dev, q, keys, 3)


@pytest.mark.parametrize("w, ld_q, ld_k, offset", [(1, 1, 1, 1), (1, 2, 3, 0), (4, 4, 4, 1), (4, 5, 6, 0), (8, 8, 8, 3),
                                                   (33, 35, 34, 0), (4, 8, 8, 0)])
def test_topk_leading_dimensions_and_bases_that_forbid_16_byte_loads(rlx, dev, w, ld_q, ld_k, offset):
    q, keys = _random(5, C + 9, w, 500 + w + ld_k)
    _check(rlx, dev, q, keys, 4, ld_q=ld_q, ld_k=ld_k, offset=offset)


def test_topk_without_distances(rlx, dev):
    q, keys = _random(3, 500, 2, 61)
    got_i, d = _topk(rlx, dev, q, keys, 4, with_dist=False)
    assert np.array_equal(got_i, R.knn_topk(q, keys, 4)[0]) and (d == -7.0).all()


def test_topk_ordering_rules(rlx, dev):
    keys = np.zeros((C + 40, 2), dtype=np.float32) + 50.0
    keys[[3, C + 5, 17]] = [1.0, 2.0]                                         # duplicates, across two chunks
    keys[9], keys[C + 9] = [0.0, 2.0], [2.0, 2.0]                             # mirrored around (1, 2)
    keys[C + 1] = [np.inf, 0.0]
    keys[30] = [np.nan, 0.0]
    q = np.array([[1.0, 2.0], [np.nan, 0.0], [1.0, 2.0]], dtype=np.float32)
    i, d = _check(rlx, dev, q, keys, 6)
    assert i[0].tolist()[:5] == [3, 17, C + 5, 9, C + 9] and d[0, :3].tolist() == [0.0, 0.0, 0.0]
    assert i[1].tolist() == [0, 1, 2, 3, 4, 5] and (bits(d[1]) == R.NAN_BITS).all()      # a NaN query: by index
    i, d = _check(rlx, dev, q[:1], keys[:64], 64)                             # every key of one chunk: the NaN at the end
    assert i[0, -1] == 30 and bits(d[0, -1:])[0] == R.NAN_BITS
    _check(rlx, dev, q[:1], keys[:C + 2].copy(), 64)


def test_topk_inf_and_nan_sort_last_on_the_device(rlx, dev):
    keys = np.array([[np.nan], [np.inf], [2.0], [np.nan], [-np.inf], [1.0]], dtype=np.float32)
    i, d = _check(rlx, dev, np.array([[1.5]], dtype=np.float32), keys, 6)
    assert i[0].tolist() == [2, 5, 1, 4, 0, 3]
    assert bits(d[0]).tolist()[2:] == [0x7f800000, 0x7f800000, 0x7fc00000, 0x7fc00000]


def test_topk_refusals(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    q, keys = _t(np.zeros((2, 4), np.float32), dev), _t(np.zeros((70, 4), np.float32), dev)
    idx = torch.zeros(2 * 64, dtype=torch.int32, device=dev)
    scratch = torch.zeros(1 << 16, dtype=torch.int64, device=dev)

    def call(width=4, n_keys=70, k=3, ld_q=4, ld_k=4, sc=scratch, nbytes=8 << 16):
        rlx.knn_topk(q, ld_q, 2, width, keys, ld_k, n_keys, k, idx, None, sc, nbytes, 0)
    call()
    with pytest.raises(RlxError, match="n_keys 2 outside"):
        call(n_keys=2, k=3)
    with pytest.raises(RlxError, match=r"k 65 outside \[1, 64\]"):
        call(k=65)
    with pytest.raises(RlxError, match="k 0 outside"):
        call(k=0)
    with pytest.raises(RlxError, match=r"width 0 outside \[1, 64\]"):
        call(width=0)
    with pytest.raises(RlxError, match="width 65 outside"):
        call(width=65)
    with pytest.raises(RlxError, match="leading dimension < width"):
        call(ld_k=3)
    with pytest.raises(RlxError, match="scratch of"):
        rlx.knn_topk(q, 4, 2, 4, keys, 4, 3 * C, 3, idx, None, None, 0, 0)
    nbytes = ctypes.c_longlong()
    with pytest.raises(RlxError, match="outside"):
        rlx.knn_topk_scratch_bytes(2, 5, 6, ctypes.byref(nbytes))
    rlx.knn_topk_scratch_bytes(2, C, 6, ctypes.byref(nbytes))
    assert nbytes.value == 0                                                  # one chunk: the search writes the result
    rlx.knn_topk_scratch_bytes(2, 33 * C + 5, 64, ctypes.byref(nbytes))
    assert nbytes.value == (34 + 2) * 64 * 2 * 8


# ------------------------------------------------------------------------------ candidates, selection, conversion
def test_candidates_every_output_word(rlx, dev):
    import torch
    rng = np.random.RandomState(3)
    n_env, k, D, W, n = 5, 3, 7, 2, 40
    keys, obs = rng.randn(n, W).astype(np.float32), rng.randn(n_env, D).astype(np.float32)
    idx = rng.randint(0, n, size=(n_env, k)).astype(np.int32)
    idx[1, 2], idx[4, 0] = n, -1                                              # outside the table: a zero key
    ld_o, ld_a = D + 2, W + 1
    co = torch.full((n_env * k, ld_o), -7.0, dtype=torch.float32, device=dev)
    ca = torch.full((n_env * k, ld_a), -7.0, dtype=torch.float32, device=dev)
    rlx.wolpertinger_candidates(_t(idx, dev), _padded(keys, W + 3, dev), W + 3, n, W, _padded(obs, D + 1, dev), D + 1, D,
                                n_env, k, co, ld_o, ca, ld_a, 0)
    torch.cuda.synchronize()
    safe = np.where((idx >= 0) & (idx < n), idx, 0)
    want_o, want_a = R.candidates(safe, keys, obs)
    want_a[[1 * k + 2, 4 * k + 0]] = 0.0
    co, ca = co.cpu().numpy(), ca.cpu().numpy()
    assert np.array_equal(bits(co[:, :D]), bits(want_o)) and (co[:, D:] == -7.0).all()
    assert np.array_equal(bits(ca[:, :W]), bits(want_a)) and (ca[:, W:] == -7.0).all()


def _select(rlx, dev, q, idx, table, stride=1):
    import torch
    n_env, k = idx.shape
    A = table.shape[1]
    qbuf = np.full(n_env * k * stride, np.nan, dtype=np.float32)
    qbuf[::stride] = q.reshape(-1)
    action = torch.full((n_env + 1,), -7, dtype=torch.int32, device=dev)
    env_action = torch.full((n_env, A + 1), -7.0, dtype=torch.float32, device=dev)
    rlx.wolpertinger_select(_t(qbuf, dev), stride, _t(idx, dev), n_env, k, _t(table, dev), A, len(table), A, action,
                            env_action, A + 1, 0)
    torch.cuda.synchronize()
    a, e = action.cpu().numpy(), env_action.cpu().numpy()
    assert a[-1] == -7 and (e[:, A] == -7.0).all()
    return a[:-1], e[:, :A]


@pytest.mark.parametrize("stride", [1, 3])
def test_select_is_np_argmax(rlx, dev, stride):
    rng = np.random.RandomState(5)
    n_env, k, n, A = 9, 5, 30, 2
    table = rng.randn(n, A).astype(np.float32)
    idx = np.stack([rng.permutation(n)[:k] for _ in range(n_env)]).astype(np.int32)
    q = rng.randn(n_env, k).astype(np.float32)
    q[1, [1, 3]] = q[1].max() + 1                                             # equal maxima: the first wins
    q[2, 2] = np.nan                                                          # a NaN counts as the maximum
    q[3, [4, 1]] = np.nan                                                     # ... the first one
    q[4] = -np.inf
    q[5, 0], q[5, 3] = np.inf, np.nan
    q[6, 4] = np.inf
    want_a, want_e = R.select(q, idx, table)
    assert want_a[1] == idx[1, 1] and want_a[2] == idx[2, 2] and want_a[3] == idx[3, 1] and want_a[4] == idx[4, 0]
    assert want_a[5] == idx[5, 3]
    a, e = _select(rlx, dev, q, idx, table, stride)
    assert np.array_equal(a, want_a) and np.array_equal(bits(e), bits(want_e))


def test_select_with_one_candidate(rlx, dev):
    table = np.arange(12, dtype=np.float32).reshape(6, 2)
    idx = np.array([[4], [0], [5]], dtype=np.int32)
    a, e = _select(rlx, dev, np.array([[np.nan], [-np.inf], [1.0]], dtype=np.float32), idx, table)
    assert a.tolist() == [4, 0, 5] and np.array_equal(e, table[[4, 0, 5]])


@pytest.mark.parametrize("A", [1, 3])
def test_discrete_to_box_and_its_status_bit(rlx, dev, A):
    import torch
    rng = np.random.RandomState(8)
    n, B = 33, 70
    table = rng.randn(n, A).astype(np.float32)
    actions = rng.randint(0, n, size=B).astype(np.int32)
    out = torch.full((B, A + 2), -7.0, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rlx.discrete_to_box(_t(actions, dev), B, _padded(table, A + 1, dev), A + 1, n, A, out, A + 2, status, 0)
    want, st = R.discrete_to_box(actions, table)
    got = out.cpu().numpy()
    assert st == 0 and int(status.item()) == 0
    assert np.array_equal(bits(got[:, :A]), bits(want)) and (got[:, A:] == -7.0).all()
    actions[[0, 40, 69]] = [n, -1, 2 ** 31 - 1]
    rlx.discrete_to_box(_t(actions, dev), B, _padded(table, A + 1, dev), A + 1, n, A, out, A + 2, status, 0)
    want, st = R.discrete_to_box(actions, table)
    assert st == 1 and int(status.item()) == 1 and (want[[0, 40, 69]] == 0).all()
    assert np.array_equal(bits(out.cpu().numpy()[:, :A]), bits(want))


# ------------------------------------------------------------------------------------------------- graph capture
def test_acting_launches_replay_in_a_graph(rlx, dev):
    """search + two merge passes, candidates and selection captured once; three replays follow their inputs"""
    import torch
    from coach_amd import _rlx
    from coach_amd.agents.vector_agent import capture
    rng = np.random.RandomState(13)
    n_env, k, D, n = 3, 64, 4, 33 * C + 5
    keys = R.knn_keys(n, np.array([2.0], dtype=np.float32)).astype(np.float32)
    table = R.target_actions(np.array([-2.0], np.float32), np.array([2.0], np.float32), n).astype(np.float32)
    d_keys, d_table = _t(keys, dev), _t(table, dev)
    proto = torch.zeros(n_env, 1, dtype=torch.float32, device=dev)
    obs = torch.zeros(n_env, D, dtype=torch.float32, device=dev)
    q = torch.zeros(n_env * k, dtype=torch.float32, device=dev)
    idx = torch.zeros(n_env, k, dtype=torch.int32, device=dev)
    co = torch.zeros(n_env * k, D, dtype=torch.float32, device=dev)
    ca = torch.zeros(n_env * k, 1, dtype=torch.float32, device=dev)
    action = torch.zeros(n_env, dtype=torch.int32, device=dev)
    env_action = torch.zeros(n_env, 1, dtype=torch.float32, device=dev)
    scratch, nbytes = _scratch(rlx, dev, n_env, n, k)

    def launches():
        s = _rlx.current_stream()
        rlx.knn_topk(proto, 1, n_env, 1, d_keys, 1, n, k, idx, None, scratch, nbytes, s)
        rlx.wolpertinger_candidates(idx, d_keys, 1, n, 1, obs, D, D, n_env, k, co, D, ca, 1, s)
        rlx.wolpertinger_select(q, 1, idx, n_env, k, d_table, 1, n, 1, action, env_action, 1, s)
    launches()
    torch.cuda.synchronize()
    graph = capture(launches)
    for _ in range(3):
        p = rng.uniform(-2.2, 2.2, (n_env, 1)).astype(np.float32)
        o, qv = rng.randn(n_env, D).astype(np.float32), rng.randn(n_env * k).astype(np.float32)
        proto.copy_(_t(p, dev)); obs.copy_(_t(o, dev)); q.copy_(_t(qv, dev))
        scratch.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        want_i, _ = R.knn_topk(p, keys, k)
        want_o, want_a = R.candidates(want_i, keys, o)
        want_act, want_env = R.select(qv, want_i, table)
        assert np.array_equal(idx.cpu().numpy(), want_i)
        assert np.array_equal(bits(co.cpu().numpy()), bits(want_o)) and np.array_equal(bits(ca.cpu().numpy()), bits(want_a))
        assert np.array_equal(action.cpu().numpy(), want_act)
        assert np.array_equal(bits(env_action.cpu().numpy()), bits(want_env))
