"""csrc/dnd.hip through its entry points and through QDND (memories/non_episodic/differentiable_neural_dictionary.py).
The lookup against a numpy fp32 restatement of the house distance and the (distance, index) order: indices equal,
element for element — the kernel performs the same fp32 operations in the same order per pair, and minima of integers
are exact.  The head against an fp64 torch restatement with autograd; the writes against a numpy restatement of the
contract in include/rlx.h."""
import numpy as np
import pytest

from tolerances import LOSS, OUT

C = 2048                                                                      # RLX_KNN_KEY_CHUNK


def dist2(q, keys):
    """[Q, W], [n, W] -> fp32 [Q, n]: acc = 0; for w ascending t = q[w] - key[w], acc = acc + t * t, each step rounded"""
    acc = np.zeros((len(q), len(keys)), dtype=np.float32)
    for w in range(q.shape[1]):
        t = q[:, w:w + 1] - keys[None, :, w]
        acc = acc + t * t
    return acc


def nearest(d2, k):
    """ascending (distance bits, index): the k smallest words of each row"""
    words = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(d2.shape[1], dtype=np.uint64)
    return np.sort(words, axis=1)[:, :k]


def _padded(x, ld, dev):
    import torch
    buf = torch.full(x.shape[:-1] + (ld,), float("nan"), dtype=torch.float32, device=dev)
    buf[..., :x.shape[-1]] = torch.from_numpy(x).to(dev)
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize("own", [False, True], ids=["all_tables", "own_table"])
@pytest.mark.parametrize("W,n,k,Q,integer", [
    (16, 2, 1, 1, False), (48, 2047, 50, 16, False), (512, C, 64, 17, False), (16, C + 1, 50, 17, True),
    (48, 51, 50, 17, True), (16, 32 * C + 1, 64, 1, False),                   # 33 chunks at k = 64: a second merge pass
])
def test_lookup(rlx, dev, W, n, k, Q, integer, own):
    import ctypes
    import torch
    rng = np.random.RandomState(W + n + k + Q)
    A, sizes = 3, [n, k, max(k + 1, n - max(1, n // 3))]                      # table 1 has k keys: no list
    draw = (lambda *s: rng.randint(-3, 4, size=s).astype(np.float32)) if integer else \
        (lambda *s: rng.randn(*s).astype(np.float32))
    keys, q = draw(A, n, W), draw(Q, W)
    q[0] = keys[0, n - 1]                                                     # a query that IS a key
    actions = ((np.arange(Q) + 1) % (A + 1) - 1 if own else np.full(Q, -1)).astype(np.int32)    # 0, 1, 2, then -1 of its
    #                                                                                              own: no table
    L = 1 if own else A
    dkeys = _padded(keys, W + 4, dev)
    for a in range(A):
        dkeys[a, sizes[a]:] = float("nan")                                    # rows past the size are never read
    idx = torch.full((Q, L, k), -7, dtype=torch.int32, device=dev)
    d2 = torch.full((Q, L, k), -7.0, dtype=torch.float32, device=dev)
    flags = torch.full((Q, L), -7, dtype=torch.int32, device=dev)
    nbytes = ctypes.c_longlong(-1)
    rlx.dnd_lookup_scratch_bytes(Q, L, n, k, ctypes.byref(nbytes))
    scratch = torch.zeros(max(1, nbytes.value // 8), dtype=torch.int64, device=dev)
    rlx.dnd_lookup(_padded(q, W + 8, dev), W + 8, Q, W, dkeys, W + 4, n, torch.tensor(sizes, dtype=torch.int32, device=dev),
                   A, n, torch.from_numpy(actions).to(dev) if own else None, L, k, k + 1, idx, d2, flags, scratch,
                   nbytes.value, 0)
    torch.cuda.synchronize()
    idx, d2, flags = idx.cpu().numpy(), d2.cpu().numpy(), flags.cpu().numpy()
    for qi in range(Q):
        for l in range(L):
            a = int(actions[qi]) if own else l
            if a < 0 or sizes[a] <= k:
                assert flags[qi, l] == 1 and (idx[qi, l] == -7).all() and (d2[qi, l] == -7.0).all()
                continue
            want = nearest(dist2(q[qi:qi + 1], keys[a, :sizes[a]]), k)[0]
            assert flags[qi, l] == 0
            assert np.array_equal(idx[qi, l], (want & np.uint64(0xffffffff)).astype(np.int32))
            assert np.array_equal(d2[qi, l].view(np.uint32), (want >> np.uint64(32)).astype(np.uint32))
            if integer:                                                       # every fp32 step exact: the fp64 answer, ties included
                d64 = ((q[qi].astype(np.float64) - keys[a, :sizes[a]].astype(np.float64)) ** 2).sum(1)
                order = np.lexsort((np.arange(sizes[a]), d64))[:k]
                assert np.array_equal(idx[qi, l], order) and np.array_equal(d2[qi, l].astype(np.float64), d64[order])


def _dnd(dev, cap, W, A, k, **kw):
    from coach_amd.memories.non_episodic.differentiable_neural_dictionary import QDND
    return QDND(cap, W, A, num_neighbors=k, device=dev, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("k", [1, 50])
@pytest.mark.parametrize("W", [16, 512])
def test_head_forward_backward(dev, B, k, W):
    import torch
    rng = np.random.RandomState(B + k + W)
    A, cap, delta = 3, 128, 0.001
    sizes = [cap, 100, k]                                                     # table 2: at most k entries, Q = 0
    dnd = _dnd(dev, cap, W, A, k, l2_norm_added_delta=delta)
    keys, values = rng.randn(A, cap, W).astype(np.float32), rng.randn(A, cap).astype(np.float32)
    stamps = rng.randint(0, 1000, size=(A, cap)).astype(np.int64)
    e = rng.randn(B, W).astype(np.float32)
    e[0] = keys[0, 5]                                                         # d = delta exactly
    dnd.keys.copy_(torch.from_numpy(keys)); dnd.values.copy_(torch.from_numpy(values))
    dnd.stamps.copy_(torch.from_numpy(stamps)); dnd.size.copy_(torch.tensor(sizes)); dnd.clock.fill_(990)
    dnd.max_keys = cap
    de = torch.from_numpy(e).to(dev)

    def restate(actions):
        """fp64 Q [B, lists] with autograd, the stamps and the clock after the call"""
        e64 = torch.from_numpy(e).double().requires_grad_(True)
        rows, clock = [], int(dnd.clock.item())
        for b in range(B):
            row = []
            for a in (range(A) if actions is None else [int(actions[b])]):
                if sizes[a] <= k:
                    row.append(e64.new_zeros(()))
                    continue
                j = (nearest(dist2(e[b:b + 1], keys[a, :sizes[a]]), k)[0] & np.uint64(0xffffffff)).astype(np.int64)
                d = ((torch.from_numpy(keys[a, j]).double() - e64[b]) ** 2).sum(1) + float(np.float32(delta))
                w = 1.0 / d
                row.append((torch.from_numpy(values[a, j]).double() * (w / w.sum())).sum())
                stamps[a, j] = np.maximum(stamps[a, j], clock + b)
            rows.append(torch.stack(row))
        return e64, torch.stack(rows), clock + B

    _, want, clock = restate(None)                                            # the acting pass: all tables
    got = dnd.query(de).cpu().numpy()
    np.testing.assert_allclose(got, want.detach().numpy(), **OUT)
    assert (got[:, 2] == 0).all() and int(dnd.clock.item()) == clock
    assert np.array_equal(dnd.stamps.cpu().numpy(), stamps)

    actions = (np.arange(B) % A).astype(np.int32)                             # the training pass: the taken action's table
    targets = rng.randn(B).astype(np.float32)
    e64, want, clock = restate(actions)
    flagged = torch.from_numpy(np.array([sizes[a] <= k for a in actions]))
    loss = ((want[:, 0] - torch.from_numpy(targets).double()) ** 2).sum() / B      # a flagged row counts with its Q = 0
    loss.backward()
    dact, dtargets = torch.from_numpy(actions).to(dev), torch.from_numpy(targets).to(dev)
    q, saved = dnd.train_query(de, dact)
    grad, scalars = dnd.loss_backward(de, dact, q, saved, dtargets)
    np.testing.assert_allclose(q.cpu().numpy(), want.detach().numpy(), **OUT)
    np.testing.assert_allclose(scalars.cpu().numpy()[0], loss.item(), **LOSS)
    np.testing.assert_allclose(grad.cpu().numpy(), e64.grad.numpy(), **OUT)
    assert (grad.cpu().numpy()[flagged.numpy()] == 0).all()
    assert int(dnd.clock.item()) == clock and np.array_equal(dnd.stamps.cpu().numpy(), stamps)


def _state(dnd):
    return [t.cpu().numpy().copy() for t in (dnd.keys, dnd.values, dnd.stamps, dnd.size)] + [int(dnd.clock.item())]


def restate_add(state, e, actions, returns, threshold, shift):
    """rlx_dnd_add's contract (include/rlx.h) on a copy of the tables"""
    keys, values, stamps, size, clock = state
    cap = keys.shape[1]
    for a in range(keys.shape[0]):
        n0, new = int(size[a]), []
        old = keys[a, :n0].copy()
        for t in np.flatnonzero(actions == a):
            j = None
            if n0:
                word = nearest(dist2(e[t:t + 1], old), 1)[0, 0]
                d2 = np.array([word >> np.uint64(32)], dtype=np.uint32).view(np.float32)[0]
                j = int(word & np.uint64(0xffffffff)) if np.sqrt(d2) <= np.float32(threshold) else None
            if j is None:
                new.append(t)
            else:
                values[a, j] = values[a, j] + np.float32(shift) * (returns[t] - values[a, j])
                stamps[a, j] = clock
        room = min(len(new), cap - n0)
        oldest = np.lexsort((np.arange(n0), stamps[a, :n0]))[:len(new) - room]
        for t, s in zip(new, list(range(n0, n0 + room)) + sorted(oldest.tolist())):
            keys[a, s], values[a, s], stamps[a, s] = e[t], returns[t], clock
        size[a] = n0 + room
    return keys, values, stamps, size, clock + 1


# (entries of tables 0 / 1 before the call, [(action, "new" or the stored entry it lies next to, return), ...])
ADD_CASES = {
    "room": ((3, 2), [(0, "new", 1.0), (1, "new", 2.0), (0, "new", 3.0), (1, "new", 4.0)]),
    "fills_exactly": ((5, 2), [(0, "new", 1.0), (0, "new", 2.0), (0, "new", 3.0)]),
    "evicts_the_oldest": ((8, 8), [(0, "new", 1.0), (1, "new", 2.0), (0, "new", 3.0), (0, "new", 4.0)]),
    "within_threshold": ((5, 2), [(0, 2, 7.0), (0, "new", 1.0)]),
    "two_keys_one_entry": ((8, 3), [(0, 1, 1.0), (0, "new", 2.0), (0, 1, 5.0), (1, "new", 3.0), (0, "new", 4.0)]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(ADD_CASES))
def test_add(dev, case):
    import torch
    rng = np.random.RandomState(len(case))
    cap, W, A, threshold, shift = 8, 16, 2, 0.25, 0.5
    dnd = _dnd(dev, cap, W, A, 2, key_error_threshold=threshold, new_value_shift_coefficient=shift)
    filled, rows = ADD_CASES[case]
    put = lambda e, a, r: dnd.add(torch.from_numpy(e).to(dev), torch.tensor(a, dtype=torch.int32, device=dev),
                                  torch.tensor(r, dtype=torch.float32, device=dev))
    for a in range(A):
        put(3 * rng.randn(filled[a], W).astype(np.float32), [a] * filled[a], rng.randn(filled[a]).tolist())
    stored = dnd.keys.cpu().numpy()
    if min(filled) > 2:                      # lookups stamp what they read: the entries near these queries are the youngest
        dnd.query(torch.from_numpy(stored[0, [1, 6]] + np.float32(0.01)).to(dev))
    state = _state(dnd)
    e = np.stack([3 * rng.randn(W).astype(np.float32) if near == "new" else stored[a, near] + np.float32(0.01 * (i + 1))
                  for i, (a, near, _) in enumerate(rows)])
    actions, returns = np.array([r[0] for r in rows], dtype=np.int32), np.array([r[2] for r in rows], dtype=np.float32)
    put(e, actions.tolist(), returns.tolist())
    want, got = restate_add(state, e, actions, returns, threshold, shift), _state(dnd)
    assert np.array_equal(got[3], want[3]) and got[4] == want[4] and int(dnd.status.item()) == 0
    for a in range(A):                       # the table as a set of (key, value, stamp) rows
        table = lambda s: sorted((s[0][a, i].tolist(), float(s[1][a, i]), int(s[2][a, i])) for i in range(int(s[3][a])))
        assert table(got) == table(want)
    with pytest.raises(ValueError, match="exceed dict_size"):
        put(rng.randn(cap + 1, W).astype(np.float32), [0] * (cap + 1), [0.0] * (cap + 1))
    with pytest.raises(ValueError, match="int32"):                            # an int64 action tensor is not misread
        dnd.add(torch.from_numpy(e).to(dev), torch.from_numpy(actions.astype(np.int64)).to(dev),
                torch.from_numpy(returns).to(dev))
    put(e[:1], [A], [0.0])                                                    # an action that names no table
    with pytest.raises(ValueError, match="status 1"):
        dnd.check_status()
    assert np.array_equal(_state(dnd)[3], want[3])


@pytest.mark.gpu
@pytest.mark.parametrize("W,k,name", [(24, 5, "width"), (520, 5, "width"), (16, 65, "k"), (16, 0, "k")])
def test_lookup_refuses_by_name(rlx, dev, W, k, name):
    import torch
    from coach_amd._rlx import RlxError
    z = torch.zeros(4096, dtype=torch.float32, device=dev)
    i = torch.zeros(4096, dtype=torch.int32, device=dev)
    with pytest.raises(RlxError, match="rlx_dnd_lookup: " + name):
        rlx.dnd_lookup(z, W, 1, W, z, W, 4, i, 1, 4, None, 1, k, max(k, 1), i, None, i, None, 0, 0)


@pytest.mark.parametrize("kw,error,name", [
    (dict(propagate_updates_to_DND=True), NotImplementedError, "propagate_updates_to_DND"),
    (dict(key_width=40), ValueError, "key_width"), (dict(num_neighbors=65), ValueError, "num_neighbors"),
    (dict(dict_size=(1 << 22) + 1), ValueError, "dict_size"),
])
def test_qdnd_refuses_by_name(kw, error, name):
    from coach_amd.memories.non_episodic.differentiable_neural_dictionary import QDND
    args = dict(dict_size=8, key_width=16, num_actions=2)
    args.update(kw)
    with pytest.raises(error, match=name):
        QDND(**args)
