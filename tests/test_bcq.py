"""csrc/bcq.hip on the GPU: rlx_nn_min_distance and rlx_bcq_masked_selector against the numpy restatement
(tests/bcq_ref.py), bit for bit.  That is derived, not measured: the kernel performs the same fp32 operations in the same
order per (query, key) pair, the minimum over keys is exact in any order, and the square root is correctly rounded."""
import os

import numpy as np
import pytest

import bcq_ref as R
from test_bcq_ref import CASES, case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 128                                                                   # RLX_NN_KEY_CHUNK: keys of one workgroup


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "bcq.npz"))


def _t(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _padded(x, ld, dev, offset=0):
    """[n, w] -> a device view [n, ld] (NaN beyond the row's w floats) that starts `offset` floats into its buffer"""
    import torch
    n, w = x.shape
    buf = np.full(offset + max(n, 1) * ld, np.nan, dtype=np.float32)
    view = buf[offset:offset + n * ld].reshape(n, ld)
    view[:, :w] = x
    return torch.from_numpy(buf).to(dev)[offset:]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _distances(rlx, dev, q, keys, offsets, ld_q=None, ld_k=None, ld_out=None, offset=0, times=1):
    import torch
    (n, w), S = q.shape, len(offsets) - 1
    ld_q, ld_k, ld_out = ld_q or w, ld_k or w, ld_out or S
    out = torch.full((n, ld_out), float("nan"), dtype=torch.float32, device=dev)
    qd, kd = _padded(q, ld_q, dev, offset), _padded(keys, ld_k, dev, offset)
    od = _t(np.asarray(offsets, dtype=np.int32), dev)
    for _ in range(times):
        rlx.nn_min_distance(qd, ld_q, n, w, kd, ld_k, len(keys), od, S, out, ld_out, 0)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[:, S:]).all()                                        # nothing written past the row's sets
    return np.ascontiguousarray(got[:, :S])


def _random(n, w, counts, seed, hits=True):
    rng = np.random.RandomState(seed)
    keys = rng.randn(sum(counts), w).astype(np.float32)
    q = rng.randn(n, w).astype(np.float32)
    if hits and len(keys):
        q[::3] = keys[rng.randint(len(keys), size=len(q[::3]))]             # every third query IS a key
    return q, keys, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_distances_on_the_recorded_shapes(rlx, dev, gold, name):
    c = case(gold, name)
    got = _distances(rlx, dev, c["emb_next"], c["keys"], c["set_offsets"])
    assert np.array_equal(bits(got), bits(c["familiarity"]))
    # the dataset against its own key sets (average_dist's pass): every transition finds itself at distance 0
    got = _distances(rlx, dev, c["emb"], c["keys"], c["set_offsets"])
    assert np.array_equal(bits(got), bits(R.nn_min_distance(c["emb"], c["keys"], c["set_offsets"])))
    assert (got[np.arange(len(got)), c["data_actions"]] == 0).all()
    avg = R.average_dist(got)
    assert avg == float(c["average_dist"]) or (np.isinf(avg) and np.isinf(float(c["average_dist"])))


@pytest.mark.parametrize("n,w", [(1, 1), (33, 64), (257, 512)])
@pytest.mark.parametrize("count", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_distances_around_the_key_chunk_size(rlx, dev, n, w, count):
    q, keys, off = _random(n, w, [count, 5, count], seed=n + count)
    want = R.nn_min_distance(q, keys, off)
    got = _distances(rlx, dev, q, keys, off)
    assert np.array_equal(bits(got), bits(want))
    assert (want == 0).any() and not np.signbit(got).any()


@pytest.mark.parametrize("ld_q,ld_k,ld_out,offset", [(40, 36, 5, 0), (35, 39, 3, 0), (33, 33, 4, 1), (36, 36, 3, 4)])
def test_distances_with_padded_leading_dimensions_and_unaligned_bases(rlx, dev, ld_q, ld_k, ld_out, offset):
    q, keys, off = _random(37, 33, [CHUNK + 3, 0, 9], seed=ld_q)
    got = _distances(rlx, dev, q, keys, off, ld_q, ld_k, ld_out, offset)
    assert np.array_equal(bits(got), bits(R.nn_min_distance(q, keys, off)))


def test_a_query_equal_to_a_key_gives_zero_an_empty_set_inf_and_a_second_call_the_same(rlx, dev):
    q, keys, off = _random(9, 100, [0, 300, 0, 1], seed=4, hits=False)
    keys = keys * np.float32(1000)
    q[:] = keys[[0, 150, 299, 300, 7, 8, 9, 10, 11]]
    q[3:5] += np.float32(0.5)
    want = R.nn_min_distance(q, keys, off)
    got = _distances(rlx, dev, q, keys, off)
    twice = _distances(rlx, dev, q, keys, off, times=2)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got), bits(twice))
    assert np.isinf(got[:, [0, 2]]).all() and (got[:, [0, 2]] > 0).all()
    assert got[[0, 1, 2, 5, 6, 7, 8], 1].tolist() == [0.0] * 7 and got[3, 1] > 0 and np.isfinite(got[:, [1, 3]]).all()
    # no keys at all: every set is empty
    none = _distances(rlx, dev, q, keys[:0], [0, 0, 0])
    assert np.isposinf(none).all()


def test_distances_at_the_largest_set_count_and_a_bad_offset_table(rlx, dev):
    counts = [3, 0, 130, 1, 7, 0, 0, 64, 2, 5, 9, 1, 1, 40, 0, 6, 8, 200]
    q, keys, off = _random(65, 20, counts, seed=18)
    got = _distances(rlx, dev, q, keys, off)
    assert got.shape == (65, 18) and np.array_equal(bits(got), bits(R.nn_min_distance(q, keys, off)))
    # offsets beyond the keys are clamped to them: the launch reads nothing past the matrix
    bad = off.copy()
    bad[-1] += 1000
    assert np.array_equal(bits(_distances(rlx, dev, q, keys, bad)), bits(got))


def test_distance_refusals(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    z = torch.zeros(64 * 520, dtype=torch.float32, device=dev)
    off = torch.zeros(32, dtype=torch.int32, device=dev)
    out = torch.zeros(64 * 32, dtype=torch.float32, device=dev)
    call = lambda q=z, ld_q=512, n=4, w=512, k=z, ld_k=512, n_keys=8, o=off, S=18, d=out, ld_out=18: \
        rlx.nn_min_distance(q, ld_q, n, w, k, ld_k, n_keys, o, S, d, ld_out, 0)
    call()
    for kw in (dict(w=513, ld_q=513, ld_k=513), dict(S=19, ld_out=19), dict(ld_q=511), dict(ld_k=511), dict(w=0),
               dict(S=0), dict(n=0), dict(ld_out=17), dict(q=None), dict(o=None), dict(d=None), dict(k=None),
               dict(n_keys=-1)):
        with pytest.raises(RlxError, match="rlx_nn_min_distance"):
            call(**kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the selector
def _selector(rlx, dev, q, fam, threshold, seed, rank, event, ld=None, count=True):
    import torch
    B, A = q.shape
    ld = ld or A
    sel = torch.full((B, ld), float("nan"), dtype=torch.float32, device=dev)
    zero = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ev = torch.tensor([event], dtype=torch.int64, device=dev)
    rlx.bcq_masked_selector(_padded(q, ld, dev), ld, _padded(fam, ld, dev), ld, float(threshold), B, A, seed, rank, ev,
                            sel, ld, zero if count else None, 0)
    torch.cuda.synchronize()
    got = sel.cpu().numpy()
    assert np.isnan(got[:, A:]).all()
    return np.ascontiguousarray(got[:, :A]), int(zero.item())


@pytest.mark.parametrize("name", sorted(CASES))
def test_selector_equals_the_restatement_and_the_reference_agent(rlx, dev, gold, name):
    c = case(gold, name)
    B, A = c["q_sel"].shape
    args = (c["q_sel"], c["familiarity"], float(c["threshold"]))
    want, mask, zero = R.masked_selector(*args, seed=3, rank=1, event=5)
    got, n_zero = _selector(rlx, dev, *args, 3, 1, 5, ld=A + 3)
    assert np.array_equal(bits(got), bits(want)) and n_zero == int(zero.sum()) == CASES[name][4]
    assert np.array_equal(np.isneginf(got) | zero[:, None], c["mask"]) and np.array_equal(zero, c["zero_rows"])
    live = ~zero
    assert np.array_equal(np.argmax(got, axis=1)[live], c["selected"][live])
    # the same event gives the same draws, another event (low or high word), seed or rank gives others
    again, _ = _selector(rlx, dev, *args, 3, 1, 5, count=False)
    assert np.array_equal(bits(again), bits(got))
    if zero.any():
        for seed, rank, event in ((3, 1, 6), (3, 1, 5 + (1 << 32)), (4, 1, 5), (3, 2, 5)):
            other, _ = _selector(rlx, dev, *args, seed, rank, event)
            assert np.array_equal(bits(other), bits(R.masked_selector(*args, seed=seed, rank=rank, event=event)[0]))
            assert np.array_equal(bits(other[live]), bits(got[live])) and not (other[zero] == got[zero]).any()
    # -inf passes through the existing head-loss launch to the reference agent's targets
    import torch
    td = torch.full((B, A), float("nan"), dtype=torch.float32, device=dev)
    dq = torch.zeros(B, A, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rlx.dqn_head_loss(_t(c["q_online"], dev), A, _t(c["q_next"], dev), _t(got, dev), A,
                      _t(c["actions"].astype(np.int32), dev), _t(c["rewards"], dev), _t(c["go"].astype(np.uint8), dev),
                      None, float(c["discount"]), B, A, 0, 1.0, dq, A, None, td, A, None, status, 0)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert np.array_equal(bits(td.cpu().numpy()[live]), bits(c["targets"][live]))
    chosen = np.argmax(got, axis=1)
    want_td = R.td_targets(c["q_online"], c["q_next"], chosen, c["actions"], c["rewards"], c["go"], float(c["discount"]))
    assert np.array_equal(bits(td.cpu().numpy()), bits(want_td))            # the zero-confidence rows too, by the device draws


def test_selector_at_the_largest_batch_with_every_row_masked(rlx, dev):
    rng = np.random.RandomState(2)
    B, A = 1024, 18
    q = rng.randn(B, A).astype(np.float32)
    fam = np.full((B, A), np.inf, dtype=np.float32)
    fam[::2, 4] = 0.25                                                       # every other row keeps one action
    want, mask, zero = R.masked_selector(q, fam, 0.5, seed=9, rank=0, event=(7 << 32) + 1)
    got, n_zero = _selector(rlx, dev, q, fam, 0.5, 9, 0, (7 << 32) + 1)
    assert np.array_equal(bits(got), bits(want)) and n_zero == 512 and ((got[zero] >= 0) & (got[zero] < 1)).all()
    assert (np.argmax(got[~zero], axis=1) == 4).all()
    # a threshold of +inf masks nothing, not even an empty set's +inf
    got, n_zero = _selector(rlx, dev, q, fam, np.inf, 9, 0, 0)
    assert np.array_equal(bits(got), bits(q)) and n_zero == 0


def test_selector_refusals(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    z = torch.zeros(2048 * 20, dtype=torch.float32, device=dev)
    out = torch.zeros(2048 * 20, dtype=torch.float32, device=dev)
    ev = torch.zeros(1, dtype=torch.int64, device=dev)
    call = lambda q=z, ld_q=4, f=z, ld_f=4, B=8, A=4, e=ev, s=out, ld_s=4: rlx.bcq_masked_selector(
        q, ld_q, f, ld_f, 1.0, B, A, 0, 0, e, s, ld_s, None, 0)
    call()
    for kw in (dict(B=1025), dict(B=0), dict(A=19, ld_q=19, ld_f=19, ld_s=19), dict(A=0), dict(ld_q=3), dict(ld_f=3),
               dict(ld_s=3), dict(q=None), dict(f=None), dict(e=None), dict(s=None)):
        with pytest.raises(RlxError, match="rlx_bcq_masked_selector"):
            call(**kw)
    torch.cuda.synchronize()


def test_reward_model_targets_equal_the_reference(rlx, dev, gold):
    import torch
    from coach_amd._rlx import RlxError
    pred, actions, rewards = gold["rm_prediction"], gold["rm_actions"].astype(np.int32), gold["rm_rewards"]
    B, A = pred.shape
    out = torch.full((B, A + 2), float("nan"), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rlx.reward_model_targets(_padded(pred, A + 1, dev), A + 1, _t(actions, dev), _t(rewards, dev), B, A, out, A + 2,
                             status, 0)
    got = out.cpu().numpy()
    assert int(status.item()) == 0 and np.isnan(got[:, A:]).all()
    assert np.array_equal(bits(got[:, :A]), bits(gold["rm_targets"]))
    # in place, and an action out of range is flagged and leaves its row the prediction
    bad = actions.copy()
    bad[2], bad[5] = A, -1
    buf = _t(pred, dev)
    rlx.reward_model_targets(buf, A, _t(bad, dev), _t(rewards, dev), B, A, buf, A, status, 0)
    got = buf.cpu().numpy()
    ok = np.ones(B, bool)
    ok[[2, 5]] = False
    assert int(status.item()) == 1 and np.array_equal(got[~ok], pred[~ok])
    assert np.array_equal(bits(got[ok]), bits(gold["rm_targets"][ok]))
    with pytest.raises(RlxError, match="rlx_reward_model_targets"):
        rlx.reward_model_targets(buf, A - 1, _t(bad, dev), _t(rewards, dev), B, A, buf, A, status, 0)
