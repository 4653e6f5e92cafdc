"""csrc/imitation.hip on the GPU: rlx_classification_head_loss and rlx_bcq_imitation_selector against the numpy
restatement (tests/imitation_ref.py), bit for bit on every output.  That is derived, not measured: per row the kernel
performs the restatement's fp32 operations in its order (the file is compiled without fused multiply-add; exp and log go
through fp64 and are rounded once), the batch sum is the stated tree, and the selector's tail is integer arithmetic."""
import numpy as np
import pytest

import bcq_ref
import imitation_ref as R

pytestmark = pytest.mark.gpu
SENT = np.float32(-777.25)                      # what padding columns and untouched outputs hold
ROWS = (1, 63, 64, 65, 1024)
ACTIONS = (1, 2, 3, 18)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _t(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _padded(x, ld, dev):
    buf = np.full((x.shape[0], ld), SENT, dtype=np.float32)
    buf[:, :x.shape[1]] = x
    return _t(buf, dev)


def _out(B, ld, dev):
    import torch
    return torch.full((B, ld), float(SENT), dtype=torch.float32, device=dev)


def _unpad(t, A):
    got = t.cpu().numpy()
    assert (got[:, A:] == SENT).all()                                        # the padding columns come back untouched
    return np.ascontiguousarray(got[:, :A])


def _head_loss(rlx, dev, logits, actions=None, labels=None, grad_scale=1.0, ld=None, optional=True):
    import torch
    B, A = logits.shape
    ld = ld or A
    dz, probs = _out(B, ld, dev), _out(B, ld, dev)
    row_loss = torch.full((B,), float(SENT), dtype=torch.float32, device=dev)
    scalars = torch.full((2,), float(SENT), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rlx.classification_head_loss(_padded(logits, ld, dev), ld,
                                 None if actions is None else _t(np.asarray(actions, dtype=np.int32), dev),
                                 None if labels is None else _padded(np.asarray(labels, dtype=np.float32), ld, dev), ld,
                                 float(grad_scale), B, A, dz, ld, probs if optional else None, ld,
                                 row_loss if optional else None, scalars, status, 0)
    torch.cuda.synchronize()
    if not optional:
        assert (probs.cpu().numpy() == SENT).all() and (row_loss.cpu().numpy() == SENT).all()
    s = scalars.cpu().numpy()
    return dict(dlogits=_unpad(dz, A), probs=_unpad(probs, A) if optional else None, row_loss=row_loss.cpu().numpy(),
                loss_sum=s[0], correct=s[1], status=int(status.item()))


def _same(got, want, optional=True):
    assert np.array_equal(bits(got["dlogits"]), bits(want["dlogits"]))
    if optional:
        assert np.array_equal(bits(got["probs"]), bits(want["probs"]))
        assert np.array_equal(bits(got["row_loss"]), bits(want["row_loss"]))
    assert bits(got["loss_sum"]) == bits(want["loss_sum"])                  # the restated tree, not np.sum
    assert got["correct"] == want["correct"] and got["status"] == want["status"]


def _soft_labels(rng, B, A):
    l = rng.rand(B, A).astype(np.float32)
    l[::4] = 0                                   # rows of zeros, rows that do not sum to one: no sum-of-labels factor
    l[1::4] *= np.float32(3)
    return l


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("B", ROWS)
def test_head_loss_equals_the_restatement(rlx, dev, B, A):
    rng = np.random.RandomState(100 * A + B)
    x = (rng.randn(B, A) * 3).astype(np.float32)
    act = rng.randint(0, A, size=B)
    for ld in (A, A + 3):
        for gs in (1.0, 0.37):
            _same(_head_loss(rlx, dev, x, actions=act, grad_scale=gs, ld=ld), R.classification_head_loss(x, actions=act, grad_scale=gs))
        hot = R.one_hot(act, A).astype(np.float32)
        got = _head_loss(rlx, dev, x, labels=hot, ld=ld)
        _same(got, R.classification_head_loss(x, labels=hot))
        _same(got, R.classification_head_loss(x, actions=act))               # the one-hot row, never formed: the same bits
        soft = _soft_labels(rng, B, A)
        _same(_head_loss(rlx, dev, x, labels=soft, grad_scale=0.37, ld=ld),
              R.classification_head_loss(x, labels=soft, grad_scale=0.37))
    _same(_head_loss(rlx, dev, x, actions=act, optional=False), R.classification_head_loss(x, actions=act), optional=False)


def test_the_batch_sum_is_the_tree_not_numpys_sum(rlx, dev):
    rng = np.random.RandomState(7)
    B, A = 1024, 18
    x = (rng.randn(B, A) * 3).astype(np.float32)
    act = rng.randint(0, A, size=B)
    want = R.classification_head_loss(x, actions=act)
    serial = np.float32(0)
    for v in want["row_loss"]:
        serial = np.float32(serial + v)
    assert bits(want["loss_sum"]) != bits(serial)                            # the order of the additions shows at this size
    got = _head_loss(rlx, dev, x, actions=act)
    assert bits(got["loss_sum"]) == bits(want["loss_sum"]) == bits(R.tree_sum(got["row_loss"]))
    # a sum over the batch, not a mean: about B times a row's loss, and the gradient carries no 1 / B
    assert got["loss_sum"] > 0.5 * B * np.median(want["row_loss"])
    assert np.array_equal(bits(got["dlogits"]), bits(want["probs"] - R.one_hot(act, A).astype(np.float32)))


@pytest.mark.parametrize("spread", [0.0, 1e-3, 80.0, 1e4])
def test_head_loss_over_logit_spreads(rlx, dev, spread):
    rng = np.random.RandomState(3)
    B, A = 65, 3
    x = (rng.rand(B, A) * 0.5).astype(np.float32)
    top = rng.randint(0, A, size=B)
    x[np.arange(B), top] += np.float32(spread)
    x += np.float32(17.0)
    act = rng.randint(0, A, size=B)
    for kw in (dict(actions=act), dict(labels=_soft_labels(rng, B, A))):
        got, want = _head_loss(rlx, dev, x, **kw), R.classification_head_loss(x, **kw)
        _same(got, want)
        for k in ("dlogits", "probs", "row_loss"):
            assert np.isfinite(got[k]).all()
        assert np.isfinite(got["loss_sum"])
    if spread == 1e4:                            # exp(-1e4) is 0 in fp64 already: the other classes' p is exactly 0
        other = np.ones((B, A), bool)
        other[np.arange(B), top] = False
        assert (got["probs"][other] == 0).all() and (got["probs"][~other] == 1).all()
    if spread == 0.0:                            # logits within 0.5 of each other: p in [1 / (1 + 2 e^.5), e^.5 / (e^.5 + 2)]
        assert (got["probs"] > 0.23).all() and (got["probs"] < 0.46).all()


def test_one_action_gives_zero_loss_and_gradient(rlx, dev):
    x = np.linspace(-50, 50, 65, dtype=np.float32).reshape(65, 1)
    for kw in (dict(actions=np.zeros(65, dtype=np.int64)), dict(labels=np.ones((65, 1), dtype=np.float32))):
        got = _head_loss(rlx, dev, x, **kw)
        _same(got, R.classification_head_loss(x, **kw))
        assert (got["dlogits"] == 0).all() and (got["row_loss"] == 0).all() and got["loss_sum"] == 0
        assert (got["probs"] == 1).all() and got["correct"] == 65


@pytest.mark.parametrize("B", [1, 65, 1024])
def test_an_action_out_of_range_in_the_first_and_last_row(rlx, dev, B):
    rng = np.random.RandomState(B)
    A = 3
    x = rng.randn(B, A).astype(np.float32)
    act = rng.randint(0, A, size=B)
    act[0], act[-1] = (A if B > 1 else -1), -1
    got, want = _head_loss(rlx, dev, x, actions=act, ld=A + 3), R.classification_head_loss(x, actions=act)
    _same(got, want)
    assert got["status"] == 1 and (got["dlogits"][[0, -1]] == 0).all() and (got["row_loss"][[0, -1]] == 0).all()
    ok = R.classification_head_loss(x[1:-1], actions=act[1:-1])
    assert got["correct"] == ok["correct"]                                   # the two rows are not counted
    if B > 2:
        assert np.array_equal(bits(got["dlogits"][1:-1]), bits(ok["dlogits"]))


def test_head_loss_refusals(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    z = torch.zeros(1024 * 24, dtype=torch.float32, device=dev)
    out = torch.zeros(1024 * 24, dtype=torch.float32, device=dev)
    act = torch.zeros(1024, dtype=torch.int32, device=dev)
    sc = torch.zeros(2, dtype=torch.float32, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    call = lambda x=z, ld=4, a=act, l=None, ld_l=4, B=8, A=4, d=out, ld_d=4, p=None, ld_p=4, s=sc, status=st: \
        rlx.classification_head_loss(x, ld, a, l, ld_l, 1.0, B, A, d, ld_d, p, ld_p, None, s, status, 0)
    call()
    call(a=None, l=z)
    for kw in (dict(x=None), dict(d=None), dict(s=None), dict(status=None), dict(a=None), dict(l=z), dict(B=0),
               dict(B=1025), dict(A=0), dict(A=19, ld=19, ld_d=19), dict(ld=3), dict(ld_d=3), dict(a=None, l=z, ld_l=3),
               dict(p=out, ld_p=3)):
        with pytest.raises(RlxError, match="rlx_classification_head_loss"):
            call(**kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the selector
def _selector(rlx, dev, q, im, threshold, probs_in, seed, rank, event, ld=None, optional=True):
    import torch
    B, A = q.shape
    ld = ld or A
    sel, fam = _out(B, ld, dev), _out(B, ld, dev)
    zero = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ev = torch.tensor([event], dtype=torch.int64, device=dev)
    rlx.bcq_imitation_selector(_padded(q, ld, dev), ld, _padded(im, ld, dev), ld, float(np.float32(threshold)),
                               R.INPUT_PROBS if probs_in else 0, B, A, seed, rank, ev, sel, ld,
                               fam if optional else None, ld, zero if optional else None, 0)
    torch.cuda.synchronize()
    if not optional:
        assert (fam.cpu().numpy() == SENT).all()
        return _unpad(sel, A), None, None
    return _unpad(sel, A), _unpad(fam, A), int(zero.item())


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("B", ROWS)
def test_selector_equals_the_restatement_in_both_input_modes(rlx, dev, B, A):
    rng = np.random.RandomState(1000 * A + B)
    q = (rng.randn(B, A) * 2).astype(np.float32)
    logits = (rng.randn(B, A) * 2).astype(np.float32)
    thr = 0.35 if A < 18 else 0.05
    logits[::5] = 0                              # uniform rows: every action below 0.35 for A >= 3, kept for A <= 2
    want, fam, mask, zero = R.imitation_selector(q, logits, thr, seed=3, rank=1, event=5)
    for ld in (A, A + 3):
        got, gfam, n_zero = _selector(rlx, dev, q, logits, thr, False, 3, 1, 5, ld=ld)
        assert np.array_equal(bits(gfam), bits(fam)) and np.array_equal(bits(got), bits(want))
        assert n_zero == int(zero.sum()) and np.array_equal(np.isneginf(got) | zero[:, None], mask | zero[:, None])
    if A == 3:
        assert zero[::5].all() and (B == 1 or not mask.all())
    if A == 1:
        assert not mask.any() and np.array_equal(bits(got), bits(q))         # one action: familiarity 1
    # the probabilities mode on the launch's own familiarity: the same bits
    again, fam2, n2 = _selector(rlx, dev, q, gfam, thr, True, 3, 1, 5, ld=A + 3)
    assert np.array_equal(bits(again), bits(got)) and np.array_equal(bits(fam2), bits(gfam)) and n2 == n_zero
    only, _, _ = _selector(rlx, dev, q, logits, thr, False, 3, 1, 5, optional=False)
    assert np.array_equal(bits(only), bits(got))


def test_selector_threshold_is_compared_in_fp32_and_nan_is_kept(rlx, dev):
    thr = np.float32(0.35)
    p = np.array([[thr, 0.65], [np.nextafter(thr, np.float32(0)), 0.65], [np.nan, 0.2], [0.1, 0.2]], dtype=np.float32)
    q = np.arange(8, dtype=np.float32).reshape(4, 2)
    want, fam, mask, zero = R.imitation_selector(q, p, 0.35, probs_in=True, seed=1, rank=0, event=9)
    assert mask.tolist() == [[False, False], [True, False], [False, True], [True, True]]
    assert (p[0, 0].astype(np.float64) < 0.35)                               # an fp64 comparison would mask it
    got, gfam, n_zero = _selector(rlx, dev, q, p, 0.35, True, 1, 0, 9)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(gfam), bits(p)) and n_zero == 1
    assert got[0].tolist() == [0.0, 1.0] and np.isneginf(got[1, 0]) and got[2, 0] == 4.0 and np.isneginf(got[2, 1])


@pytest.mark.parametrize("B,A", [(1, 2), (65, 3), (1024, 18)])
def test_fully_masked_rows_draw_what_the_knn_selector_draws_and_a_graph_follows_the_event(rlx, dev, B, A):
    import torch
    from coach_amd import _rlx
    rng = np.random.RandomState(B)
    q, logits = _t(rng.randn(B, A).astype(np.float32), dev), _t(rng.randn(B, A).astype(np.float32), dev)
    far = torch.full((B, A), float("inf"), dtype=torch.float32, device=dev)
    out_nn, out_knn = _out(B, A, dev), _out(B, A, dev)
    z_nn = torch.zeros(1, dtype=torch.int32, device=dev)
    z_knn = torch.zeros(1, dtype=torch.int32, device=dev)
    event = torch.tensor([5], dtype=torch.int64, device=dev)

    def launch():
        s = _rlx.current_stream()
        rlx.bcq_imitation_selector(q, A, logits, A, 2.0, 0, B, A, 3, 1, event, out_nn, A, None, A, z_nn, s)   # p < 2
        rlx.bcq_masked_selector(q, A, far, A, 0.5, B, A, 3, 1, event, out_knn, A, z_knn, s)                  # inf > 0.5
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for ev in (5, (7 << 32) + 6):
        event.fill_(ev)                          # changed on the device between two replays of the one graph
        g.replay()
        torch.cuda.synchronize()
        a, b = out_nn.cpu().numpy(), out_knn.cpu().numpy()
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(bcq_ref.uniforms(B, A, 3, 1, ev)))
        assert int(z_nn.item()) == int(z_knn.item()) == B
        seen.append(a)
    assert not (seen[0] == seen[1]).all()


def test_selector_refusals(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    z = torch.zeros(2048 * 20, dtype=torch.float32, device=dev)
    out = torch.zeros(2048 * 20, dtype=torch.float32, device=dev)
    ev = torch.zeros(1, dtype=torch.int64, device=dev)
    call = lambda q=z, ld_q=4, i=z, ld_i=4, flags=0, B=8, A=4, e=ev, s=out, ld_s=4, f=None, ld_f=4: \
        rlx.bcq_imitation_selector(q, ld_q, i, ld_i, 0.35, flags, B, A, 0, 0, e, s, ld_s, f, ld_f, None, 0)
    call()
    call(flags=1)
    for kw in (dict(B=1025), dict(B=0), dict(A=19, ld_q=19, ld_i=19, ld_s=19), dict(A=0), dict(ld_q=3), dict(ld_i=3),
               dict(ld_s=3), dict(f=out, ld_f=3), dict(q=None), dict(i=None), dict(e=None), dict(s=None), dict(flags=2)):
        with pytest.raises(RlxError, match="rlx_bcq_imitation_selector"):
            call(**kw)
    torch.cuda.synchronize()
