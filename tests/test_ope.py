"""csrc/ope.hip on the GPU: rlx_ope_rows, rlx_ope_reduce and rlx_behaviour_probabilities against the numpy restatement
(tests/ope_ref.py), on the recorded cases of tests/golden/ope.npz and on the edge cases of the kernels.

  * pi against the restatement's fp32 softmax depends on the device's expf.  Measured on these cases: the worst distance
    is PI_ULP_MEASURED units in the last place; the tests assert 4 x that.
  * Everything else is compared with the restatement FED THE DEVICE'S pi read back, so no expf is left in the comparison.
    The per-row columns are then the same fp64 operations in the same order (the file is compiled without FMA
    contraction): equal bit for bit.  The five estimates reorder fp64 sums and compositions: |device - restatement| <=
    (number of rows) * 2^-52 * scale, the worst case of reordering that many terms (ope_ref.bound), derived, not measured.
"""
import os

import numpy as np
import pytest

import ope_ref as R
from test_ope_ref import case, cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PI_ULP_MEASURED = 5
PI_ULP = 4 * PI_ULP_MEASURED
ROW_COLUMNS = ("rho", "v", "q_taken", "ips", "dm", "dr")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "ope.npz"))


def _t(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _padded(x, ld, dev, offset=0):
    """[n, w] fp32 -> a device view (NaN beyond the row's w floats) that starts `offset` floats into its buffer"""
    import torch
    n, w = x.shape
    buf = np.full(offset + n * ld, np.nan, dtype=np.float32)
    buf[offset:offset + n * ld].reshape(n, ld)[:, :w] = x
    return torch.from_numpy(buf).to(dev)[offset:]


def ulps(a, b):
    """distance in units in the last place between non-negative fp32 arrays"""
    a, b = (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    return int(np.abs(a - b).max())


def make(lengths, A, seed, T=0.2, q_offset=1.0, q_scale=0.15, batch_size=32):
    rng = np.random.RandomState(seed)
    n = int(sum(lengths))
    c = dict(lengths=np.array(lengths), n_actions=A, temperature=T, discount=0.99, batch_size=batch_size)
    c["q"] = (rng.randn(n, A) * q_scale + q_offset).astype(np.float32)
    c["reward_model"] = (rng.randn(n, A) * 0.5).astype(np.float32)
    c["actions"] = rng.randint(0, A, size=n)
    c["rewards"] = (rng.randn(n) + 0.25).astype(np.float32)
    mu = (0.2 / A + 0.8 * rng.dirichlet(np.ones(A), size=n)).astype(np.float32)
    mu[::2] = np.float32(1) / np.float32(A)
    c["mu"] = mu
    c["episode_offsets"] = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    c["returns"] = rng.randn(n) * 3 + 1.0
    return c


def device_run(rlx, dev, c, d=None, lds=(0, 0, 0, 0), offset=0, times=1):
    """-> (pi, row columns {name: fp64 [n]}, episode columns [3, E], out [7], status) of `times` calls in a row"""
    import torch
    d = int(c["batch_size"]) if d is None else d
    (n, A), E = c["q"].shape, len(c["episode_offsets"]) - 1
    ld_q, ld_rm, ld_mu, ld_pi = (A + x for x in lds)
    q, rm, mu = (_padded(c[k], ld, dev, offset) for k, ld in (("q", ld_q), ("reward_model", ld_rm), ("mu", ld_mu)))
    pi = torch.full((offset + n * ld_pi,), float("nan"), dtype=torch.float32, device=dev)[offset:]
    act, rew = _t(np.asarray(c["actions"], dtype=np.int32), dev), _t(np.asarray(c["rewards"], dtype=np.float32), dev)
    off, ret = _t(np.asarray(c["episode_offsets"], dtype=np.int32), dev), _t(np.asarray(c["returns"], dtype=np.float64), dev)
    cols = torch.full((6, n), float("nan"), dtype=torch.float64, device=dev)
    eps = torch.full((3, E), float("nan"), dtype=torch.float64, device=dev)
    out = torch.full((7,), float("nan"), dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for _ in range(times):
        rlx.ope_rows(q, ld_q, rm, ld_rm, d, act, rew, mu, ld_mu, float(c["temperature"]), n, A, pi, ld_pi, cols, status, 0)
        rlx.ope_reduce(off, E, n, cols, rew, ret, float(c["discount"]), eps, out, 0)
    torch.cuda.synchronize()
    p = pi.cpu().numpy().reshape(n, ld_pi)
    assert np.isnan(p[:, A:]).all()                                          # nothing written past a row's actions
    host = cols.cpu().numpy()
    return (np.ascontiguousarray(p[:, :A]), {k: host[i] for i, k in enumerate(ROW_COLUMNS)}, eps.cpu().numpy(),
            out.cpu().numpy(), int(status.item()))


def check(rlx, dev, c, d=None, **kw):
    """the assertions of the module's docstring on one case -> (device pi, device out, restated values)"""
    d = int(c["batch_size"]) if d is None else d
    pi, cols, eps, out, status = device_run(rlx, dev, c, d, **kw)
    T = float(c["temperature"])
    distance = ulps(pi, R.softmax32(c["q"], T))
    print("pi: worst distance %d ulp" % distance)
    assert distance <= PI_ULP
    values, scales, extras = R.evaluate(c["q"], c["reward_model"], d, c["actions"], c["rewards"], c["mu"], T,
                                        c["episode_offsets"], c["returns"], float(c["discount"]), pi=pi)
    assert status == extras["status"]
    for k in ROW_COLUMNS:
        assert np.array_equal(cols[k], extras[k], equal_nan=True), k
    n, E = len(c["actions"]), len(c["episode_offsets"]) - 1
    finite = np.isfinite(values) & np.isfinite(scales)
    limit = R.bound(n, scales)
    ok = np.isfinite(extras["ep_seq_dr"]) & np.isfinite(extras["ep_seq_dr_scale"])
    with np.errstate(invalid="ignore"):                                       # (a case may hold an inf or a NaN on purpose)
        print("estimates: |device - restatement| = %s, bound %s" % (np.abs(out[:5] - values), limit))
        assert (np.abs(out[:5] - values)[finite] <= limit[finite]).all()
        assert np.array_equal(out[:5][~finite], values[~finite], equal_nan=True)
        assert (np.abs(eps[0] - extras["ep_seq_dr"])[ok] <= R.bound(n, extras["ep_seq_dr_scale"])[ok]).all()
    assert np.allclose(eps[1], extras["ep_w"], rtol=n * 2.0 ** -52, atol=0, equal_nan=True)
    assert out[6] == E and (np.isclose(out[5], extras["sum_w"], rtol=n * 2.0 ** -52, atol=0) or not np.isfinite(out[5]))
    return pi, out, values


def test_recorded_cases(rlx, dev, gold):
    for i in cases(gold):
        c = case(gold, i)
        _, out, _ = check(rlx, dev, c)
        assert np.isfinite(out).all()


@pytest.mark.parametrize("lengths", [[64], [65], [1], [128, 129, 1, 2]])
def test_around_one_pass_of_the_episode_wave(rlx, dev, lengths):
    check(rlx, dev, make(lengths, 3, seed=sum(lengths), q_scale=0.05))


@pytest.mark.parametrize("d", [1, 32, 1000])
def test_direct_method_divisors(rlx, dev, d):
    c = make([7, 64, 65, 1, 13], 4, seed=d)
    _, out, _ = check(rlx, dev, c, d=d)
    _, other, _ = check(rlx, dev, c, d=1 if d != 1 else 32)
    assert out[1] != other[1] and out[2] != other[2] and np.array_equal(out[[0, 3, 4]], other[[0, 3, 4]])


@pytest.mark.parametrize("lds,offset", [((3, 1, 2, 5), 0), ((0, 0, 0, 0), 1), ((2, 2, 2, 2), 3)])
@pytest.mark.parametrize("A", [1, 2, 18])
def test_padded_leading_dimensions_and_unaligned_bases(rlx, dev, lds, offset, A):
    c = make([5, 70, 1], A, seed=A + offset)
    plain = device_run(rlx, dev, c)
    pi, _, _, out, _ = device_run(rlx, dev, c, lds=lds, offset=offset)
    check(rlx, dev, c, lds=lds, offset=offset)
    assert np.array_equal(pi, plain[0]) and np.array_equal(out, plain[3])


def test_large_q_over_temperature_needs_the_maximum_taken_off(rlx, dev):
    c = make([9, 66], 3, seed=5, T=0.2, q_offset=100.0, q_scale=0.05)       # q / T near 500: expf(500) is inf
    pi, out, _ = check(rlx, dev, c)
    assert np.isfinite(pi).all() and np.isfinite(out).all() and np.allclose(pi.sum(axis=1), 1, atol=1e-5)


def test_underflowed_policy_probabilities_give_a_wis_of_exactly_zero(rlx, dev):
    c = make([3, 65, 1], 3, seed=9, T=0.2)
    n = len(c["actions"])
    c["q"][np.arange(n), c["actions"]] -= np.float32(120 * 0.2)            # more than 110 T below the row's maximum
    pi, out, values = check(rlx, dev, c)
    assert (pi[np.arange(n), c["actions"]] == 0).all()
    assert out[4] == 0 and out[5] == 0 and out[0] == 0 and values[4] == 0 and not np.signbit(out[4])


def test_a_zero_behaviour_probability_propagates_as_in_numpy(rlx, dev):
    c = make([4, 1, 6], 3, seed=13)
    c["mu"][4, c["actions"][4]] = 0.0                                         # the episode of one row
    _, out, values = check(rlx, dev, c)
    assert np.isinf(out[0]) and np.isfinite(out[1]) and np.isinf(out[2]) and np.isinf(out[3]) and np.isnan(out[4])
    assert np.array_equal(out[:5], values, equal_nan=True)


def test_a_bad_action_sets_the_status_bit_and_leaves_the_other_rows_alone(rlx, dev):
    c = make([4, 70], 3, seed=17)
    good = device_run(rlx, dev, c)
    assert good[4] == 0
    for bad in (-1, 3):
        b = dict(c, actions=c["actions"].copy())
        b["actions"][5] = bad
        pi, cols, _, out, status = device_run(rlx, dev, b)
        assert status == 1 and np.array_equal(pi, good[0])
        keep = np.arange(len(b["actions"])) != 5
        for k in ROW_COLUMNS:
            assert cols[k][5] == 0 and np.array_equal(cols[k][keep], good[1][k][keep])
        check(rlx, dev, b)


def test_the_same_call_twice_gives_identical_bits(rlx, dev, gold):
    c = case(gold, 4)
    a, b = device_run(rlx, dev, c), device_run(rlx, dev, c, times=2)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
    assert np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64))
    for k in ROW_COLUMNS:
        assert np.array_equal(a[1][k].view(np.uint64), b[1][k].view(np.uint64))


def test_capturable(rlx, dev):
    import torch
    c = make([5, 70, 1], 2, seed=3)
    want = device_run(rlx, dev, c)
    (n, A), E = c["q"].shape, 3
    q, rm, mu = (_t(c[k], dev) for k in ("q", "reward_model", "mu"))
    act, rew = _t(c["actions"].astype(np.int32), dev), _t(c["rewards"], dev)
    off, ret = _t(c["episode_offsets"], dev), _t(c["returns"], dev)
    pi = torch.zeros(n, A, dtype=torch.float32, device=dev)
    cols, eps = torch.zeros(6, n, dtype=torch.float64, device=dev), torch.zeros(3, E, dtype=torch.float64, device=dev)
    out, status = torch.zeros(7, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            s = torch.cuda.current_stream().cuda_stream
            rlx.ope_rows(q, A, rm, A, 32, act, rew, mu, A, 0.2, n, A, pi, A, cols, status, s)
            rlx.ope_reduce(off, E, n, cols, rew, ret, 0.99, eps, out, s)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[3]) and np.array_equal(pi.cpu().numpy(), want[0])


def test_bad_arguments_are_refused(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    z = torch.zeros(64, dtype=torch.float64, device=dev)
    f, i = z.view(torch.float32), z.view(torch.int32)
    with pytest.raises(RlxError, match="actions"):
        rlx.ope_rows(f, 19, f, 19, 1, i, f, f, 19, 1.0, 1, 19, f, 19, z, i, 0)
    with pytest.raises(RlxError, match="leading dimension"):
        rlx.ope_rows(f, 2, f, 3, 1, i, f, f, 3, 1.0, 1, 3, f, 3, z, i, 0)
    with pytest.raises(RlxError, match="dm_row_divisor"):
        rlx.ope_rows(f, 3, f, 3, 0, i, f, f, 3, 1.0, 1, 3, f, 3, z, i, 0)
    with pytest.raises(RlxError, match="actions"):
        rlx.behaviour_probabilities(f, 0, z, 0.5, 0, 1.0, 1, 0, f, 1, 0)


# ------------------------------------------------------------------------------------------------ the acting side
def _behaviour(rlx, dev, q, u, eps, force, T, ld_q=None, ld_out=None):
    import torch
    n, A = q.shape
    ld_q, ld_out = ld_q or A, ld_out or A
    out = torch.full((n, ld_out), float("nan"), dtype=torch.float32, device=dev)
    rlx.behaviour_probabilities(_padded(q, ld_q, dev), ld_q, _t(np.asarray(u, dtype=np.float64), dev), float(eps),
                                int(force), float(T), n, A, out, ld_out, 0)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[:, A:]).all()
    return np.ascontiguousarray(got[:, :A])


@pytest.mark.parametrize("A,n", [(2, 1), (3, 2), (18, 70)])
def test_behaviour_probabilities(rlx, dev, A, n):
    import torch
    rng = np.random.RandomState(A)
    q = (rng.randn(n, A) + 1).astype(np.float32)
    u = rng.rand(n)
    u[0] = 0.5                                                              # u < epsilon is strict
    T = 0.2
    uniform = np.float32(1) / np.float32(A)
    # the policy probabilities rlx_ope_rows writes for the same Q values: the greedy rows share its function
    c = make([n], A, seed=1, T=T)
    c["q"] = q
    pi = device_run(rlx, dev, c)[0]
    # the draws rlx_egreedy explores on: with every random action out of range, an explored row is the one that is not
    # its argmax
    for eps in (0.0, 0.5, 1.0):
        got = _behaviour(rlx, dev, q, u, eps, False, T, ld_q=A + 1, ld_out=A + 3)
        explore = u < eps
        assert (got[explore].view(np.uint32) == uniform.view(np.uint32)).all()
        assert np.array_equal(got[~explore].view(np.uint32), pi[~explore].view(np.uint32))
        assert explore.all() if eps == 1.0 else not explore[0]               # u = 0.5 is not below epsilon = 0.5
        acts = torch.zeros(n, dtype=torch.int32, device=dev)
        marker = torch.full((n,), 0, dtype=torch.int32, device=dev)       # the random action is 0 ...
        qq = q.copy()
        qq[:, 0] = -100.0                                                   # ... which the greedy choice never is (A > 1)
        rlx.egreedy(_t(qq, dev), A, _t(u, dev), marker, _t(rng.rand(n, A), dev), float(eps), n, A, acts, 0)
        torch.cuda.synchronize()
        if A > 1:
            assert np.array_equal(acts.cpu().numpy() == 0, explore)
    forced = _behaviour(rlx, dev, q, u, 0.0, True, T)
    assert (forced.view(np.uint32) == uniform.view(np.uint32)).all()
    assert ulps(pi, R.softmax32(q, T)) <= PI_ULP
