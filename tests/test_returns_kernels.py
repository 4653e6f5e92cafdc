"""csrc/returns.hip, every entry point called by name against tests/returns_ref.py: the per-episode sequential float64
recurrence (rlx_gae, rlx_discounted_returns), numpy's mean / std (rlx_standardize), per-env totals
(rlx_episode_stats_step) and the reference's pad-and-add n-step return (rlx_episode_nstep_returns).

Tolerances.  The scan re-associates the recurrence, so its float64 outputs are held to the project's own figure from
tests/test_returns.py, rtol 1e-11 + atol 1e-12 (SCAN_RTOL / SCAN_ATOL).  An fp32 output is the kernel's last step, one
rounding of its float64 value (+ float64(values) for the value target): bit-identical to that rounding, and within one
fp32 ulp of the reference plus what the scan tolerance allows the float64 value underneath.  Everything else is a
sequence of single float64 operations in the reference's order and is compared bit for bit.

Every output is an interior slice of a larger allocation filled with 0xA5 (tests.test_frontend_kernels.Guarded); the
bytes around it and every input buffer must come back unchanged."""
import numpy as np
import pytest

import returns_ref as R
from test_frontend_kernels import FILL, Guarded, same_bits

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SCAN_RTOL, SCAN_ATOL = 1e-11, 1e-12
SEQ_LENS = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097]
HYPER = [(0.99, 0.95), (1.0, 1.0), (0.0, 0.95), (0.99, 0.0)]
SINGLE_FLAGS = [3, 4, 255, 256, 1023, 1024]      # reversed index j (t = L - 1 - j): thread-item, wave and tile boundaries
BOOTSTRAPS = np.array([0.7, -1.3, 2.1], dtype=F32)


def _patterns(L, rng):
    out = [("none", np.zeros(L, dtype=np.uint8)), ("all", np.ones(L, dtype=np.uint8))]
    last = np.zeros(L, dtype=np.uint8)
    last[-1] = 1
    out.append(("last", last))
    out.append(("random", (rng.rand(L) < 0.15).astype(np.uint8)))
    for j in SINGLE_FLAGS:
        if j < L:
            one = np.zeros(L, dtype=np.uint8)
            one[L - 1 - j] = 1
            out.append(("single_j%d" % j, one))
    return out


class Inputs(object):
    """device copies of the inputs, guarded like the outputs: a kernel must not write them"""

    def __init__(self, dev, **arrays):
        import torch
        kinds = {np.dtype(F32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(F64): torch.float64}
        self.host = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        self.dev = {k: Guarded(v.nbytes, dev, kinds[v.dtype], init=v) for k, v in self.host.items()}

    def __getitem__(self, k):
        return self.dev[k].t

    def part(self, k, lo, hi):
        return self.dev[k].t[lo:hi]

    def check_unchanged(self):
        for k, g in self.dev.items():
            assert np.array_equal(g.numpy().view(np.uint8), self.host[k].view(np.uint8)), "%s was written" % k
            g.check_guards()


def _out(dev, n, double):
    import torch
    return Guarded((8 if double else 4) * n, dev, torch.float64 if double else torch.float32)


def _class_of(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    x = np.asarray(x, dtype=F64)
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0)))


def _assert_scan64(got, want, what):
    assert np.array_equal(_class_of(got), _class_of(want)), (what, "finite / inf / NaN pattern",
                                                             np.flatnonzero(_class_of(got) != _class_of(want))[:8])
    ok = np.isfinite(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=SCAN_RTOL, atol=SCAN_ATOL, err_msg=str(what))


def _assert_out32(got32, dev64, plus, ref, ref_scan, what):
    """got32: the fp32 output; dev64 (+ plus): the device's own float64 value it was rounded from; ref: the reference of the
    same quantity; ref_scan: the reference of the scanned quantity, whose tolerance carries over"""
    with np.errstate(invalid="ignore", over="ignore"):
        own = (dev64 if plus is None else dev64 + plus.astype(F64)).astype(F32)
        assert same_bits(got32, own), (what, "not the rounding of the float64 output")
        ok = np.isfinite(ref) & np.isfinite(ref.astype(F32))
        assert np.array_equal(_class_of(got32[~ok]), _class_of(ref.astype(F32)[~ok])), what
        ulp = np.spacing(np.abs(ref[ok]).astype(F32)).astype(F64)
        slack = SCAN_RTOL * np.abs(ref_scan[ok]) + SCAN_ATOL
        assert np.all(np.abs(got32[ok].astype(F64) - ref[ok]) <= ulp + slack), what


def _run_gae(rlx, dev, inp, n_seq, L, disc, lam, lo=0, with_vt=True, boot=True):
    adv, vt = _out(dev, n_seq * L, True), _out(dev, n_seq * L, False)
    hi = lo + n_seq * L
    rlx.gae(inp.part("rewards", lo, hi), inp.part("values", lo, hi), inp.part("go", lo, hi),
            inp.part("boot", lo // L, lo // L + n_seq) if boot else None, n_seq, L, disc, lam, adv.t,
            vt.t if with_vt else None, 0)
    adv.check_guards()
    vt.check_guards()
    if not with_vt:
        assert (vt.numpy().view(np.uint8) == FILL).all()
    return adv.numpy(), vt.numpy()


def _run_returns(rlx, dev, inp, n_seq, L, disc, lo=0, with_32=True):
    ret, ret32 = _out(dev, n_seq * L, True), _out(dev, n_seq * L, False)
    hi = lo + n_seq * L
    rlx.discounted_returns(inp.part("rewards", lo, hi), inp.part("go", lo, hi), n_seq, L, disc, ret.t,
                           ret32.t if with_32 else None, 0)
    ret.check_guards()
    ret32.check_guards()
    if not with_32:
        assert (ret32.numpy().view(np.uint8) == FILL).all()
    return ret.numpy(), ret32.numpy()


def _check_scans(rlx, dev, rewards, values, go, L, disc, lam, what, isolated_calls=True):
    """3 sequences of L steps with their own bootstraps: rlx_gae and rlx_discounted_returns against the reference, with and
    without the fp32 output, and each sequence alone"""
    n_seq = 3
    inp = Inputs(dev, rewards=rewards, values=values, go=go, boot=BOOTSTRAPS)
    ref_adv, ref_vt, ref_ret = np.empty(n_seq * L), np.empty(n_seq * L), np.empty(n_seq * L)
    for q in range(n_seq):
        s = slice(q * L, (q + 1) * L)
        ref_adv[s], ref_vt[s] = R.gae(rewards[s], values[s], go[s], BOOTSTRAPS[q], disc, lam)
        ref_ret[s] = R.discounted_returns(rewards[s], go[s], disc)
    adv, vt = _run_gae(rlx, dev, inp, n_seq, L, disc, lam)
    _assert_scan64(adv, ref_adv, what + ("gae",))
    _assert_out32(vt, adv, values, ref_vt, ref_adv, what + ("value targets",))
    ret, ret32 = _run_returns(rlx, dev, inp, n_seq, L, disc)
    _assert_scan64(ret, ref_ret, what + ("returns",))
    _assert_out32(ret32, ret, None, ref_ret, ref_ret, what + ("returns32",))
    # the optional outputs change nothing
    assert same_bits(_run_gae(rlx, dev, inp, n_seq, L, disc, lam, with_vt=False)[0], adv), what + ("value_targets=None",)
    assert same_bits(_run_returns(rlx, dev, inp, n_seq, L, disc, with_32=False)[0], ret), what + ("returns32=None",)
    if isolated_calls:
        for q in range(n_seq):
            s = slice(q * L, (q + 1) * L)
            a1, v1 = _run_gae(rlx, dev, inp, 1, L, disc, lam, lo=q * L)
            r1, r321 = _run_returns(rlx, dev, inp, 1, L, disc, lo=q * L)
            assert same_bits(a1, adv[s]) and same_bits(v1, vt[s]), what + ("sequence %d alone, gae" % q,)
            assert same_bits(r1, ret[s]) and same_bits(r321, ret32[s]), what + ("sequence %d alone, returns" % q,)
    inp.check_unchanged()
    return adv, ret


@pytest.mark.parametrize("disc,lam", HYPER)
@pytest.mark.parametrize("L", SEQ_LENS)
def test_scans_equal_the_per_episode_recurrence(rlx, dev, L, disc, lam):
    rng = np.random.RandomState(L)
    for name, one in _patterns(L, rng):
        rewards, values = rng.randn(3 * L).astype(F32), rng.randn(3 * L).astype(F32)
        go = np.concatenate([one, one, one]) if name != "random" else (rng.rand(3 * L) < 0.15).astype(np.uint8)
        _check_scans(rlx, dev, rewards, values, go, L, disc, lam, (name, L, disc, lam))


def test_a_bootstrap_under_a_final_game_over_is_ignored(rlx, dev):
    rng = np.random.RandomState(3)
    L = 1027
    rewards, values = rng.randn(L).astype(F32), rng.randn(L).astype(F32)
    go = (rng.rand(L) < 0.1).astype(np.uint8)
    go[-1] = 1
    outs = []
    for boot in (None, 0.0, 55.5, np.nan):
        inp = Inputs(dev, rewards=rewards, values=values, go=go, boot=np.array([0.0 if boot is None else boot], dtype=F32))
        outs.append(_run_gae(rlx, dev, inp, 1, L, 0.99, 0.95, boot=boot is not None))
    for adv, vt in outs[1:]:
        assert same_bits(adv, outs[0][0]) and same_bits(vt, outs[0][1])
    _assert_scan64(outs[0][0], R.gae(rewards, values, go, None, 0.99, 0.95)[0], ("final game_over",))


# ------------------------------------------------------------------------------------------------ isolation
# the game_over sits at reversed index j, the non-finite value one step later in time, at j - 1: the pair lies inside one
# thread's four items (2), in neighbouring lanes (4), waves (256) and tiles (1024), and the same in the second tile
ISOLATION_J = [2, 4, 256, 1024, 1026, 1028, 1280, 2048]
ISOLATION_L = 2100


@pytest.mark.parametrize("far", [False, True], ids=["next_step", "last_step"])
@pytest.mark.parametrize("poison", ["reward+inf", "reward-inf", "rewardnan", "valuenan"])
@pytest.mark.parametrize("j", ISOLATION_J)
def test_nonfinite_values_do_not_cross_a_game_over(rlx, dev, j, poison, far):
    """A reward of +-inf / NaN (for GAE also a NaN value) in the episode AFTER a game_over: every earlier episode stays
    finite and within tolerance, and the outputs are non-finite, in the same class, exactly where the reference's are.
    far: the value sits at the trajectory's last step instead, so all of the later episode is non-finite and reaches the
    game_over through every wave total and tile carry in between."""
    L = ISOLATION_L
    rng = np.random.RandomState(j)
    rewards, values = rng.randn(3 * L).astype(F32), rng.randn(3 * L).astype(F32)
    go = np.zeros(3 * L, dtype=np.uint8)
    for q in range(3):
        go[q * L + L - 1 - j] = 1
        if j + 700 < L:
            go[q * L + L - 1 - (j + 700)] = 1
        t = q * L + (L - 1 if far else L - 1 - (j - 1))
        if poison == "valuenan":
            values[t] = np.nan
        else:
            rewards[t] = {"reward+inf": np.inf, "reward-inf": -np.inf, "rewardnan": np.nan}[poison]
    adv, ret = _check_scans(rlx, dev, rewards, values, go, L, 0.99, 0.95, (j, poison, far), isolated_calls=False)
    for q in range(3):
        first_bad = q * L + L - 1 - (j - 1)
        assert np.isfinite(adv[q * L:first_bad]).all() and np.isfinite(ret[q * L:first_bad]).all()
        assert not np.isfinite(adv[first_bad]) and (poison == "valuenan" or not np.isfinite(ret[first_bad]))


@pytest.mark.parametrize("j", [1, 2, 4, 256, 1024])
def test_a_zero_discount_keeps_the_references_nan(rlx, dev, j):
    """discount = 0 makes every map's slope 0 WITHOUT a game_over: inside one episode the reference computes
    r + 0 * inf = NaN for the step before an inf, and so must the kernel (a == 0 is not a cut)."""
    L = ISOLATION_L
    rng = np.random.RandomState(j)
    rewards, values = rng.randn(3 * L).astype(F32), rng.randn(3 * L).astype(F32)
    go = np.zeros(3 * L, dtype=np.uint8)
    for q in range(3):
        go[q * L + L - 1] = 1
        rewards[q * L + L - 1 - (j - 1)] = np.inf
    adv, ret = _check_scans(rlx, dev, rewards, values, go, L, 0.0, 0.95, (j, "discount 0"), isolated_calls=False)
    for q in range(3):
        t = q * L + L - 1 - j                                     # the step before the inf
        assert np.isnan(ret[t]) and np.isnan(adv[t]) and np.isposinf(ret[t + 1])
        assert np.isnan(ret[q * L:t]).all()                      # 0 * NaN: the reference's NaN runs to the episode's start


# ------------------------------------------------------------------------------------------------ rlx_standardize

def _standardize(rlx, dev, x, out32=True, out64=True, stats=True):
    import torch
    n = x.size
    inp = Inputs(dev, x=x)
    o32, o64, ms = _out(dev, n, False), _out(dev, n, True), _out(dev, 2, True)
    rlx.standardize(inp["x"], n, o32.t if out32 else None, o64.t if out64 else None, ms.t if stats else None, 0)
    for buf, used in ((o32, out32), (o64, out64), (ms, stats)):
        buf.check_guards()
        assert used or (buf.numpy().view(np.uint8) == FILL).all()
    inp.check_unchanged()
    return o32.numpy(), o64.numpy(), ms.numpy()


@pytest.mark.parametrize("offset", [0.0, 1e6])
@pytest.mark.parametrize("n", [2, 1023, 1024, 1025, 5000])
def test_standardize_equals_numpy(rlx, dev, n, offset):
    """(x - mean) / std with numpy's mean and std, no epsilon.  Unit-scale data: the project's tolerances (1e-12 for the
    statistics, 1e-10 for the values, tests/test_returns.py).  Mean 1e6, std 1: x - mean loses log2(max|x| / std) bits
    in either implementation, so the absolute terms are scaled by max|x| / std."""
    x = np.random.RandomState(n).randn(n) + offset
    want, mean, std = R.standardize(x)
    scale = np.abs(x).max() / std if offset else 1.0
    o32, o64, ms = _standardize(rlx, dev, x)
    np.testing.assert_allclose(ms[0], mean, rtol=1e-12, atol=1e-14 * scale)
    np.testing.assert_allclose(ms[1], std, rtol=1e-12 * scale, atol=0)
    np.testing.assert_allclose(o64, want, rtol=1e-10, atol=1e-12 * scale)
    assert same_bits(o32, o64.astype(F32))
    a32, _, ms_a = _standardize(rlx, dev, x, out64=False)
    _, b64, _ = _standardize(rlx, dev, x, out32=False, stats=False)
    assert same_bits(a32, o32) and same_bits(b64, o64) and same_bits(ms_a, ms)


@pytest.mark.parametrize("case", ["one_element", "constant"])
def test_standardize_of_a_zero_spread_is_nan_as_in_numpy(rlx, dev, case):
    """no epsilon in the reference (clipped_ppo_agent.py:201): 0 / 0.  1024 copies of 0.5 have an exact mean in any order."""
    x = np.array([3.25]) if case == "one_element" else np.full(1024, 0.5)
    want, mean, std = R.standardize(x)
    assert np.isnan(want).all() and std == 0.0
    o32, o64, ms = _standardize(rlx, dev, x)
    assert np.isnan(o32).all() and np.isnan(o64).all()
    assert ms[0] == mean and ms[1] == 0.0


# ------------------------------------------------------------------------------------------------ rlx_episode_stats_step

@pytest.mark.parametrize("with_last", [True, False])
@pytest.mark.parametrize("n_env", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_episode_stats_step(rlx, dev, n_env, with_last):
    """ep_return / ep_len / last_return / last_len are single float64 adds and copies per env: bit for bit.  The 8
    accumulators are tree sums over the envs: the project's rtol 1e-12.  last_* are written where an episode ended and keep
    their sentinel elsewhere.  A step without a game_over leaves the accumulators' bits alone, +-inf included."""
    import torch
    rng = np.random.RandomState(n_env)
    ep_ret, ep_len, acc = _out(dev, n_env, True), Guarded(4 * n_env, dev, torch.int32), _out(dev, 8, True)
    last_ret = Guarded(8 * n_env, dev, torch.float64, init=np.full(n_env, -7.5))
    last_len = Guarded(4 * n_env, dev, torch.int32, init=np.full(n_env, -3, dtype=np.int32))
    rlx.episode_stats_init(ep_ret.t, ep_len.t, n_env, acc.t, 0)
    ref = R.EpisodeStats(n_env, np.full(n_env, -7.5), np.full(n_env, -3))
    assert same_bits(acc.numpy(), ref.acc())
    for s in range(10):
        rew = rng.randn(n_env).astype(F32)
        done = (rng.rand(n_env) < 0.2).astype(np.uint8)
        if s in (0, 5):
            done[:] = 0
        if s == 1:
            done[-1] = 1                                  # the last env (a second trip of the loop for n_env > 1024)
        before = acc.numpy().copy()
        inp = Inputs(dev, rew=rew, done=done)
        rlx.episode_stats_step(inp["rew"], inp["done"], ep_ret.t, ep_len.t, n_env, acc.t, last_ret.t if with_last else None,
                               last_len.t if with_last else None, 0)
        ref.step(rew, done)
        inp.check_unchanged()
        if not done.any():
            assert same_bits(acc.numpy(), before), "a step without a game_over changed the accumulators"
            if s == 0:
                assert np.isneginf(before[3]) and np.isposinf(before[4]) and np.isneginf(before[6]) and np.isposinf(before[7])
        np.testing.assert_allclose(acc.numpy(), ref.acc(), rtol=1e-12)
        assert same_bits(ep_ret.numpy(), ref.ep_return) and np.array_equal(ep_len.numpy(), ref.ep_len)
        if with_last:
            assert same_bits(last_ret.numpy(), ref.last_return) and np.array_equal(last_len.numpy(), ref.last_len)
        else:
            assert (last_ret.numpy() == -7.5).all() and (last_len.numpy() == -3).all()
        for b in (ep_ret, ep_len, acc, last_ret, last_len):
            b.check_guards()
    assert ref.acc()[0] >= 1


# ------------------------------------------------------------------------------------------------ rlx_episode_nstep_returns

def _nstep_cases():
    out = []
    for T in R.NSTEP_T:
        for n_step in sorted(set(k for k in R.nstep_cases(T) if k != 0)):
            out.append((T, n_step))
    return out


def _nstep_setup(dev, T, rng):
    """a time-major ring of T + 3 steps x 3 envs whose env 1 holds an episode of T steps that starts on the ring's last row
    (so it wraps for T >= 2); the other envs' rewards are noise"""
    n_env, env, ring = 3, 1, T + 3
    first = ring - 1
    rewards = rng.randn(ring * n_env).astype(F32)
    rows = ((first + np.arange(T)) % ring) * n_env + env
    rewards[rows] = R.nstep_rewards(T)
    assert T < 2 or first + T > ring
    return n_env, env, ring, first, rewards, rows


@pytest.mark.parametrize("outputs", ["out", "compact", "both"])
@pytest.mark.parametrize("T,n_step", _nstep_cases())
def test_episode_nstep_returns_equal_the_reference_order(rlx, dev, T, n_step, outputs):
    """Episode.update_discounted_rewards (core_types.py:771-801): float64, the reference's order of additions and its
    running product of discounts, so bit for bit.  Rows of the other envs and rows outside the episode keep their bytes."""
    n_env, env, ring, first, rewards, rows = _nstep_setup(dev, T, np.random.RandomState(T))
    want = R.nstep_returns(rewards[rows], 0.97, n_step)
    inp = Inputs(dev, rewards=rewards)
    out, compact = _out(dev, ring * n_env, True), _out(dev, T, True)
    rlx.episode_nstep_returns(inp["rewards"], out.t if outputs != "compact" else None,
                              compact.t if outputs != "out" else None, first, T, env, n_env, ring, 0.97, n_step, 0)
    got, sentinel = out.numpy(), np.frombuffer(bytes([FILL]) * 8, dtype=F64)[0]
    expect = np.full(ring * n_env, sentinel)
    if outputs != "compact":
        expect[rows] = want
    assert np.array_equal(got.view(np.uint64), expect.view(np.uint64))
    if outputs != "out":
        assert same_bits(compact.numpy(), want)
    else:
        assert (compact.numpy().view(np.uint8) == FILL).all()
    out.check_guards()
    compact.check_guards()
    inp.check_unchanged()


@pytest.mark.parametrize("why", ["ring_shorter_than_the_episode", "n_step_0", "n_step_-2"])
def test_episode_nstep_returns_refusals(rlx, dev, why):
    from coach_amd._rlx import RlxError
    T = 5
    n_env, env, ring, first, rewards, rows = _nstep_setup(dev, T, np.random.RandomState(0))
    inp = Inputs(dev, rewards=rewards)
    out, compact = _out(dev, ring * n_env, True), _out(dev, T, True)
    with pytest.raises(RlxError, match="geometry" if why.startswith("ring") else "n-step should be an integer"):
        rlx.episode_nstep_returns(inp["rewards"], out.t, compact.t, 0, T, env, n_env, T - 1 if why.startswith("ring") else ring,
                                  0.97, {"n_step_0": 0, "n_step_-2": -2}.get(why, 2), 0)
    assert (out.numpy().view(np.uint8) == FILL).all() and (compact.numpy().view(np.uint8) == FILL).all()
    out.check_guards()
    compact.check_guards()
    inp.check_unchanged()
