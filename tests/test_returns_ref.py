"""tests/returns_ref.py against oracle/returns.py (pinned to the reference by tests/golden/gae.npz) and, where the reference
tree is present, against the reference's own Episode class.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import returns_ref as R
from oracle import returns as O

F32, F64 = np.float32, np.float64
CASES = ["small", "ppo2048", "ragged"]


def _u64(x):
    return np.ascontiguousarray(x, dtype=F64).view(np.uint64)


def test_split_episodes():
    assert R.split_episodes([0, 0, 1, 0, 1]) == [(0, 3, True), (3, 5, True)]
    assert R.split_episodes([1, 1, 0]) == [(0, 1, True), (1, 2, True), (2, 3, False)]
    assert R.split_episodes([0]) == [(0, 1, False)]
    assert R.split_episodes([]) == []


@pytest.mark.parametrize("name", CASES)
def test_gae_equals_fill_advantages_on_the_golden_rollouts(golden, name):
    """the same statements in the same order on the same fp32 inputs: bit for bit.  (fill_advantages returns the complete
    episodes only; the golden rollouts end in a game_over.)"""
    g = golden("gae")
    disc, lam = g[name + "_hp"]
    rewards, values, go = g[name + "_rewards"].astype(F32), g[name + "_values"].astype(F32), g[name + "_go"]
    assert go[-1]
    _, ref_vt, ref_adv = O.fill_advantages(rewards, values.astype(F64), go, disc, lam)
    adv, vt = R.gae(rewards, values, go, None, disc, lam)
    assert np.array_equal(_u64(adv), _u64(ref_adv))
    assert np.array_equal(_u64(vt), _u64(ref_vt))
    # the oracle adds the discounted rewards in another order (the reference's pad-and-add): the project's scan tolerance
    np.testing.assert_allclose(R.discounted_returns(rewards, go, disc), O.discounted_returns(rewards, go, disc),
                               rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("T", [1, 2, 3, 7, 64, 300])
@pytest.mark.parametrize("disc,lam", [(0.99, 0.95), (1.0, 1.0), (0.0, 0.95), (0.99, 0.0)])
def test_small_random_cases(T, disc, lam):
    rng = np.random.RandomState(T)
    rewards, values = rng.randn(T).astype(F32), rng.randn(T).astype(F32)
    go = rng.rand(T) < 0.2
    go[-1] = True
    _, ref_vt, ref_adv = O.fill_advantages(rewards, values.astype(F64), go, disc, lam)
    adv, vt = R.gae(rewards, values, go, 123.0, disc, lam)             # a bootstrap under a final game_over is ignored
    assert np.array_equal(_u64(adv), _u64(ref_adv)) and np.array_equal(_u64(vt), _u64(ref_vt))
    np.testing.assert_allclose(R.discounted_returns(rewards, go, disc), O.discounted_returns(rewards, go, disc),
                               rtol=1e-11, atol=1e-12)
    # an open end: discounted_returns continues into 0 as the oracle does; gae sees the bootstrap as one more value
    go[-1] = False
    np.testing.assert_allclose(R.discounted_returns(rewards, go, disc), O.discounted_returns(rewards, go, disc),
                               rtol=1e-11, atol=1e-12)
    start = max([b for _, b, closed in R.split_episodes(go) if closed] + [0])
    adv, vt = R.gae(rewards, values, go, 0.7, disc, lam)
    tail_adv, tail_vt = O.gae_episode(rewards[start:], np.append(values[start:].astype(F64), F64(F32(0.7))), disc, lam)
    assert np.array_equal(_u64(adv[start:]), _u64(tail_adv)) and np.array_equal(_u64(vt[start:]), _u64(tail_vt))
    assert np.array_equal(_u64(adv[:start]), _u64(ref_adv[:start]))


def test_nonfinite_values_stay_inside_their_episode():
    """rewards [1, 2, 3, inf, 1] with game_over at steps 2 and 4: the first episode is finite"""
    go = [0, 0, 1, 0, 1]
    r = np.array([1, 2, 3, np.inf, 1], dtype=F32)
    with np.errstate(invalid="ignore"):
        want = O.discounted_returns(r, go, 0.99)
    got = R.discounted_returns(r, go, 0.99)
    np.testing.assert_allclose(got[:3], [1 + 0.99 * (2 + 0.99 * 3), 2 + 0.99 * 3, 3], rtol=1e-15)
    assert np.isposinf(got[3]) and got[4] == 1.0
    assert np.array_equal(np.isposinf(want), np.isposinf(got)) and np.isfinite(want[:3]).all()
    np.testing.assert_allclose(got[:3], want[:3], rtol=1e-12)
    v = np.array([0.5, 0.25, -1, np.nan, 2], dtype=F32)
    adv, vt = R.gae(np.ones(5, dtype=F32), v, go, None, 0.99, 0.95)
    with np.errstate(invalid="ignore"):
        _, ref_vt, ref_adv = O.fill_advantages(np.ones(5, dtype=F32), v.astype(F64), go, 0.99, 0.95)
    assert np.isfinite(adv[:3]).all() and np.isnan(adv[3]) and np.isfinite(adv[4])
    assert np.array_equal(np.isnan(adv), np.isnan(ref_adv)) and np.array_equal(_u64(adv[:3]), _u64(ref_adv[:3]))
    assert np.array_equal(np.isnan(vt), np.isnan(ref_vt))


def test_a_zero_discount_keeps_the_references_own_nan():
    """inside ONE episode the reference computes r + 0 * inf = NaN for the step before an inf: that is not a leak"""
    r = np.array([1, 2, np.inf, 4], dtype=F32)
    go = [0, 0, 0, 1]
    with np.errstate(invalid="ignore"):
        want = O.lfilter_discount(r.astype(F64), 0.0)
    got = R.discounted_returns(r, go, 0.0)
    assert np.isnan(want[1]) and np.isnan(got[1]) and np.isnan(got[0])
    assert np.isposinf(got[2]) and got[3] == 4.0
    assert np.array_equal(np.isnan(want), np.isnan(got))


@pytest.mark.parametrize("T", R.NSTEP_T)
def test_nstep_returns_equals_the_oracles_episode_return(T):
    rewards = R.nstep_rewards(T)
    full = R.nstep_returns(rewards, 0.97, -1)
    assert np.array_equal(_u64(full), _u64(O.discounted_returns_episode(rewards, 0.97)))
    assert np.array_equal(_u64(R.nstep_returns(rewards, 0.97, T + 5)), _u64(full))
    assert np.array_equal(_u64(R.nstep_returns(rewards, 0.97, T)), _u64(full))
    assert np.array_equal(_u64(R.nstep_returns(rewards, 0.97, 1)), _u64(rewards.astype(F64)))
    if T >= 3:
        two = R.nstep_returns(rewards, 0.97, 2)
        r = rewards.astype(F64)
        assert np.array_equal(_u64(two[:-1]), _u64(r[:-1] + 0.97 * r[1:])) and two[-1] == r[-1]
    with pytest.raises(ValueError):
        R.nstep_returns(rewards, 0.97, 0)


@pytest.mark.reference
def test_nstep_returns_equals_the_references_episode():
    """a process of its own: the stub-import harness replaces modules for everything imported after it"""
    res = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "returns_ref.py"),
                          "--against-reference"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    n_cases = sum(len([k for k in R.nstep_cases(T) if k != 0]) for T in R.NSTEP_T)
    assert "equals the reference's Episode in %d cases" % n_cases in res.stdout, res.stdout[-4000:]


@pytest.mark.parametrize("n_env", [1, 5, 65])
def test_episode_stats_equals_the_oracle(n_env):
    rng = np.random.RandomState(n_env)
    mine = R.EpisodeStats(n_env, np.full(n_env, -7.5), np.full(n_env, -3))
    theirs = O.EpisodeStatsOracle(n_env)
    never = np.ones(n_env, dtype=bool)
    for s in range(10):
        rew = rng.randn(n_env).astype(F32)
        done = rng.rand(n_env) < 0.25
        if s == 4:
            done[:] = False
            before = mine.acc().copy()
        mine.step(rew, done)
        theirs.step(rew, done)
        if s == 4:
            assert np.array_equal(mine.acc(), before)
        never &= ~done
        np.testing.assert_allclose(mine.acc(), theirs.acc(), rtol=1e-15)
        assert np.array_equal(mine.ep_return, theirs.ep_return) and np.array_equal(mine.ep_len, theirs.ep_len)
    assert (mine.last_return[never] == -7.5).all() and (mine.last_len[never] == -3).all()
    assert (mine.last_len[~never] >= 1).all()


def test_standardize_is_numpys():
    x = np.random.RandomState(0).randn(1025)
    out, mean, std = R.standardize(x)
    assert mean == np.mean(x) and std == np.std(x) and np.array_equal(out, (x - np.mean(x)) / np.std(x))
    assert np.isnan(R.standardize(np.array([3.0]))[0]).all()                       # 0 / 0
    assert np.isnan(R.standardize(np.full(1024, 0.5))[0]).all()
