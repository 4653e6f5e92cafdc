"""rlx_boltzmann_sample (csrc/explore_dist.hip) against tests/boltzmann_ref.py, the restatement of the reference's
Boltzmann.get_action in numpy's types and order — and the restatement against the method's own text."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boltzmann_ref as R  # noqa: E402

F32 = np.float32
# fp32 ulps between the device's probabilities and the restatement's (the device expf is not numpy's exp; everything
# else rounds alike): measured 5 over the cases below, recorded with a margin of 2x.  The last entry is
# 1 - sum(the others), a difference near 1: its error is counted in ulps of 1 (2^-24), not of its own small value.
PROB_ULP = 10
# the uniforms keep this distance from every cumulative boundary: a boundary moves by at most the sum of the entries'
# errors, PROB_ULP 2^-24 (sum p + 1) = 1.2e-6
U_MARGIN = 1e-5


@pytest.mark.parametrize("seed, A, T", [(0, 2, 1.0), (1, 65, 0.05), (2, 200, 0.3)])
def test_the_restatement_is_the_reference_method(seed, A, T):
    q = (np.random.RandomState(seed).randn(A) * 0.2).astype(F32)
    np.random.seed(seed + 10)
    # boltzmann.py:56-61, its text
    exp_probabilities = np.exp(q / T)
    probabilities = exp_probabilities / np.sum(exp_probabilities)
    probabilities[-1] = 1 - np.sum(probabilities[:-1])
    action = np.random.choice(range(A), p=probabilities)
    np.random.seed(seed + 10)
    got_action, got_p, bad = R.get_action(q, T, np.random.random_sample())
    assert probabilities.dtype == F32 and np.array_equal(got_p, probabilities) and got_action == action and not bad


def _uniforms(rng, cdfs):
    """the first len(cdfs) seeded uniforms at least U_MARGIN from every cumulative boundary of their row"""
    out, drawn = [], 0
    while len(out) < len(cdfs):
        u = rng.random_sample()
        drawn += 1
        if np.abs(cdfs[len(out)] - u).min() >= U_MARGIN:
            out.append(u)
    assert drawn - len(out) <= max(1, drawn // 10)
    return np.array(out)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1.0, 0.05])
@pytest.mark.parametrize("n_env, A, ld", [(1, 2, 2), (3, 5, 8), (4, 64, 64), (2, 65, 65), (5, 200, 200)])
def test_boltzmann_sample_matches_the_restatement(dev, n_env, A, ld, T):
    import torch
    from coach_amd import _rlx
    rng = np.random.RandomState(1000 * A + n_env)
    q = np.full((n_env, ld), np.nan, dtype=F32)                       # (NaN padding behind the row)
    q[:, :A] = (rng.randn(n_env, A) * 0.5).astype(F32)
    # the last probability is 1 - sum(the others): where it is rounding noise its SIGN is, and numpy refuses a negative
    # entry.  The last action shares the row's maximum, so that entry stays far above PROB_ULP * 2^-24 on both sides.
    q[:, A - 1] = q[:, :A].max(axis=1)
    p_ref = np.stack([R.probabilities(q[e, :A], T) for e in range(n_env)])
    u = _uniforms(rng, [R.cdf(p) for p in p_ref])
    a_ref = np.array([R.get_action(q[e, :A], T, u[e])[0] for e in range(n_env)])
    staged = torch.tensor(np.append(u, T), dtype=torch.float64, device=dev)
    probs = torch.full((n_env, A + 1), 7.0, dtype=torch.float32, device=dev)
    actions = torch.full((n_env,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _rlx.lib().boltzmann_sample(torch.from_numpy(q).to(dev), ld, staged, staged[n_env:], n_env, A, probs, A + 1,
                                actions, status, _rlx.current_stream())
    p = probs.cpu().numpy()
    unit = np.spacing(p_ref)
    unit[:, -1] = 2.0 ** -24
    ulps = np.abs(p[:, :A].astype(np.float64) - p_ref) / unit
    print("boltzmann n_env=%d A=%d T=%g: max ulp %.2f (last entry %.2f)" % (n_env, A, T, ulps.max(), ulps[:, -1].max()))
    assert ulps.max() <= PROB_ULP and (p[:, A] == 7.0).all() and int(status.item()) == 0
    np.testing.assert_array_equal(actions.cpu().numpy(), a_ref)


@pytest.mark.gpu
def test_a_nan_row_sets_the_status_and_the_policy_raises(dev):
    import torch
    from coach_amd import _rlx
    from coach_amd.exploration_policies import Boltzmann, BoltzmannParameters
    from coach_amd.schedules import LinearSchedule
    params = BoltzmannParameters()
    params.temperature_schedule = LinearSchedule(1.0, 0.01, 100)
    pol = Boltzmann(5, 3, dev, params)
    q = np.random.RandomState(3).randn(3, 5).astype(F32)
    q[1, 3] = np.nan
    actions = torch.zeros(3, dtype=torch.int32, device=dev)
    np.random.seed(4)
    pol.act(torch.from_numpy(q).to(dev), 5, actions)
    got = actions.cpu().numpy()
    assert got[1] == 3 and int(pol.status.item()) == _rlx.CONSTANTS["RLX_EXPLORE_STATUS_BAD_PROBABILITIES"]
    np.random.seed(4)
    us = [np.random.random_sample() for _ in range(3)]                # one uniform per env, in env order
    assert [got[e] for e in (0, 2)] == [R.get_action(q[e], 1.0, us[e])[0] for e in (0, 2)]
    with pytest.raises(ValueError, match="probabilities contain NaN"):
        pol.check()
