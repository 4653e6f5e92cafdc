"""tests/ope_ref.py (the numpy restatement of csrc/ope.hip) against the reference's own OpeManager, DoublyRobust,
SequentialDoublyRobust and WeightedImportanceSampling, as recorded in tests/golden/ope.npz by make_golden_ope.py.

The two differ only by the reference's fp32 intermediates (it divides, multiplies and sums the fp32 network outputs in
fp32; the restatement widens them once and works in fp64).  Measured on the committed cases: the worst
|restatement - recording| / scale over the seven cases and five estimates is MEASURED_WORST (the scale is the
restatement's own: the same computation on absolute values).  The test asserts 10 x that.
"""
import os

import numpy as np
import pytest

import ope_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEASURED_WORST = 4.1e-7          # case 3 (A = 3, T = 1), sequential doubly robust; the other 34 figures are <= 1.5e-7
TOLERANCE = 10 * MEASURED_WORST


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "ope.npz"))


def cases(gold):
    return range(int(gold["cases"]))


def case(gold, i):
    p = "c%d_" % i
    return {k[len(p):]: gold[k] for k in gold.files if k.startswith(p)}


def restated(c, d=None, pi=None):
    d = int(c["batch_size"]) if d is None else d
    return R.evaluate(c["q"], c["reward_model"], d, c["actions"], c["rewards"], c["mu"], float(c["temperature"]),
                      c["episode_offsets"], c["returns"], float(c["discount"]), pi=pi)


def test_the_cases_are_the_ones_the_fixture_was_asked_for(gold):
    seen = [(case(gold, i)["lengths"].tolist(), int(case(gold, i)["n_actions"]), int(case(gold, i)["batch_size"]),
             float(case(gold, i)["temperature"])) for i in cases(gold)]
    for lengths, A in (([1], 2), ([1] * 5, 2), ([7, 64, 65, 1, 200, 13], 3), ([129, 1, 63, 300], 18)):
        assert any(s[0] == lengths and s[1] == A for s in seen)
    assert {s[3] for s in seen} == {0.2, 1.0}
    assert any(s[2] == 32 for s in seen) and any(s[2] > sum(s[0]) > 32 for s in seen)
    for i in cases(gold):
        c = case(gold, i)
        assert c["mu"].dtype == np.float32 and c["rewards"].dtype == np.float32
        A = int(c["n_actions"])
        assert (c["mu"][::2] == np.float32(1) / np.float32(A)).all() and (c["mu"] >= np.float32(0.2 / A) * 0.999).all()
        # the input condition: sum w_e is not made of products that underflowed in the reference's fp32
        assert restated(c)[2]["ep_w"].max() > 1e-3


def test_restatement_equals_the_recording(gold):
    worst = 0.0
    for i in cases(gold):
        c = case(gold, i)
        values, scales, extras = restated(c)
        assert np.isfinite(values).all() and np.isfinite(c["ref_estimates"]).all()
        err = np.abs(values - c["ref_estimates"]) / scales
        print("case %d: |restatement - recording| / scale = %s" % (i, " ".join("%s=%.3e" % kv for kv in zip(R.NAMES, err))))
        worst = max(worst, float(err.max()))
        assert (err <= TOLERANCE).all(), (i, err)
        # the policy probabilities the manager kept are the stand-in's softmax; its v values are their fp32 sums
        assert np.array_equal(c["ref_pi"], extras["pi"])
        assert np.allclose(c["ref_v"], extras["v"], rtol=0, atol=1e-5)
    print("worst: %.3e" % worst)
    assert worst >= MEASURED_WORST / 10, "the documented figure is stale: measured %.3e" % worst


def test_the_direct_method_quirk_is_what_was_recorded(gold):
    """ope_manager.py:80 multiplies every row of inference batch i by the reward model's output of dataset row i: the
    recording is met with d = batch size and missed, in DM and in DR (which adds DM), with the paper's d = 1"""
    differs = 0
    for i in cases(gold):
        c = case(gold, i)
        values, scales, _ = restated(c, d=1)
        err = np.abs(values - c["ref_estimates"]) / scales
        assert (err[[0, 3, 4]] <= TOLERANCE).all()                          # IPS, sequential DR and WIS do not use it
        if len(c["actions"]) > 1:
            assert err[1] > 100 * TOLERANCE and err[2] > 100 * TOLERANCE, (i, err)      # far outside the agreement
            differs += 1
        else:
            assert (err <= TOLERANCE).all()                                   # one row: row 0 either way
    assert differs >= 5


def test_softmax_and_behaviour_probabilities():
    q = np.array([[1.0, 2.0, 3.0], [100.0, 99.0, -50.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    p = R.softmax32(q, 0.2)
    assert p.dtype == np.float32 and np.isfinite(p).all()                    # q / T = 500: finite only with the maximum taken off
    assert np.allclose(p.sum(axis=1), 1, atol=1e-6) and p[1, 2] == 0 and (p[2] == np.float32(1) / np.float32(3)).all()
    b = R.behaviour_probabilities(q, [0.1, 0.6, 0.4], 0.5, False, 0.2)
    assert (b[0] == np.float32(1) / np.float32(3)).all() and np.array_equal(b[1], p[1]) and (b[2] == p[2]).all()
    assert (R.behaviour_probabilities(q, None, 0.0, True, 0.2) == np.float32(1) / np.float32(3)).all()


def test_rows_edge_cases():
    q = np.array([[1.0, 2.0], [3.0, 1.0], [0.5, 0.25]], dtype=np.float32)
    rm = np.array([[0.5, -1.0], [2.0, 4.0], [1.0, 1.0]], dtype=np.float32)
    mu = np.array([[0.5, 0.5], [0.0, 1.0], [0.25, 0.75]], dtype=np.float32)
    cols = R.rows(q, rm, 1, [1, 0, 7], [1.0, 2.0, 3.0], mu, 1.0)
    assert cols["status"] == 1 and np.isinf(cols["rho"][1]) and cols["rho"][2] == 0 and cols["dm"][2] == 0
    pi = cols["pi"].astype(np.float64)
    assert cols["rho"][0] == pi[0, 1] / 0.5 and cols["dr"][0] == cols["rho"][0] * (1.0 - -1.0)
    assert cols["dm"][1] == pi[1, 0] * 2.0 + pi[1, 1] * 4.0
    assert R.rows(q, rm, 2, [1, 0, 1], [1.0, 2.0, 3.0], mu, 1.0)["dm"][1] == pi[1, 0] * 0.5 + pi[1, 1] * -1.0
