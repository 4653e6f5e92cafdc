"""tests/mlp_ref.py on the CPU: (1) the float64 reference of the MLP DQN update against the fp32 numpy oracle
(oracle.agents.DQNOracle, pinned to the reference's learn_from_batch by tests/test_update_pins.py) at every seeded case
of tests/test_mlp_fused_edges.py, to fp32 rounding; (2) the unambiguous-input check of every one of those cases: the sign
of every pre-activation, the arg-max of every selecting Q row and the Huber branch of every row are further from their
discontinuity than an fp32 evaluation in any order can be from float64 -- so the GPU file compares every element of every
case, and a disagreement there is a wrong kernel, never an unlucky input.  The seeds stand in mlp_ref.SEEDS."""
import numpy as np
import pytest

import mlp_ref as R

CASES = R.case_list()
_ids = lambda k: "%s-%s-%s-%s" % ("x".join(map(str, R.SHAPES[k[0]][0])), "huber" if k[1] else "mse", "ddqn" if k[2] else "dqn", k[3])


def _oracle(c):
    from oracle.agents import DQNOracle
    arrays = {R.PARAM_NAMES[k]: [c["W"][k]] for k in R.NAMES}
    orc = DQNOracle(arrays, (c["dims"][0],), c["A"], "relu", R.LR, R.BETA1, R.BETA2, R.EPS, c["huber"])
    tower, head = orc.target
    for l, k in ((tower.layers[0], "1"), (tower.layers[1], "2"), (head, "3")):
        l.W[...] = c["Wt"]["w" + k]
        l.b[...] = c["Wt"]["b" + k]
    return orc


def test_case_list_covers_the_issue():
    """every shape with MSE and with Huber; DQN and Double DQN on the first, fourth and last; importance weights absent,
    fp32 and fp64; a seed for every case"""
    assert set(CASES) == set(R.SEEDS)
    for i in range(len(R.SHAPES)):
        assert {k[1] for k in CASES if k[0] == i} == {False, True}
    for i in (0, 3, len(R.SHAPES) - 1):
        assert {k[2] for k in CASES if k[0] == i} == {False, True}
    assert {k[3] for k in CASES} == {None, "f32", "f64"}


@pytest.mark.parametrize("key", CASES, ids=_ids)
def test_reference_matches_the_fp32_oracle(key):
    """Values: rtol 2e-5 + the a-priori fp32 bound (the oracle IS an fp32 evaluation).  Gradients: per tensor rtol 1e-4,
    atol 1e-5 max|g| -- numpy's fp32 matmul over K <= 2048 terms, error relative to the sum of the terms' magnitudes,
    not to a cancelled result."""
    c = R.make_case(key)
    res, orc = R.run_case(c), _oracle(c)
    w32 = None if c["iw"] is None else c["iw"]
    out = orc.learn_from_batch(c["s"], c["s2"], c["a"], c["r"], c["done"].astype(bool), R.DISCOUNT, w32, c["ddqn"], apply=False)
    rows = np.arange(c["B"])
    np.testing.assert_allclose(orc.head.y, res["q"], rtol=2e-5, atol=float(res["fwd"]["eq"].max()))
    got_y = out["td_targets"][rows, c["a"]]
    np.testing.assert_allclose(got_y, res["targets"], rtol=2e-5, atol=float(res["fwd_next_target"]["eq"].max()) + 1e-7)
    tol_td = res["fwd"]["eq"][rows, c["a"]] + res["fwd_next_target"]["eq"][rows, res["selected"]] + 1e-7
    assert np.all(np.abs(out["td_errors"] - res["td"]) <= tol_td + 2e-5 * np.abs(res["td"]))
    np.testing.assert_allclose(out["loss"], res["loss"], rtol=1e-4)
    np.testing.assert_allclose(out["norm"], res["norm"], rtol=1e-4)
    g32 = orc.grads()
    for k in R.NAMES:
        ref = res["grads"][k]
        np.testing.assert_allclose(g32[R.PARAM_NAMES[k]][0], ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max(), err_msg=k)
    # the first Adam step: the oracle's per-tensor TF1 Adam against adam_first_step
    orc.adam_step()
    w64, _, _ = R.adam_first_step(c["W"], res["grads"])
    w32 = orc.weights()
    for k in R.NAMES:
        np.testing.assert_allclose(w32[R.PARAM_NAMES[k]][0], w64[k], rtol=0, atol=5e-6, err_msg=k)


@pytest.mark.parametrize("key", CASES, ids=_ids)
def test_seeded_case_is_unambiguous(key):
    c = R.make_case(key)
    res = R.run_case(c)
    amb = R.ambiguity(res, c["huber"], c["ddqn"])
    print(key, amb)
    assert np.isfinite(res["loss"]) and res["status"] == 0
    assert amb["z"] > 1.0, "a pre-activation within its fp32 bound of 0"
    assert amb["gap"] > 1.0, "two Q values of a selecting row within their fp32 bounds"
    assert amb["huber"] > 1.0, "|e| within its fp32 bound of 1"
    if c["iw"] is not None and c["B"] > 1:
        assert (c["iw"] == 0).sum() == 1
    for g in res["grads"].values():                  # nothing degenerate: every tensor has a gradient to get wrong
        assert np.abs(g).max() > 0


@pytest.mark.parametrize("ddqn", [False, True])
def test_nan_case_reaches_inactive_units_and_matches_the_oracle_mask(ddqn):
    """The NaN case of the GPU file: unambiguous like the others; at least one unit of each hidden layer is inactive over
    the whole batch beyond its fp32 bound; under Double DQN some rows select the NaN column and some do not.  The oracle
    multiplies by relu' as mlp_ref does: the two agree on which gradient elements are NaN, and a select in their place
    (dy where y > 0, else 0) would not -- which is what the GPU test then asks of both device paths."""
    c = R.make_nan_case(ddqn)
    with np.errstate(invalid="ignore"):
        res, orc = R.run_case(c), _oracle(c)
        out = orc.learn_from_batch(c["s"], c["s2"], c["a"], c["r"], c["done"].astype(bool), R.DISCOUNT, None, ddqn, apply=False)
    amb = R.ambiguity(res, c["huber"], ddqn)
    assert min(amb.values()) > 1.0, amb
    dead1, dead2 = R.inactive_units(res)
    print("inactive over the batch: h1", dead1, "h2", dead2)
    assert len(dead1) >= 1 and len(dead2) >= 1
    nan_rows = np.isnan(res["td"])
    assert np.array_equal(nan_rows, res["selected"] == 1) and nan_rows.any()
    assert nan_rows.all() if not ddqn else not nan_rows.all()
    assert np.isnan(res["loss"]) and np.isnan(out["loss"])
    g32 = orc.grads()
    for k in R.NAMES:
        ref = res["grads"][k]
        got = g32[R.PARAM_NAMES[k]][0]
        assert np.array_equal(np.isnan(got), np.isnan(ref)), k
        fin = ~np.isnan(ref)
        if fin.any():
            np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-4, atol=1e-5 * np.abs(ref[fin]).max(), err_msg=k)
    # the multiplication reaches the inactive units: their column of W2 / entry of b2 (and of W1 / b1) is NaN
    assert np.isnan(res["grads"]["w2"][:, dead2]).all() and np.isnan(res["grads"]["b2"][dead2]).all()
    assert np.isnan(res["grads"]["w1"][:, dead1]).all() and np.isnan(res["grads"]["b1"][dead1]).all()
    # ... where a select would have left them finite
    f = res["fwd"]
    with np.errstate(invalid="ignore"):
        dq = np.zeros((c["B"], c["A"]))
        dq[np.arange(c["B"]), c["a"]] = 2.0 * res["e"] / c["B"]
        dz2_select = np.where(f["h2"] > 0, dq @ c["W"]["w3"].astype(np.float64).T, 0.0)
    assert np.isfinite(dz2_select.sum(0)[dead2]).all()


@pytest.mark.parametrize("ddqn", [False, True])
@pytest.mark.parametrize("variant", R.EDGE_VARIANTS)
def test_semantic_edge_cases_are_unambiguous(variant, ddqn):
    c, discount = R.make_edge_case(variant, ddqn)
    res = R.run_case(c, discount)
    amb = R.ambiguity(res, c["huber"], ddqn, discount)
    assert min(amb.values()) > 1.0, amb
    rows = {"all_done": np.arange(c["B"]), "done_255": np.array([7]), "discount_0": np.arange(c["B"]),
            "bad_actions": np.array([], dtype=int)}[variant]
    assert np.array_equal(res["targets"][rows], c["r"][rows].astype(np.float64))
    assert res["status"] == (1 if variant == "bad_actions" else 0)


@pytest.mark.parametrize("sign", [1, -1])
def test_huber_one_case_sits_on_the_branch_point(sign):
    c = R.make_huber_one_case(sign)
    res = R.run_case(c)
    assert np.array_equal(res["e"], np.full(c["B"], float(sign)))
    assert abs(res["loss"] - 0.5 * c["iw"].astype(np.float64).mean()) < 1e-12
    assert all(not res["grads"][k].any() for k in R.NAMES[:-1]) and res["grads"]["b3"].any()


def test_invalid_actions_take_no_part():
    dims, A, B = R.EDGE_SHAPE
    rng = np.random.RandomState(0)
    W = R.make_weights(dims, A, rng)
    s, s2 = rng.randn(B, dims[0]).astype(np.float32), rng.randn(B, dims[0]).astype(np.float32)
    a = rng.randint(0, A, B).astype(np.int32)
    r, done = rng.randn(B).astype(np.float32), np.zeros(B, np.uint8)
    full = R.update(W, W, s, s2, a, r, done, huber=True)
    a[3], a[11] = -1, A
    part = R.update(W, W, s, s2, a, r, done, huber=True)
    ok = np.ones(B, bool)
    ok[[3, 11]] = False
    assert part["status"] == 1 and full["status"] == 0
    assert np.isnan(part["td"][~ok]).all() and np.array_equal(part["td"][ok], full["td"][ok])
    assert part["loss"] < full["loss"]
