"""tests/targets_ref.py against what it builds on and against an independent derivative: oracle.targets and the fixtures of
tests/golden/targets.npz (bit for bit), torch autograd in float64 (the head loss and its gradient), the derived bound of
the fp32 loss sum, and a table of which input NaN reaches which output."""
import numpy as np
import pytest

import targets_ref as R
from oracle import targets as T
from test_frontend_kernels import same_bits

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ oracle and fixtures

@pytest.mark.parametrize("name", ["dqn", "ddqn"])
def test_dqn_targets_equal_the_oracle_and_the_fixtures(golden, name):
    g = golden("targets")
    sel = g[name + "_q_next_o"] if name == "ddqn" else None
    args = (g[name + "_actions"], g[name + "_rewards"], g[name + "_go"], 0.99)
    tt, err, status = R.dqn_targets(g[name + "_q_next_t"], sel, g[name + "_q_onl"], *args)
    o_tt, o_err = T.dqn_targets(g[name + "_q_next_t"], g[name + "_q_onl"], *args, q_next_online=sel)
    assert status == 0
    assert same_bits(tt, o_tt) and same_bits(err, o_err)
    assert same_bits(tt, g[name + "_targets"]) and same_bits(err, g[name + "_errors"])
    for huber in (0, 1):
        r = R.dqn_head_loss(g[name + "_q_onl"], g[name + "_q_next_t"], sel, *args[:3], None, 0.99, huber, 1.0)
        assert same_bits(r["td_targets"], g[name + "_targets"]) and same_bits(r["td_errors"], g[name + "_errors"])
        assert r["valid"].all() and not r["nan_huber"].any() and r["status"] == 0


def test_ac_wrappers_equal_the_oracle_and_the_fixtures(golden):
    g = golden("targets")
    t = R.ac_td_targets(g["ddpg_rewards"], g["ddpg_go"], g["ddpg_q_next"], 1, 0.99, 0, (-3.0, 3.0))
    assert same_bits(t, g["ddpg_targets"][:, 0].astype(F32))
    t = R.ac_td_targets(g["td3_rewards"], g["td3_go"], g["td3_q_next"], 1, 0.99, 0, None)
    assert same_bits(t, g["td3_targets"][:, 0].astype(F32))
    # q_stride: the columns behind the first are not looked at
    wide = np.full((len(g["td3_rewards"]), 3), np.nan, dtype=F32)
    wide[:, 0] = g["td3_q_next"][:, 0]
    assert same_bits(R.ac_td_targets(g["td3_rewards"], g["td3_go"], wide, 3, 0.99, 0, None), t)
    na = g["td3_next_actions"]
    A = na.shape[1]
    sm = R.td3_smooth_actions(na, g["td3_noise"], 0.5, np.full(A, -0.8, dtype=F32), np.full(A, 0.8, dtype=F32))
    # the fixture was clipped to the float64 bounds +-0.8; the entry point's bounds are fp32 numbers
    o = T.td3_smooth_actions(na, g["td3_noise"], 0.5, F64(F32(-0.8)), F64(F32(0.8)))
    assert same_bits(sm, o.astype(F32))
    inside = np.abs(g["td3_smoothed"]) < 0.8
    assert inside.any() and same_bits(sm[inside], g["td3_smoothed"][inside].astype(F32))
    obs = np.arange(na.shape[0] * 2, dtype=F32).reshape(-1, 2)
    m2, only = R.ac_merge_inputs(na, obs, na, g["td3_noise"], 0.5, np.full(A, -0.8, dtype=F32), np.full(A, 0.8, dtype=F32),
                                 obs + 1)
    assert same_bits(m2[0], np.concatenate([na, obs], 1)) and same_bits(m2[1], np.concatenate([sm, obs + 1], 1))
    assert same_bits(only, obs)
    m2, _ = R.ac_merge_inputs(na, obs, na, None, 0.5, None, None, obs + 1)
    assert same_bits(m2[1, :, :A], na.astype(F32))


def test_non_zero_terminal_discount_is_the_references_fp32_product():
    """ddpg_agent.py:157 / td3_agent.py:173 on the reference's operand types: `discount * q_st_plus_1` is a python float
    times the fp32 network output, which numpy evaluates in fp32 (discount rounded to fp32, the product rounded to fp32);
    only the sum with the float64 rewards is float64.  A product taken in float64 gives other fp32 targets in about
    three rows of ten, so the two are told apart here."""
    rng = np.random.RandomState(0)
    B = 1000
    rewards, q = rng.randn(B).astype(F32), (2 * rng.randn(B, 1)).astype(F32)
    literal = (rewards.astype(F64)[:, None] + 0.99 * q)[:, 0]              # the reference's statement, its dtypes
    assert (0.99 * q).dtype == F32 and literal.dtype == F64
    got = R.ac_td_targets(rewards, np.ones(B, dtype=np.uint8), q, 1, 0.99, 1, None)
    assert same_bits(got, literal.astype(F32))
    stated = (rewards.astype(F64) + (F32(0.99) * q[:, 0]).astype(F64)).astype(F32)
    assert same_bits(got, stated)
    in_float64 = (rewards.astype(F64) + 0.99 * q[:, 0].astype(F64)).astype(F32)
    assert 0.1 < np.mean(got != in_float64) < 0.6
    # the default branch is float64 throughout: (1.0 - game_overs) is a float64 array
    default = R.ac_td_targets(rewards, np.zeros(B, dtype=np.uint8), q, 1, 0.99, 0, None)
    assert same_bits(default, in_float64)


def test_rows_with_an_action_outside_the_range():
    q = np.arange(12, dtype=F32).reshape(4, 3)
    tt, err, status = R.dqn_targets(q + 1, None, q, [0, -1, 3, 2], np.ones(4, dtype=F32), [0, 0, 0, 255], 0.5)
    assert status == 1
    assert same_bits(tt[1:3], q[1:3]) and np.isnan(err[1:3]).all()
    assert tt[0, 0] == 1 + 0.5 * 3 and tt[3, 2] == 1.0 and err[3] == 10.0          # done = 255 is a done
    r = R.dqn_head_loss(q, q + 1, None, [0, -1, 3, 2], np.ones(4, dtype=F32), [0, 0, 0, 255], None, 0.5, 0, 1.0)
    assert not r["dq"][1:3].any() and r["terms64"][1] == 0 and r["terms64"][2] == 0
    assert r["valid"].tolist() == [True, False, False, True]


# ------------------------------------------------------------------------------------------------ autograd

def _batch(B, A, seed):
    rng = np.random.RandomState(seed)
    return dict(q=rng.randn(B, A).astype(F32), q_next=rng.randn(B, A).astype(F32), q_sel=rng.randn(B, A).astype(F32),
                actions=rng.randint(0, A, size=B), rewards=(2 * rng.randn(B)).astype(F32),
                dones=(rng.rand(B) < 0.3).astype(np.uint8), weights=rng.rand(B) + 0.1)


@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("huber", [0, 1])
@pytest.mark.parametrize("B,A", [(1, 1), (7, 3), (100, 18)])
def test_head_loss_and_gradient_equal_autograd_in_float64(B, A, huber, weighted, grad_scale):
    """the same targets, the loss written the way heads/q_head.py and head.py:172-181 state it (a weighted mean over the
    batch of the per-sample loss of the target matrix), differentiated by torch in float64.  The reference's dq is an fp32
    chain of 4 roundings on the way from e (the subtraction, grad_scale * w, * g, / B): gamma_4 of the float64 value."""
    import torch
    c = _batch(B, A, B + A)
    w = c["weights"] if weighted else None
    r = R.dqn_head_loss(c["q"], c["q_next"], c["q_sel"], c["actions"], c["rewards"], c["dones"], w, 0.99, huber, grad_scale)
    q = torch.tensor(c["q"].astype(F64), requires_grad=True)
    y = torch.tensor(r["td_targets"].astype(F64))
    w64 = torch.tensor((np.ones(B) if w is None else w.astype(F32)).astype(F64))
    e = q - y                                                    # zero outside the taken action's column
    per = (torch.nn.functional.huber_loss(q, y, reduction="none", delta=1.0) if huber else e * e).sum(1)
    loss = (w64 * per).mean()
    (float(F32(grad_scale)) * loss).backward()
    assert abs(loss.item() - r["loss_f64"]) <= 4 * B * 2.0 ** -53 * abs(loss.item())
    dq = q.grad.numpy()
    assert (np.abs(r["dq"].astype(F64) - dq) <= R.gamma(4) * np.abs(dq) + 4 * R.TINY).all()
    taken = np.zeros((B, A), dtype=bool)
    taken[np.arange(B), c["actions"]] = True
    assert not r["dq"][~taken].any() and not dq[~taken].any()
    assert abs(float(r["loss_f32"]) - r["loss_f64"]) <= r["loss_bound"]


@pytest.mark.parametrize("huber", [0, 1])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000, 1024])
def test_loss_f32_lies_inside_its_bound(B, huber):
    c = _batch(B, 4, B)
    r = R.dqn_head_loss(c["q"], c["q_next"], None, c["actions"], c["rewards"], c["dones"], c["weights"], 0.99, huber, 1.0)
    assert R.loss_threads(B) == {1: 64, 63: 64, 64: 64, 65: 128, 1000: 1024, 1024: 1024}[B]
    err = abs(float(r["loss_f32"]) - r["loss_f64"])
    print("MEASURED ref_loss_err_over_bound[B=%d,huber=%d] %.6g" % (B, huber, err / r["loss_bound"]))
    assert 0 < r["loss_bound"] < 1e-5 * r["loss_f64"]
    assert err <= r["loss_bound"]


def test_loss_tree_is_the_halving_tree_and_not_a_running_sum():
    """64 terms of which the tree pairs i with i + 32 first: 1e8 and -1e8 cancel exactly before the 1.0 is added; a sum in
    index order loses the 1.0"""
    terms = np.zeros(64, dtype=F32)
    terms[0], terms[1], terms[32] = 1e8, 1.0, -1e8
    assert R.loss_tree_f32(terms, 64) == F32(1.0) / F32(64)
    run = F32(0)
    for t in terms:
        run = F32(run + t)
    assert run == 0


# ------------------------------------------------------------------------------------------------ the NaN table

def _dqn(**poison):
    q = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], dtype=F32)
    c = dict(q=q, q_next=np.array([[1, 2, 3], [1, 2, 3], [3, 2, 1]], dtype=F32),
             q_sel=np.array([[1, 2, 3], [1, 2, 3], [3, 2, 1]], dtype=F32), rewards=np.ones(3, dtype=F32),
             weights=np.ones(3))
    for k, idx in poison.items():
        c[k] = c[k].copy()
        c[k][idx] = np.nan
    return c


def _dqn_targets_out(ddqn, **poison):
    c = _dqn(**poison)
    tt, err, _ = R.dqn_targets(c["q_next"], c["q_sel"] if ddqn else None, c["q"], [0, 2, 1], c["rewards"], [0, 0, 0], 0.5)
    return dict(td_targets=tt, td_errors=err)


def _head_loss_out(ddqn, huber, **poison):
    c = _dqn(**poison)
    r = R.dqn_head_loss(c["q"], c["q_next"], c["q_sel"] if ddqn else None, [0, 2, 1], c["rewards"], [0, 0, 0], c["weights"],
                        0.5, huber, 1.0)
    return dict(dq=r["dq"], td_errors=r["td_errors"], td_targets=r["td_targets"], loss=np.array([r["loss_f32"]]),
                loss_f64=np.array([r["loss_f64"]]))


def _ac_out(clip, **poison):
    c = dict(rewards=np.ones(3, dtype=F32), q_next=np.arange(6, dtype=F32).reshape(3, 2))
    for k, idx in poison.items():
        c[k][idx] = np.nan
    return dict(td_targets=R.ac_td_targets(c["rewards"], [0, 1, 0], c["q_next"], 2, 0.5, 0, clip))


def _merge_out(smooth, **poison):
    c = dict(actions=np.zeros((3, 2), dtype=F32), next_actions=np.zeros((3, 2), dtype=F32), noise=np.ones((3, 2)),
             obs=np.ones((3, 1), dtype=F32), next_obs=np.ones((3, 1), dtype=F32), low=-np.ones(2, dtype=F32),
             high=np.ones(2, dtype=F32))
    for k, idx in poison.items():
        c[k][idx] = np.nan
    m2, only = R.ac_merge_inputs(c["actions"], c["obs"], c["next_actions"], c["noise"] if smooth else None, 0.5, c["low"],
                                 c["high"], c["next_obs"])
    out = dict(online=m2[0], target=m2[1], obs_only=only)
    if smooth:
        out["smoothed"] = R.td3_smooth_actions(c["next_actions"], c["noise"], 0.5, c["low"], c["high"])
    return out


def _sac_out(**poison):
    c = dict(q_min=np.ones(3, dtype=F32), logprob=np.ones(3, dtype=F32))
    for k, idx in poison.items():
        c[k][idx] = np.nan
    return dict(value_targets=R.sac_value_targets(c["q_min"], c["logprob"]))


# (function, its fixed arguments, the poisoned input and the index of its NaN) -> {output: indices that become NaN}.
# Rows: actions [0, 2, 1]; row 1's selector is [1, 2, 3] (column 2 selected), row 2's is [3, 2, 1] (column 0).
NAN_TABLE = [
    # DQN: the target net selects.  A NaN mid-row wins the argmax, so the target is that NaN
    (_dqn_targets_out, (False,), ("q_next", (1, 1)), dict(td_targets=[(1, 2)], td_errors=[1])),
    (_dqn_targets_out, (False,), ("q_next", (2, 2)), dict(td_targets=[(2, 1)], td_errors=[2])),
    # DDQN: a NaN of the selector moves the column the target net is read at and nothing else
    (_dqn_targets_out, (True,), ("q_sel", (1, 1)), dict()),
    # DDQN: a NaN of the target net counts only in the selected column
    (_dqn_targets_out, (True,), ("q_next", (1, 1)), dict()),
    (_dqn_targets_out, (True,), ("q_next", (1, 2)), dict(td_targets=[(1, 2)], td_errors=[1])),
    (_dqn_targets_out, (True,), ("rewards", 0), dict(td_targets=[(0, 0)], td_errors=[0])),
    # Q_online at the taken action is replaced by the target: only the error sees it; elsewhere it is copied
    (_dqn_targets_out, (True,), ("q", (1, 2)), dict(td_errors=[1])),
    (_dqn_targets_out, (True,), ("q", (1, 0)), dict(td_targets=[(1, 0)])),
    (_head_loss_out, (False, 0), ("q_next", (1, 1)), dict(dq=[(1, 2)], td_errors=[1], td_targets=[(1, 2)], loss=[0], loss_f64=[0])),
    (_head_loss_out, (False, 1), ("q_next", (1, 1)), dict(dq=[(1, 2)], td_errors=[1], td_targets=[(1, 2)], loss=[0], loss_f64=[0])),
    (_head_loss_out, (True, 0), ("q_sel", (1, 1)), dict()),
    (_head_loss_out, (True, 0), ("q", (1, 2)), dict(dq=[(1, 2)], td_errors=[1], loss=[0], loss_f64=[0])),
    (_head_loss_out, (True, 0), ("q", (1, 0)), dict(td_targets=[(1, 0)])),
    (_head_loss_out, (True, 1), ("weights", 2), dict(dq=[(2, 1)], loss=[0], loss_f64=[0])),
    (_head_loss_out, (True, 1), ("rewards", 2), dict(dq=[(2, 1)], td_errors=[2], td_targets=[(2, 1)], loss=[0], loss_f64=[0])),
    (_ac_out, (None,), ("rewards", 1), dict(td_targets=[1])),
    (_ac_out, ((-3.0, 3.0),), ("rewards", 1), dict(td_targets=[1])),          # np.clip keeps it
    (_ac_out, ((-3.0, 3.0),), ("q_next", (0, 0)), dict(td_targets=[0])),
    (_ac_out, ((-3.0, 3.0),), ("q_next", (1, 0)), dict(td_targets=[1])),      # done: 0 * NaN is NaN
    (_ac_out, ((-3.0, 3.0),), ("q_next", (0, 1)), dict()),                    # a column q_stride skips
    (_merge_out, (True,), ("noise", (1, 0)), dict(target=[(1, 0)], smoothed=[(1, 0)])),
    (_merge_out, (True,), ("next_actions", (2, 1)), dict(target=[(2, 1)], smoothed=[(2, 1)])),
    (_merge_out, (True,), ("actions", (0, 0)), dict(online=[(0, 0)])),
    (_merge_out, (True,), ("obs", (0, 0)), dict(online=[(0, 2)], obs_only=[(0, 0)])),
    (_merge_out, (True,), ("next_obs", (0, 0)), dict(target=[(0, 2)])),
    (_merge_out, (False,), ("next_actions", (2, 1)), dict(target=[(2, 1)])),
    (_merge_out, (False,), ("low", 0), dict()),                               # DDPG: the bounds are not looked at
    (_merge_out, (False,), ("high", 1), dict()),
    (_sac_out, (), ("q_min", 1), dict(value_targets=[1])),
    (_sac_out, (), ("logprob", 2), dict(value_targets=[2])),
]


@pytest.mark.parametrize("row", range(len(NAN_TABLE)))
def test_nan_table(row):
    fn, fixed, (name, idx), reaches = NAN_TABLE[row]
    clean, dirty = fn(*fixed), fn(*fixed, **{name: idx})
    assert sorted(clean) == sorted(dirty)
    for out in clean:
        assert not np.isnan(clean[out]).any(), out
        want = np.zeros(clean[out].shape, dtype=bool)
        for i in reaches.get(out, []):
            want[i] = True
        assert np.array_equal(np.isnan(dirty[out]), want), (fn.__name__, name, idx, out, dirty[out])
        assert same_bits(dirty[out][~want], clean[out][~want]) or name == "q_sel", out
    if name == "q_sel" and fn is _dqn_targets_out:
        # the target is finite, but read at the NaN's column: r + 0.5 * q_next[1][1] and not r + 0.5 * q_next[1][2]
        assert dirty["td_targets"][1, 2] == 1 + 0.5 * 2 and clean["td_targets"][1, 2] == 1 + 0.5 * 3


def test_first_nan_and_first_maximum_win_the_selection():
    for row, col in (([1, np.nan, 3], 1), ([np.nan, 3, np.nan], 0), ([2, 2, 1], 0), ([0.0, -0.0, 0.0], 0),
                     ([-0.0, 0.0, -1], 0), ([1, 2, 2], 1), ([3, np.inf, np.inf], 1)):
        q_next = np.array([[10, 20, 30]], dtype=F32)
        tt, _, _ = R.dqn_targets(q_next, np.array([row], dtype=F32), np.zeros((1, 3), dtype=F32), [0], [0.0], [0], 1.0)
        assert tt[0, 0] == q_next[0, col], (row, col)


# ------------------------------------------------------------------------------------------------ the backward bounds

@pytest.mark.parametrize("lower", [0, 1, 2])
def test_head_backward_bounds_hold_for_a_plain_fp32_evaluation(lower):
    """an fp32 evaluation in index order (numpy, no FMA) lies inside the order-independent bounds, and the bounds are
    tight enough to tell a wrong value: a few units of roundoff times the magnitude of the sum"""
    rng = np.random.RandomState(lower)
    B, K, N = 65, 17, 5
    x = np.tanh(rng.randn(B, K)).astype(F32) if lower == 2 else np.maximum(rng.randn(B, K), 0).astype(F32)
    w = rng.randn(K, N).astype(F32)
    dq = np.zeros((B, N), dtype=F32)
    dq[np.arange(B), rng.randint(0, N, size=B)] = rng.randn(B).astype(F32)
    r = R.head_backward(x, w, dq, lower)
    dw = np.zeros((K, N), dtype=F32)
    db = np.zeros(N, dtype=F32)
    for b in range(B):
        dw = dw + x[b][:, None] * dq[b][None, :]
        db = db + dq[b]
    f = {0: np.ones_like(x), 1: (x > 0).astype(F32), 2: F32(1) - x * x}[lower]
    dx = (dq @ w.T).astype(F32) * f
    for got, key in ((dw, "dw"), (db, "db"), (dx, "dx")):
        ok, ratio = R.within(got, r[key], r[key + "_bound"])
        assert ok, (key, ratio)
        assert (r[key + "_bound"] <= 1e-5 * (np.abs(r[key]).max() + 1)).all(), key
    wrong = dx.copy()
    wrong[3, 4] = wrong[3, 4] * F32(1 + 2.0 ** -18) + F32(1e-6)
    assert not R.within(wrong, r["dx"], r["dx_bound"])[0]
