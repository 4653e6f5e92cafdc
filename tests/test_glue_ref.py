"""tests/glue_ref.py validated on the CPU: against torch.autograd in float64, against torch.nn.utils.clip_grad_norm_ and
closed forms, and against the project's fp32 oracle (oracle/ac_nets.py, which glue_ref.py does not import) -- plus the
conditions that the inputs and the tolerances of tests/test_glue_kernels.py must satisfy before any kernel runs."""
import numpy as np
import pytest

import glue_ref as R
from test_glue_kernels import (CATEGORY_SHAPE_MIN_B, SAC_BWD_C, SAC_LOGP_C_G, SAC_LOGP_C_T, SAC_SHAPES, assert_categories,
                               logp_bound)

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24


def test_clamp_and_minimum_gradients_are_inclusive_at_the_bounds():
    """torch.clamp passes the gradient at x == lo and x == hi, as TF's minimum(maximum(x, lo), hi) does (maximum gives
    the gradient to x where x >= lo, minimum where x <= hi): confirmed here, not assumed, because the SAC head's
    backward test below leans on it."""
    import torch
    x = torch.tensor([-20.5, -20.0, 0.0, 2.0, 2.5], dtype=torch.float64, requires_grad=True)
    torch.clamp(x, -20, 2).sum().backward()
    assert x.grad.tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]
    y = torch.tensor([-20.5, -20.0, 0.0, 2.0, 2.5], dtype=torch.float64, requires_grad=True)
    lo, hi = torch.tensor(-20.0, dtype=torch.float64), torch.tensor(2.0, dtype=torch.float64)
    m = torch.maximum(y, lo)
    # torch splits the gradient of maximum / minimum on a tie (0.5 each); TF does not -- which is why the reference is
    # compared with clamp, whose rule is TF's
    torch.minimum(m, hi).sum().backward()
    assert y.grad.tolist() == [0.0, 0.5, 1.0, 0.5, 0.0]


@pytest.mark.parametrize("B,A", SAC_SHAPES)
def test_sac_head_case_holds_every_category(B, A):
    """the shares (a)-(f) for every shape of the GPU tests with at least CATEGORY_SHAPE_MIN_B rows, both paddings"""
    for pad in (0, 5):
        x, normals, plain = R.sac_head_case(np.random.RandomState(B * 1000 + A * 10 + pad), B, A, 2 * A + pad)
        fwd = R.sac_head_forward(x, normals, A)
        assert_categories(fwd, B)
        if B >= CATEGORY_SHAPE_MIN_B:
            assert plain.sum() == B // 8 >= 7
            assert not (fwd["below"] | fwd["above"] | fwd["on_bound"])[plain].any()
            assert np.abs(fwd["raw"][plain]).max() <= 1 + 1e-5
        assert np.all(x[:, 2 * A:] == F32(7e4))


@pytest.mark.parametrize("B,A", SAC_SHAPES)
def test_logp_bound_is_tight_on_plain_rows(B, A):
    """On rows made only of interior log-std and unsaturated samples the per-row bound of test_sac_policy_head, with the
    constants it records, stays below 1e-5 max(1, |logp|): it cannot silently become vacuous."""
    x, normals, plain = R.sac_head_case(np.random.RandomState(B * 1000 + A * 10), B, A, plain_rows=B)
    fwd = R.sac_head_forward(x, normals, A, raw=R.sac_head_forward(x, normals, A)["raw"].astype(F32))
    bound = logp_bound(fwd, SAC_LOGP_C_T, SAC_LOGP_C_G)
    assert np.all(bound < 1e-5 * np.maximum(1.0, np.abs(fwd["logp"]))), (bound / np.maximum(1.0, np.abs(fwd["logp"]))).max()


def test_backward_bound_is_tight_on_plain_rows():
    """the same for the backward pass: on plain rows the per-element bound is a few 1e-6 of the gradient's scale."""
    B, A = 64, 6
    x, normals, _ = R.sac_head_case(np.random.RandomState(1), B, A, plain_rows=B)
    aw = np.random.RandomState(2).randn(B, A).astype(F32)
    ref = R.sac_head_backward(x, normals, A, 1.0, aw, -1.0)
    scale = 1.0 / B + np.abs(aw)
    assert np.all(SAC_BWD_C * U24 * ref["mu_unit"] < 2e-5 * scale)


@pytest.mark.parametrize("lw,with_aw", [(0.0, False), (0.0, True), (1.0, False), (1.0, True)])
def test_sac_head_backward_matches_autograd(lw, with_aw):
    """float64 autograd through clamp -> exp -> reparameterised sample -> tanh -> Normal.log_prob - log(1 - t^2 + eps), on
    inputs where 20% of the log-std entries lie below -20, 20% above 2 and 10% exactly on each bound (asserted), for
    the four combinations of logp_weight and action_weights.  Autograd's own float64 noise sets the absolute terms: it
    takes 1 - tanh^2 by subtraction (a few 1e-16 there are a few 1e-9 of the squash gradient once divided by eps), and
    it sends the Gaussian term's gradient down two paths, +-z / sd each, that cancel only to 1e-16 z / sd (sd = 2e-9
    where log_std is clipped at -20)."""
    import torch
    B, A = 64, 5
    rng = np.random.RandomState(11)
    x, normals, _ = R.sac_head_case(rng, B, A, plain_rows=0)
    aw = rng.randn(B, A).astype(F32) if with_aw else None
    ref = R.sac_head_backward(x, normals, A, lw, aw, -0.75)
    fwd = R.sac_head_forward(x, normals, A)
    for k, share in (("below", 0.2), ("above", 0.2)):
        assert abs(ref[k].mean() - share) < 0.01
    assert abs((x[:, A:] == F32(-20)).mean() - 0.1) < 0.01 and abs((x[:, A:] == F32(2)).mean() - 0.1) < 0.01
    xt = torch.tensor(x.astype(F64), requires_grad=True)
    mu, ls = xt[:, :A], torch.clamp(xt[:, A:], -20, 2)
    raw = mu + torch.exp(ls) * torch.tensor(normals.astype(F32).astype(F64))
    act = torch.tanh(raw)
    logp = torch.distributions.Normal(mu, torch.exp(ls)).log_prob(raw).sum(1) - torch.log(1 - act ** 2 + R.EPS32).sum(1)
    np.testing.assert_allclose(fwd["logp"], logp.detach().numpy(), rtol=1e-9, atol=1e-7)
    np.testing.assert_allclose(fwd["act"], act.detach().numpy(), rtol=1e-15, atol=0)
    obj = lw * logp.mean()
    if with_aw:
        obj = obj + -0.75 * (act * torch.tensor(aw.astype(F64))).sum()
    if not (lw or with_aw):
        assert not ref["d_mu"].any() and not ref["d_ls"].any()
        return
    obj.backward()
    g = xt.grad.numpy()
    scale = lw / B + (np.abs(aw).max() if with_aw else 0.0)
    noise = 1e-8 * scale + 1e-15 * (lw / B) * np.abs(fwd["z"]) / np.exp(fwd["log_std"])
    assert np.all(np.abs(ref["d_mu"] - g[:, :A]) <= 1e-9 * np.abs(g[:, :A]) + noise)
    assert np.all(np.abs(ref["d_ls"] - g[:, A:]) <= 1e-9 * np.abs(g[:, A:]) + noise * (1 + np.exp(2) * np.abs(normals)))
    clipped = ref["below"] | ref["above"]
    assert not g[:, A:][clipped].any() and not ref["d_ls"][clipped].any()
    if lw:
        assert np.all(g[:, A:][ref["on_bound"]] != 0) and np.all(ref["d_ls"][ref["on_bound"]] != 0)


@pytest.mark.parametrize("B,A", [(1, 1), (7, 2), (64, 6), (65, 51)])
def test_dueling_combine_matches_autograd(B, A):
    import torch
    rng = np.random.RandomState(B + A)
    v, adv, dq = rng.randn(B).astype(F32), (rng.randn(B, A) + 1e4).astype(F32), rng.randn(B, A).astype(F32)
    vt = torch.tensor(v.astype(F64), requires_grad=True)
    at = torch.tensor(adv.astype(F64), requires_grad=True)
    q = vt[:, None] + (at - at.mean(1, keepdim=True))
    q.backward(torch.tensor(dq.astype(F64)))
    np.testing.assert_allclose(R.dueling_combine(v, adv), q.detach().numpy(), rtol=1e-14, atol=1e-12)
    dv, dadv = R.dueling_combine_backward(dq)
    np.testing.assert_allclose(dv, vt.grad.numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(dadv, at.grad.numpy(), rtol=1e-13, atol=1e-15)
    # the fp32 restatements stay within the bound the GPU test asserts for the kernel
    err = np.abs(R.dueling_combine_f32(v, adv).astype(F64) - R.dueling_combine(v, adv))
    assert np.all(err <= A * U24 * (np.abs(v.astype(F64)) + np.abs(adv.astype(F64)).sum(1))[:, None])
    s32, d32 = R.dueling_combine_backward_f32(dq)
    bound = A * U24 * np.abs(dq.astype(F64)).sum(1)
    assert np.all(np.abs(s32 - dv) <= bound) and np.all(np.abs(d32 - dadv) <= bound[:, None])


def test_clip_by_global_norm_matches_torch_above_the_clip_value():
    """torch scales by max_norm / (norm + 1e-6): comparable only where norm > clip, and then up to 1e-6 / norm."""
    import torch
    rng = np.random.RandomState(4)
    g = rng.randn(1000).astype(F32)
    norm = R.global_norm(g)
    assert abs(norm - np.sqrt(np.sum(g.astype(F64) ** 2))) == 0
    for clip in (0.5, 10.0, norm / 1.7):
        p = torch.nn.Parameter(torch.zeros(1000, dtype=torch.float64))
        p.grad = torch.tensor(g.astype(F64))
        total = torch.nn.utils.clip_grad_norm_([p], float(F32(clip)))
        np.testing.assert_allclose(float(total), norm, rtol=1e-14)
        ref = R.clip_by_global_norm(g, F32(norm), clip)
        np.testing.assert_allclose(ref, p.grad.numpy(), rtol=1e-6 / norm + 2 * U24, atol=0)     # + float32(norm)
        np.testing.assert_allclose(R.global_norm(ref.astype(F32)), float(F32(clip)), rtol=4 * U24)
        np.testing.assert_allclose(R.clip_by_global_norm_f32(g, F32(norm), F32(clip)), ref, rtol=4 * U24, atol=0)


def test_clip_by_global_norm_closed_forms():
    """norm < clip: the scale is clip * (1 / clip) = 1; norm 0: 1 / 0 = inf loses the min, scale 1, zeros stay zeros;
    NaN norm: every entry NaN (TF's minimum keeps a NaN first argument -- and so does Python's min in
    oracle/agents.py:207, evaluated here); infinite norm: scale 0."""
    g = np.random.RandomState(5).randn(100).astype(F32)
    for clip in (40.0, 10.0, 0.5, 1024.0):
        assert F32(clip) * (F32(1) / F32(clip)) == F32(1)
    assert np.array_equal(R.clip_by_global_norm(g, F32(9.5), 40.0), g.astype(F64))
    assert np.array_equal(R.clip_by_global_norm_f32(g, F32(9.5), F32(40.0)), g)
    z = R.clip_by_global_norm_f32(np.zeros(5, dtype=F32), F32(0), F32(40.0))
    assert np.array_equal(z, np.zeros(5, dtype=F32)) and not np.signbit(z).any()
    assert np.array_equal(R.clip_by_global_norm(np.zeros(5, dtype=F32), F32(0), 40.0), np.zeros(5))
    assert np.isnan(R.clip_by_global_norm(g, F32("nan"), 40.0)).all()
    assert np.isnan(R.clip_by_global_norm_f32(g, F32("nan"), F32(40.0))).all()
    c = F32(40.0)
    with np.errstate(all="ignore"):
        assert np.isnan(c * min(F32(1.0) / F32("nan"), F32(1.0) / c))                # oracle/agents.py:207's expression
        assert c * min(F32(1.0) / F32("inf"), F32(1.0) / c) == 0
    assert np.array_equal(R.clip_by_global_norm(g, F32("inf"), 40.0), g.astype(F64) * 0.0)


def test_small_references():
    """the one-line references against their definitions"""
    rng = np.random.RandomState(6)
    x, y = rng.randn(50).astype(F32), rng.randn(50).astype(F32)
    ref, mag = R.axpby(0.37, x, -1.25, y)
    np.testing.assert_allclose(ref, F64(F32(0.37)) * x - 1.25 * y.astype(F64), rtol=1e-15)
    assert np.array_equal(R.axpby(0.37, x, 1.0, None)[0], F64(F32(0.37)) * x)
    assert np.array_equal(R.copy_2d(x, -1.0), -x.astype(F64))
    m, g1, g2 = R.min_pair(x, y, 0.25)
    assert np.array_equal(m, np.minimum(x, y)) and np.array_equal(g1 + g2, np.full(50, 0.25, dtype=F32))
    m, g1, g2 = R.min_pair(np.array([0.0, -0.0, 1.0], dtype=F32), np.array([-0.0, 0.0, 1.0], dtype=F32), 1.0)
    assert np.signbit(m).tolist() == [False, True, False] and g1.tolist() == [1, 1, 1] and g2.tolist() == [0, 0, 0]
    nan = F32("nan")                       # a NaN of one side or of both is the minimum, as in np.minimum
    m, g1, g2 = R.min_pair(np.array([nan, 1.0, nan], dtype=F32), np.array([1.0, nan, nan], dtype=F32), 1.0)
    assert np.isnan(m).all() and np.isnan(np.minimum(nan, F32(1.0))) and np.isnan(np.minimum(F32(1.0), nan))
    assert g1.tolist() == [1, 0, 1] and g2.tolist() == [0, 1, 0]
    dy =rng.randn(6).astype(F32)
    yy = np.array([0.0, -0.0, 1e-40, -1e-40, 1.0, -1.0], dtype=F32)
    assert R.act_backward(dy, yy, "relu").tolist() == [0, 0, float(dy[2]), 0, float(dy[4]), 0]
    assert R.act_backward(dy, yy, "tanh")[4:].tolist() == [0, 0]
    assert np.array_equal(R.act_backward(dy, yy, "none"), dy.astype(F64))
    assert R.exp_rows(np.array([0.0, 1.0], dtype=F32), 3).shape == (3, 2)
    assert R.ulp_distance(F32(1) + np.finfo(F32).eps, 1.0) == 1.0


def _head_only_oracle(x):
    """SACPolicyOracle whose dense output is exactly x [B, 2A]: a one-hot input per row, the rows of x as the kernel, no
    bias -- and whose kernel gradient is then exactly the head's d_mu_logsig."""
    from oracle import ac_nets as O
    B = x.shape[0]
    hn = "policy/sac_policy_head/policy_mu_logsig"
    pol = O.SACPolicyOracle({hn + "/kernel": [x.copy()], hn + "/bias": [np.zeros(x.shape[1], dtype=F32)]})
    return pol, np.eye(B, dtype=F32), hn + "/kernel"


@pytest.mark.parametrize("lw,with_aw", [(1.0, False), (0.0, True), (1.0, True)])
def test_reference_agrees_with_the_project_oracle(lw, with_aw):
    """At ordinary inputs (plain rows only) SACPolicyOracle.forward / .backward, fp32 numpy, agree with the float64
    reference to the round-off of the oracle's own arithmetic.  Bounds, u = 2^-24 per fp32 rounding:
      raw    exp (<= 2u), product, sum: <= 4u (|mu| + |sd e|)
      logp   evaluated at the oracle's own fp32 raw.  Squash term per element: tanh (<= 4u |t|), t t, 1 - t^2, + eps
             (<= u each on values <= 1) give du <= (8 t^2 + 3) u <= 4 (2|t| + 1) u, the log 2u more, each divided by
             1 - t^2 + eps: <= 6u (2|t| + 1) cond.  Gaussian term per element: raw - mu, / sd, sd itself (<= 4u on z,
             8u on z^2), the products and the two subtractions (<= 4u): <= 12u (z^2 / 2 + |ls| + 0.92).  The two row sums
             add at most A u of sum |terms| each.  Together <= u [6 logp_t_unit + (12 + 2A) logp_g_unit].
      grads  16 u unit: the error model of glue_ref.sac_head_backward counts one rounding per intermediate and two for
             the sample; the oracle spends up to four on tanh, four on the sample, and eight more across the products,
             the quotient and the sum."""
    B, A = 48, 6
    rng = np.random.RandomState(21)
    x, normals, _ = R.sac_head_case(rng, B, A, plain_rows=B)
    aw = rng.randn(B, A).astype(F32) if with_aw else None
    pol, eye, kernel = _head_only_oracle(x)
    o = pol.forward(eye, normals)
    fwd = R.sac_head_forward(x, normals, A)
    assert np.array_equal(o["mean"], x[:, :A]) and np.array_equal(o["log_std"], fwd["log_std"].astype(F32))
    assert np.all(np.abs(o["raw_actions"] - fwd["raw"]) <= 4 * U24 * fwd["raw_mag"])
    at = R.sac_head_forward(x, normals, A, raw=o["raw_actions"])
    assert np.all(R.ulp_distance(o["actions"], at["act"]) <= 2)
    bound = U24 * (6 * at["logp_t_unit"] + (12 + 2 * A) * at["logp_g_unit"])
    assert np.all(np.abs(o["logprob"] - at["logp"]) <= bound), (np.abs(o["logprob"] - at["logp"]) / bound).max()
    assert np.all(bound < 1e-4 * np.maximum(1, np.abs(at["logp"])))          # ... which is a tight statement here
    pol.backward(logp_weight=lw, action_weights=aw, action_weight_scale=-1.0)
    d = pol.grads()[kernel][0]
    ref = R.sac_head_backward(x, normals, A, lw, aw, -1.0)
    for got, want, unit in ((d[:, :A], ref["d_mu"], ref["mu_unit"]), (d[:, A:], ref["d_ls"], ref["ls_unit"])):
        assert np.all(np.abs(got - want) <= 16 * U24 * unit), (np.abs(got - want) / (16 * U24 * unit)).max()


def test_reference_and_oracle_agree_on_the_clip_mask():
    """beyond ordinary inputs only the exact statements are compared: where the oracle zeroes d_ls, so does the
    reference, boundaries included."""
    B, A = 64, 5
    x, normals, _ = R.sac_head_case(np.random.RandomState(31), B, A, plain_rows=0)
    pol, eye, kernel = _head_only_oracle(x)
    pol.forward(eye, normals)
    with np.errstate(all="ignore"):
        pol.backward(logp_weight=1.0)
    d = pol.grads()[kernel][0]
    ref = R.sac_head_backward(x, normals, A, 1.0)
    assert np.array_equal(d[:, A:] == 0, ref["d_ls"] == 0)
    assert np.array_equal(ref["d_ls"] == 0, ref["below"] | ref["above"])
    assert SAC_BWD_C >= 1 and CATEGORY_SHAPE_MIN_B >= 1
