"""tests/head_loss_ref.py validated on the CPU: against torch.autograd and torch.distributions in float64, against the
project's fp32 oracle (oracle/losses.py, which head_loss_ref.py does not import), against the reference's MXNet known
answer -- plus the properties its case generators promise, which tests/test_loss_kernels.py relies on before any kernel
runs."""
import numpy as np
import pytest

import head_loss_ref as R

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24
SHAPES = [(1, 1), (1, 6), (6, 2), (63, 2), (65, 6), (64, 18), (1024, 1), (1025, 6), (2049, 2)]


def _t(x, grad=False):
    import torch
    return torch.tensor(np.asarray(x, dtype=F32).astype(F64), requires_grad=grad)


# ------------------------------------------------------------------------------------------------ generators
@pytest.mark.parametrize("B,n", SHAPES)
@pytest.mark.parametrize("pad", [0, 5])
def test_ppo_discrete_case_properties(B, n, pad):
    c = R.ppo_discrete_case(np.random.RandomState(B * 100 + n + pad), B, n, 0.2, n + pad, n + pad)
    r = R.ppo_discrete_loss(c["logits"][:, :n], c["actions"], c["advantages"], c["old_probs"][:, :n], 0.2, 0.01)
    _check_case(r, c, B, n >= 2)
    assert np.all(c["old_probs"][:, :n] > 0) and np.all(np.isfinite(c["logits"][:, :n]))
    assert np.all(np.isnan(c["logits"][:, n:])) and np.all(np.isnan(c["old_probs"][:, n:]))
    assert c["logits"].shape == (B, n + pad) and c["actions"].dtype == np.int32
    if B >= 3:
        s = c["old_probs"][:, :n].astype(F64).sum(axis=1)
        assert (np.abs(s - 1) > 0.01).any() and (np.abs(s - 1) < 1e-5).any()       # un-normalised and normalised rows
    if n == 1:
        assert np.all(r["ratio"] == 1.0)


@pytest.mark.parametrize("B,A", [(1, 1), (1, 6), (6, 2), (65, 1), (65, 18), (1024, 2), (1024, 6)])
@pytest.mark.parametrize("pad", [0, 5])
def test_ppo_continuous_case_properties(B, A, pad):
    c = R.ppo_continuous_case(np.random.RandomState(B * 100 + A + pad), B, A, 0.2, A + pad, A + pad)
    r = R.ppo_continuous_loss(c["mean"][:, :A], c["log_std"], c["actions"], c["advantages"], c["old_mean"][:, :A],
                              c["old_std"][:, :A], 0.2, 0.01)
    _check_case(r, c, B, True)
    assert np.all(c["old_std"][:, :A] > 0)
    assert np.all(np.isnan(c["mean"][:, A:])) and np.all(np.isnan(c["old_mean"][:, A:])) and np.all(np.isnan(c["old_std"][:, A:]))


def _check_case(r, c, B, can_leave_band):
    lo, hi, adv = r["lo"], r["hi"], c["advantages"].astype(F64)
    assert np.all(np.abs(r["ratio"] - lo) >= R.CLIP_MARGIN * lo) and np.all(np.abs(r["ratio"] - hi) >= R.CLIP_MARGIN * hi)
    assert np.all(np.abs(adv) >= 0.1)
    kinds = R.quadrant_of(r["ratio"], adv, lo, hi)
    if can_leave_band:
        assert np.array_equal(kinds, c["kinds"])
        if B >= R.MIN_QUADRANT_ROWS:
            for k in R.QUADRANTS:
                assert (kinds == k).sum() >= max(1, B // 16), k
    else:
        assert set(kinds) <= {"in_pos", "in_neg"}
    # the routing the four quadrants stand for
    want = {"hi_pos": False, "hi_neg": True, "lo_pos": True, "lo_neg": False, "in_pos": True, "in_neg": True}
    assert np.array_equal(r["passes"], np.array([want[k] for k in kinds]))
    # the margin is wide against the counted error of the ratio: no row can change sides on the device
    assert np.all(U24 * r["ratio_units"] < 0.5 * R.CLIP_MARGIN * r["ratio"])


@pytest.mark.parametrize("B,D", [(1, 1), (1, 18), (3, 2), (63, 6), (1025, 1)])
def test_huber_case_holds_the_edges(B, D):
    out, target, w = R.huber_case(np.random.RandomState(B + D), B, D, D + 5, D + 5)
    e = (out[:, :D] - target[:, :D]).reshape(-1)                      # the fp32 subtraction of the kernel
    k = min(B * D, 7)
    assert np.array_equal(e[:k], np.array(R.HUBER_EDGES[:k], dtype=F32))
    assert sorted(float(v) for v in R.HUBER_EDGES) == [-1 - 2.0 ** -23, -1.0, -1 + 2.0 ** -24, 0.0, 1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -23]
    assert np.all(np.isnan(out[:, D:])) and np.all(np.isnan(target[:, D:])) and np.all(w > 0)
    r = R.regression_loss(out[:, :D], target[:, :D], w, "huber")
    ee = e[:k].astype(F64)
    assert np.array_equal(r["grad"].reshape(-1)[:k] * B / np.repeat(w.astype(F64), D)[:k], np.clip(ee, -1, 1))


# ------------------------------------------------------------------------------------------------ autograd, float64
@pytest.mark.parametrize("kind", ["mse", "huber"])
@pytest.mark.parametrize("weighted", [False, True])
def test_regression_loss_matches_autograd(kind, weighted):
    import torch
    out, target, w = R.huber_case(np.random.RandomState(3), 37, 5)
    # autograd's huber derivative at exactly |e| = 1 is 1 from both sides, as the clip's
    r = R.regression_loss(out, target, w if weighted else None, kind, 0.5, 0.75)
    o = _t(out, True)
    l = (o - _t(target)) ** 2 if kind == "mse" else torch.nn.functional.huber_loss(o, _t(target), reduction="none", delta=1.0)
    loss = (F64(F32(0.5)) * (_t(w) if weighted else 1.0) * l.sum(1)).mean()
    (0.75 * loss).backward()
    np.testing.assert_allclose(r["loss"], loss.item(), rtol=1e-13)
    np.testing.assert_allclose(r["grad"], o.grad.numpy(), rtol=1e-12, atol=1e-300)
    assert np.all(r["grad_units"] == 5 * np.abs(r["grad"])) and r["loss_units"] > 0


@pytest.mark.parametrize("B,n", [(6, 2), (65, 6), (64, 18), (7, 1)])
def test_ppo_discrete_loss_matches_autograd(B, n):
    import torch
    c = R.ppo_discrete_case(np.random.RandomState(B + n), B, n, 0.2)
    beta, gs = 0.05, 0.5
    r = R.ppo_discrete_loss(c["logits"], c["actions"], c["advantages"], c["old_probs"], 0.4, beta, 0.5, gs)
    z = _t(c["logits"], True)
    new = torch.distributions.Categorical(probs=torch.softmax(z, 1))
    old = torch.distributions.Categorical(probs=_t(c["old_probs"]))
    a, adv = torch.tensor(c["actions"].astype(np.int64)), _t(c["advantages"])
    ratio = torch.exp(new.log_prob(a) - old.log_prob(a))
    ce = float(F64(F32(0.4)) * F64(F32(0.5)))
    clipped = torch.clamp(ratio, 1 - ce, 1 + ce)
    sur = -torch.minimum(ratio * adv, clipped * adv).mean()
    ent = new.entropy().mean()
    kl = torch.distributions.kl_divergence(old, new).mean()
    total = sur - float(F32(beta)) * ent
    (gs * total).backward()
    np.testing.assert_allclose(r["ratio"], ratio.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(r["clipped"], clipped.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(r["scalars"], [sur.item(), ent.item(), kl.item(), total.item()], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(r["dlogits"], z.grad.numpy(), rtol=1e-9, atol=1e-14)
    if n >= 2:
        blocked = ~r["passes"]
        assert blocked.sum() >= 2              # rows whose surrogate gradient is cut: only the entropy term is left


@pytest.mark.parametrize("B,A", [(6, 1), (65, 2), (64, 6), (33, 18)])
def test_ppo_continuous_loss_matches_autograd(B, A):
    import torch
    c = R.ppo_continuous_case(np.random.RandomState(B + A), B, A, 0.2)
    beta, gs = 0.05, 0.5
    r = R.ppo_continuous_loss(c["mean"], c["log_std"], c["actions"], c["advantages"], c["old_mean"], c["old_std"], 0.4,
                              beta, 0.5, gs)
    mu, ls = _t(c["mean"], True), _t(c["log_std"], True)
    new = torch.distributions.Normal(mu, torch.exp(ls) + R.EPS32)
    old = torch.distributions.Normal(_t(c["old_mean"]), _t(c["old_std"]) + R.EPS32)
    x, adv = _t(c["actions"]), _t(c["advantages"])
    ratio = torch.exp(new.log_prob(x).sum(1) - old.log_prob(x).sum(1))
    ce = float(F64(F32(0.4)) * F64(F32(0.5)))
    clipped = torch.clamp(ratio, 1 - ce, 1 + ce)
    sur = -torch.minimum(ratio * adv, clipped * adv).mean()
    ent = (torch.distributions.Normal(torch.zeros(A, dtype=torch.float64), torch.exp(ls) + R.EPS32)).entropy().sum()
    kl = torch.distributions.kl_divergence(old, new).sum(1).mean()
    total = sur - float(F32(beta)) * ent
    (gs * total).backward()
    np.testing.assert_allclose(r["ratio"], ratio.detach().numpy(), rtol=1e-11)
    np.testing.assert_allclose(r["scalars"], [sur.item(), ent.item(), kl.item(), total.item()], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(r["dmean"], mu.grad.numpy(), rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(r["dlog_std"], ls.grad.numpy(), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("twin,clip,nonzero,T", [(False, None, False, 1), (True, (-1.5, 1.5), False, 2),
                                                (True, None, True, 4), (False, (-1.5, 1.5), True, 3)])
def test_ac_critic_losses_matches_autograd(twin, clip, nonzero, T):
    import torch
    rng = np.random.RandomState(T)
    B = 65
    q1, q2, rew = rng.randn(B).astype(F32), rng.randn(B).astype(F32), rng.randn(B).astype(F32)
    done = (rng.rand(B) < 0.3).astype(np.uint8)
    q = rng.randn(T, B).astype(F32)
    r = R.ac_critic_losses(q1, q2 if twin else None, rew, done, 0.99, q, 0.5, clip, nonzero)
    qn = np.minimum(q1, q2) if twin else q1
    assert np.array_equal(r["q_min"], qn)
    # the reference's own two statements (ddpg_agent.py:157 / :159-160) on its operand types: float64 rewards and game_overs,
    # a python float discount, the fp32 network output -- numpy makes the first product fp32 and the second float64
    y = rew.astype(F64) + 0.99 * qn if nonzero else rew.astype(F64) + (1.0 - done.astype(F64)) * 0.99 * qn
    y = y if clip is None else np.clip(y, *clip)
    np.testing.assert_allclose(r["y"], y, rtol=1e-15)
    if clip is not None:
        assert (r["y"] == clip[0]).any() and (r["y"] == clip[1]).any()
    qt = _t(q, True)
    losses = 0.5 * ((qt - _t(y.astype(F32))) ** 2).mean(1)
    losses.sum().backward()
    np.testing.assert_allclose(r["loss"], losses.detach().numpy(), rtol=1e-13)
    np.testing.assert_allclose(r["total"], losses.sum().item(), rtol=1e-13)
    np.testing.assert_allclose(r["dq"], qt.grad.numpy(), rtol=1e-13)
    other = R.ac_critic_losses(q1, None, rew, done, 0.99, q, 0.5, None, nonzero, td_targets=np.zeros(B, dtype=F32))
    np.testing.assert_allclose(other["loss"], 0.5 * (q.astype(F64) ** 2).mean(1), rtol=1e-13)


def test_softmax_edges():
    import torch
    z = np.array([[0, 0, 0, 0], [1e4, -1e4, 3, 1e4], [80, -80, 0, 79], [-np.inf, 2, -np.inf, 1], [5, 5, 5, 5]], dtype=F32)
    p, units = R.softmax(z)
    assert np.all(np.isfinite(p)) and np.all(np.isfinite(units)) and np.all(units > 0)
    np.testing.assert_allclose(p.sum(1), 1, rtol=1e-15)
    np.testing.assert_allclose(p, torch.softmax(torch.tensor(z.astype(F64)), 1).numpy(), rtol=1e-14, atol=1e-300)
    assert p[3, 0] == 0 and p[1, 1] == 0 and np.all(p[0] == 0.25)
    assert np.all(units[0] == 0.25 * (2 * R.EXPF + 4))                       # no exponent error on an all-equal row
    assert R.softmax(np.array([[3.0]], dtype=F32))[0][0, 0] == 1.0


# ------------------------------------------------------------------------------------------------ the fp32 oracle
def test_reference_agrees_with_the_project_oracle():
    """oracle/losses.py evaluates the same formulas in numpy fp32, in its own order: agreement to fp32 round-off --
    a few 1e-6 relative, with an absolute floor for sums that cancel (KL, the gradients)."""
    from oracle import losses as L
    from oracle import nn as N
    rng = np.random.RandomState(12)
    for B, n in ((64, 6), (6, 2), (100, 18)):
        c = R.ppo_discrete_case(rng, B, n, 0.2)
        r = R.ppo_discrete_loss(c["logits"], c["actions"], c["advantages"], c["old_probs"], 0.2, 0.01)
        o = L.ppo_discrete_loss(c["logits"], c["actions"], c["advantages"], c["old_probs"], 0.2, 0.01)
        np.testing.assert_allclose([o["surrogate"], o["entropy"], o["kl"], o["total"]], r["scalars"], rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(o["ratio"], r["ratio"], rtol=2e-5)
        np.testing.assert_allclose(o["clipped"], r["clipped"], rtol=2e-5)
        np.testing.assert_allclose(o["dlogits"], r["dlogits"], rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(N.softmax(c["logits"]), R.softmax(c["logits"])[0], rtol=1e-5, atol=1e-8)
    for B, A in ((64, 6), (7, 1), (100, 17)):
        c = R.ppo_continuous_case(rng, B, A, 0.2)
        args = (c["mean"], c["log_std"], c["actions"], c["advantages"], c["old_mean"], c["old_std"], 0.2, 0.01)
        r, o = R.ppo_continuous_loss(*args), L.ppo_continuous_loss(*args)
        np.testing.assert_allclose([o["surrogate"], o["entropy"], o["kl"], o["total"]], r["scalars"], rtol=5e-5, atol=2e-6)
        np.testing.assert_allclose(o["ratio"], r["ratio"], rtol=5e-5)
        np.testing.assert_allclose(o["dmean"], r["dmean"], rtol=5e-5, atol=1e-7)
        np.testing.assert_allclose(o["dlog_std"], r["dlog_std"], rtol=2e-4, atol=2e-6)
    for kind in ("mse", "huber"):
        out, target, w = R.huber_case(rng, 33, 5)
        r = R.regression_loss(out, target, w, kind, 0.5)
        ol, og = L.regression_head_loss(out, target, w, kind, 0.5)
        np.testing.assert_allclose(ol, r["loss"], rtol=1e-5)
        np.testing.assert_allclose(og, r["grad"], rtol=1e-5, atol=1e-9)


def test_reference_mxnet_known_answer():
    """rl_coach/tests/architectures/mxnet_components/heads/test_ppo_head.py:363-376: surrogate = -0.142857153 (fp32)"""
    new = np.array([[0.9, 0.1], [0.2, 0.8], [0.4, 0.6]], dtype=F32)
    old = np.array([[0.7, 0.3], [0.2, 0.8], [0.4, 0.6]], dtype=F32)
    r = R.ppo_discrete_loss(np.log(new), [0, 1, 0], [-2, 2, 1], old, 0.2, 0.0)
    assert abs(r["scalars"][0] - (-0.142857153)) <= U24 * r["scalars_units"][0]
    assert abs(r["scalars"][0] + 1 / 7) < 2e-8
    # a rejected row leaves the divisor at B
    bad = R.ppo_discrete_loss(np.log(new), [0, 5, 0], [-2, 2, 1], old, 0.2, 0.0)
    assert bad["valid"].tolist() == [True, False, True]
    np.testing.assert_allclose(bad["scalars"][0], -(r["surrogate_rows"][0] + r["surrogate_rows"][2]) / 3, rtol=1e-15)


def test_counted_bounds_stay_tight():
    """the counted tolerances on ordinary inputs are a few 1e-5 of the value's own scale: they cannot silently become
    vacuous.  (Scale: the value itself; for sums that cancel, the sum of the absolute terms.)"""
    c = R.ppo_discrete_case(np.random.RandomState(1), 1024, 18, 0.2)
    r = R.ppo_discrete_loss(c["logits"], c["actions"], c["advantages"], c["old_probs"], 0.2, 0.01)
    assert np.all(U24 * r["ratio_units"] < 2e-5 * r["ratio"])
    assert np.all(U24 * r["scalars_units"][:2] < 2e-5 * np.abs(r["scalars"][:2]))
    assert U24 * r["scalars_units"][2] < 5e-5
    scale = (np.abs(c["advantages"].astype(F64)) * r["ratio"])[:, None] / 1024
    assert np.all(U24 * r["dlogits_units"] < 5e-5 * scale)
    c = R.ppo_continuous_case(np.random.RandomState(2), 1024, 6, 0.2)
    r = R.ppo_continuous_loss(c["mean"], c["log_std"], c["actions"], c["advantages"], c["old_mean"], c["old_std"], 0.2, 0.01)
    assert np.all(U24 * r["ratio_units"] < 1e-4 * r["ratio"])
    out, target, w = R.huber_case(np.random.RandomState(3), 2049, 18)
    r = R.regression_loss(out, target, w, "huber")
    assert U24 * r["loss_units"] < 5e-6 * r["loss"]
    p, units = R.softmax(np.random.RandomState(4).randn(129, 18).astype(F32))
    assert np.all(U24 * units < 2e-6 * p)
    assert [R.block_for(b) for b in (1, 63, 64, 65, 1024, 1025, 2049)] == [64, 64, 64, 128, 1024, 1024, 1024]
    assert [R.sum_depth(b) for b in (1, 64, 65, 1024, 1025, 2049)] == [6, 6, 7, 10, 11, 12]
