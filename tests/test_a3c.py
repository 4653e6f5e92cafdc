"""Actor-Critic (A3C) on the device: rlx_a3c_window_loss (csrc/a3c.hip) against the numpy restatement (tests/a3c_ref.py,
itself pinned to the reference agent by tests/test_a3c_ref.py) and against the reference agent's own targets
(tests/golden/a3c.npz), the network update against the oracle's layers + TF1 Adam composed with that restatement, the
agent's windows, targets and cadence on the device CartPole, the backend interface and the CartPole_A3C preset.

Tolerances.  The launch is compared with the restatement BIT FOR BIT on every output: the fp64 targets and advantages
are restated operation by operation, the fp32 row arithmetic is pg_ref's with its rounding points, and the batch sums are
restated in the launch's own fixed order (a3c_ref.tree_sum).  The network update goes through GEMMs whose fp32 summation
order is a tuning parameter: it is compared under tests/tolerances.py's LOSS and WEIGHTS, as
test_pg.py::test_network_update_equals_the_composed_oracle compares PG's."""
import numpy as np
import pytest

import a3c_ref as R
import pg_ref
from test_a3c_ref import fixture_case
from tolerances import LOSS, OUT, WEIGHTS

pytestmark = pytest.mark.gpu

BITS64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
BITS32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
SCALARS = ("loss", "value_loss", "policy_loss", "entropy")


def _t(x, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t if dtype is None else t.to(dtype)


def _launch(rlx, dev, V, logits, actions, rewards, game_over, discount, gae_lambda, rescaler, estimate_gae, beta,
            v_weight=0.5, pad=3, given=None):
    """V [rows], logits [rows, A] -> every output of one launch.  Both heads' buffers get a leading dimension with `pad`
    more columns, filled with NaN, which the launch must neither read nor write."""
    import torch
    rows, A = logits.shape
    T = len(actions)
    ld, ld_v = A + pad, 1 + pad
    zb = np.full((rows, ld), np.nan, np.float32)
    zb[:, :A] = logits
    vb = np.full((rows, ld_v), np.nan, np.float32)
    vb[:, 0] = V
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    dz, dv, sc = nan(rows, ld), nan(rows, ld_v), nan(4)
    if given is None:
        tgt = torch.full((T,), float("nan"), dtype=torch.float64, device=dev)
        adv = torch.full((T,), float("nan"), dtype=torch.float64, device=dev)
    else:
        tgt, adv = _t(np.asarray(given[0], np.float64), dev), _t(np.asarray(given[1], np.float64), dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    go = _t(np.array([int(bool(game_over))], np.uint8), dev)
    rlx.a3c_window_loss(_t(vb, dev), ld_v, _t(zb, dev), ld, _t(np.asarray(actions, np.int32), dev),
                        _t(np.asarray(rewards, np.float32), dev), go, T, rows, A, float(discount), float(gae_lambda),
                        int(rescaler), int(estimate_gae), float(beta), float(v_weight), tgt, adv, dv, ld_v, dz, ld, sc,
                        status, 0)
    torch.cuda.synchronize()
    dz, dv, sc = dz.cpu().numpy(), dv.cpu().numpy(), sc.cpu().numpy()
    if int(status.item()) & R.STATUS_NO_BOOTSTRAP_ROW:
        assert np.isnan(dz).all() and np.isnan(dv).all() and np.isnan(sc).all()
        return dict(status=int(status.item()))
    assert np.isnan(dz[:, A:]).all() and np.isnan(dv[:, 1:]).all()
    return dict(targets=tgt.cpu().numpy(), advantages=adv.cpu().numpy(), dV=dv[:, 0], dlogits=dz[:, :A], loss=sc[0],
                value_loss=sc[1], policy_loss=sc[2], entropy=sc[3], status=int(status.item()))


def _assert_bit_equal(k, r, what=""):
    assert k["status"] == r["status"], what
    assert np.array_equal(BITS64(k["targets"]), BITS64(r["targets"])), what
    assert np.array_equal(BITS64(k["advantages"]), BITS64(r["advantages"])), what
    assert np.array_equal(BITS32(k["dV"]), BITS32(r["dV"])), what
    assert np.array_equal(BITS32(k["dlogits"]), BITS32(r["dlogits"])), what
    for name in SCALARS:
        assert BITS32(k[name]) == BITS32(r[name]), (what, name, k[name], r[name])


# (rescaler, gae_lambda, estimate_state_value_using_gae)
MODES = ((R.A_VALUE, 0.96, False), (R.GAE, 0.96, False), (R.GAE, 1.0, True), (R.GAE, 1.0, False))


@pytest.mark.parametrize("A", [1, 2, 18])
@pytest.mark.parametrize("T", [1, 2, 5, 63, 64, 65, 200, 1024, 1025])
def test_window_loss_kernel_equals_the_restatement_bit_for_bit(rlx, dev, T, A):
    """T around the wave (64), one thread per row (<= 256), the strided-row path and more than one chunk of the
    recurrence (> 256), a whole number of chunks and one row more (1024, 1025); both rescalers (GAE with and without the
    GAE value targets), bootstrapped and terminal, beta 0 and 0.01; a saturated row; NaN padding in both heads' buffers;
    a terminal window is launched with and without the bootstrap row."""
    rng = np.random.RandomState(T * 100 + A)
    logits = (rng.randn(T + 1, A) * 2).astype(np.float32)
    if A > 1:
        logits[0] = -30.0
        logits[0, A - 1] = 30.0
    V = (rng.randn(T + 1) * 0.3).astype(np.float32)
    actions = rng.randint(0, A, size=T)
    actions[0] = 0
    rewards = (rng.uniform(-1, 2, size=T).astype(np.float32) * np.float32(1 / 200.))
    for (rescaler, lam, est), game_over, beta in [(m, g, b) for m in MODES for g in (False, True) for b in (0.0, 0.01)]:
        what = "T %d A %d rescaler %d lambda %g est %d game_over %d beta %g" % (T, A, rescaler, lam, est, game_over, beta)
        k = _launch(rlx, dev, V, logits, actions, rewards, game_over, 0.99, lam, rescaler, est, beta)
        r = R.window_loss(V, logits, actions, rewards, game_over, 0.99, lam, rescaler, est, beta)
        assert k["status"] == 0
        _assert_bit_equal(k, r, what)
        # the bootstrap row's gradients are exactly zero, whatever its logits and V are
        assert k["dV"][T] == 0 and np.all(k["dlogits"][T] == 0) and np.any(k["dV"][:T] != 0)
        if game_over:
            # ... and the means divide by T, not T + 1: the same window without the row gives the same bits
            bare = _launch(rlx, dev, V[:T], logits[:T], actions, rewards, True, 0.99, lam, rescaler, est, beta)
            for name in SCALARS + ("targets", "advantages"):
                assert np.asarray(bare[name]).tobytes() == np.asarray(k[name]).tobytes(), (what, name)
            assert bare["dV"].tobytes() == k["dV"][:T].tobytes() and bare["dlogits"].tobytes() == k["dlogits"][:T].tobytes()
    again = _launch(rlx, dev, V, logits, actions, rewards, False, 0.99, 0.96, R.GAE, False, 0.01)
    first = _launch(rlx, dev, V, logits, actions, rewards, False, 0.99, 0.96, R.GAE, False, 0.01)
    assert all(np.asarray(again[n]).tobytes() == np.asarray(first[n]).tobytes() for n in again)


def test_kernel_on_the_golden_cases_gives_the_reference_agents_targets(rlx, dev, golden):
    """what the reference's own ActorCriticAgent.learn_from_batch handed to accumulate_gradients, bit for bit, fed the
    recorded stand-in network's V values"""
    z = golden("a3c")
    rng = np.random.RandomState(0)
    for c in (fixture_case(z, k) for k in range(int(z["n_cases"]))):
        T = c["rewards"].size
        V = np.concatenate([c["v"].reshape(-1), c["boot"].reshape(-1)])
        logits = rng.randn(T + 1, 3).astype(np.float32)
        k = _launch(rlx, dev, V, logits, c["actions"], c["rewards"], c["game_over"], c["discount"], c["gae_lambda"],
                    c["rescaler"], c["estimate_gae"], 0.01)
        assert k["status"] == 0
        assert np.array_equal(BITS64(k["targets"]), BITS64(c["targets"]))
        assert np.array_equal(BITS64(k["advantages"]), BITS64(c["advantages"]))
        assert np.array_equal(BITS64(k["advantages"]), BITS64(c["advantages_signal"].reshape(-1)))


@pytest.mark.parametrize("beta", [0.0, 0.01])
@pytest.mark.parametrize("T,A", [(1, 2), (65, 6), (257, 18), (200, 1)])
def test_policy_half_is_bit_identical_to_the_pg_head_loss(rlx, dev, T, A, beta):
    """with the V head's loss weight 0: dlogits, the loss and the mean entropy of rlx_pg_head_loss on the same logits,
    actions and (fp32) advantages — one definition of the row arithmetic"""
    import torch
    rng = np.random.RandomState(T + A)
    logits = (rng.randn(T + 1, A) * 2).astype(np.float32)
    V = (rng.randn(T + 1) * 0.3).astype(np.float32)
    actions = rng.randint(0, A, size=T)
    rewards = rng.uniform(-1, 2, size=T).astype(np.float32)
    k = _launch(rlx, dev, V, logits, actions, rewards, False, 0.99, 0.96, R.GAE, False, beta, v_weight=0.0, pad=0)
    assert k["value_loss"] == 0 and not k["dV"].any()
    d = torch.full((T + 1, A), float("nan"), dtype=torch.float32, device=dev)
    sc = torch.full((2,), float("nan"), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rlx.pg_head_loss(_t(logits, dev), A, _t(actions.astype(np.int32), dev), _t(k["advantages"].astype(np.float32), dev),
                     float(beta), T + 1, T, A, d, A, sc, status, 0)
    pg_loss, pg_entropy = sc.cpu().numpy()
    assert d.cpu().numpy().tobytes() == k["dlogits"].tobytes()
    assert BITS32(pg_entropy) == BITS32(k["entropy"])
    assert pg_loss == k["loss"] and BITS32(np.abs(pg_loss)) == BITS32(np.abs(k["loss"]))       # 0 + x: -0 becomes +0
    if beta == 0:
        assert pg_loss == k["policy_loss"]


def test_given_targets_are_read_not_computed(rlx, dev):
    """RLX_A3C_TARGETS_GIVEN (what the backend interface's accumulate_gradients is handed): the two fp64 arrays are
    inputs, rounded to fp32 once; rewards and the game-over flag are not read"""
    rng = np.random.RandomState(8)
    T, A = 70, 3
    logits, V = rng.randn(T, A).astype(np.float32), rng.randn(T).astype(np.float32)
    actions, tgt, adv = rng.randint(0, A, size=T), rng.randn(T), rng.randn(T)
    k = _launch(rlx, dev, V, logits, actions, np.full(T, np.nan, np.float32), False, 0.99, 0.96, -1, False, 0.01,
                given=(tgt, adv))
    r = R.head_losses(V, logits, actions, tgt.astype(np.float32), adv.astype(np.float32), 0.01, 0.5, T)
    assert k["status"] == 0 and np.array_equal(k["targets"], tgt) and np.array_equal(k["advantages"], adv)
    _assert_bit_equal(k, dict(r, targets=tgt, advantages=adv))


def test_out_of_range_actions_a_missing_bootstrap_row_and_bad_arguments(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    rng = np.random.RandomState(2)
    T, A = 5, 3
    logits, V = rng.randn(T + 1, A).astype(np.float32), rng.randn(T + 1).astype(np.float32)
    actions = np.array([0, 3, 1, -1, 2])
    rewards = rng.uniform(-1, 2, size=T).astype(np.float32)
    k = _launch(rlx, dev, V, logits, actions, rewards, False, 0.99, 0.96, R.A_VALUE, False, 0.01)
    r = R.window_loss(V, logits, actions, rewards, False, 0.99, 0.96, R.A_VALUE, False, 0.01)
    assert k["status"] == R.STATUS_BAD_ACTION == r["status"]
    assert np.all(k["dlogits"][[1, 3]] == 0) and np.any(k["dlogits"][0] != 0) and np.all(k["dV"][:T] != 0)
    _assert_bit_equal(k, r)
    # no term: the policy sums are those of the three valid rows alone
    p, q, S, lp, H = pg_ref.head_rows(logits[[0, 2, 4]])
    np.testing.assert_allclose(k["entropy"], H.sum() / 5, **LOSS)
    # a window that is not a game over needs the bootstrap row: status, and nothing is written
    assert _launch(rlx, dev, V[:T], logits[:T], [0, 1, 2, 0, 1], rewards, False, 0.99, 0.96, R.GAE, False,
                   0.01)["status"] == R.STATUS_NO_BOOTSTRAP_ROW
    f = torch.zeros(8, 32, dtype=torch.float32, device=dev)
    d = torch.zeros(8, dtype=torch.float64, device=dev)
    it = torch.zeros(8, dtype=torch.int32, device=dev)
    go = torch.zeros(1, dtype=torch.uint8, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(T=4, rows=5, A=2, rescaler=R.GAE, ld=32, ld_v=1, V=f, rewards=f, game_over=go, status=st):
        rlx.a3c_window_loss(V, ld_v, f, ld, it, rewards, game_over, T, rows, A, 0.99, 0.96, rescaler, 0, 0.0, 0.5, d, d,
                            f, ld_v, f, ld, f, status, 0)
    call()
    for kw in (dict(T=0, rows=1), dict(T=-1, rows=0), dict(A=0), dict(A=19), dict(rows=3), dict(rows=6), dict(ld=1),
               dict(ld_v=0), dict(V=None), dict(rewards=None), dict(game_over=None), dict(status=None)) + \
            tuple(dict(rescaler=x) for x in (0, 1, 2, 3, 4, 6, 7, 9, -2)):
        with pytest.raises(RlxError):
            call(**kw)


def _oracle_for(net, obs_shape, lr, eps):
    """the oracle's DQN chain (embedder, middleware, one Dense head = the policy head) on the network's weights, with a
    second Dense head (V) on the same torso registered for the norm and the Adam step"""
    from oracle import nn as N
    from oracle.agents import DQNOracle
    arrays = {k.replace("main/policy_values_head/fc", "main/q_head/dense"): v
              for k, v in net.params.named_arrays().items()}
    o = DQNOracle(arrays, obs_shape, net.A, lr=lr, eps=eps)
    vn = "main/v_values_head/output"
    o.v_head = N.Dense(arrays[vn + "/kernel"][0].copy(), arrays[vn + "/bias"][0].copy())
    o.chains.append(("vh", 0, N.Chain([o.v_head])))
    o.names[("vh", 0)] = [vn]
    return o


def test_network_update_equals_the_composed_oracle(dev):
    """ActorCriticNet: forward on T + 1 rows, the window launch, both heads and the torso backward, accumulation over
    three windows of different lengths (bootstrapped and terminal, both rescalers), one Adam step — twice — against
    oracle layers + TF1 Adam + the restatement, in the manner and at the tolerances of
    test_pg.py::test_network_update_equals_the_composed_oracle."""
    import torch
    from coach_amd.nn.networks import ActorCriticNet
    from oracle import nn as N
    rng = np.random.RandomState(7)
    A, lr, beta = 2, 5e-4, 0.01
    net = ActorCriticNet(dev, (4,), A, learning_rate=lr, optimizer_epsilon=1e-4, beta_entropy=beta, seed=3)
    names = net.params.entries
    assert "main/policy_values_head/fc/kernel" in names and "main/v_values_head/output/kernel" in names
    assert net.target is None and net.clip_gradients == 40.0
    o = _oracle_for(net, (4,), lr, 1e-4)
    cases = ((9, False, R.GAE, 1.0), (1, True, R.A_VALUE, 0.96), (37, False, R.A_VALUE, 0.96))
    for step in range(2):
        w0 = net.params.weights.clone()
        shards, acc_before = [], None
        for T, game_over, rescaler, lam in cases:
            obs = rng.randn(T + 1, 4).astype(np.float32)
            actions = rng.randint(0, A, size=T)
            rewards = rng.uniform(-1, 2, size=T).astype(np.float32)
            tgt = torch.zeros(T, dtype=torch.float64, device=dev)
            adv = torch.zeros(T, dtype=torch.float64, device=dev)
            loss = net.accumulate_window(_t(obs, dev), T, True, _t(actions.astype(np.int32), dev), tgt, adv,
                                         _t(rewards, dev), _t(np.array([int(game_over)], np.uint8), dev), 0.99, lam,
                                         rescaler, False)
            feat = o.tower.forward(N.prep_obs(obs, False))
            z, v = o.head.forward(feat).astype(np.float32), o.v_head.forward(feat).astype(np.float32)[:, 0]
            r = R.window_loss(v, z, actions, rewards, game_over, 0.99, lam, rescaler, False, beta)
            o.tower.backward(o.head.backward(r["dlogits"]) + o.v_head.backward(r["dV"][:, None]))
            shards.append(o.snapshot_grads())
            # the targets are formed from the device's own V: compared at the V head's output tolerance
            np.testing.assert_allclose(net.values.cpu().numpy(), v, **OUT)
            np.testing.assert_allclose(tgt.cpu().numpy(), r["targets"], **OUT)
            np.testing.assert_allclose(adv.cpu().numpy(), r["advantages"], rtol=1e-4, atol=4e-6)
            np.testing.assert_allclose(float(loss.item()), r["loss"], **LOSS)
            np.testing.assert_allclose(float(net.value_loss.item()), r["value_loss"], **LOSS)
            np.testing.assert_allclose(float(net.policy_loss.item()), r["policy_loss"], **LOSS)
            np.testing.assert_allclose(float(net.entropy.item()), r["entropy"], **LOSS)
            np.testing.assert_allclose(float(net.norm.item()), o.global_norm(), **LOSS)
            assert o.global_norm() < 40.0                            # (nothing is clipped in this test)
            expect = net.params.grads.clone() if acc_before is None else acc_before + net.params.grads
            assert torch.equal(net.accumulated, expect) and net.accumulated.abs().sum() > 0
            acc_before = net.accumulated.clone()
            assert torch.equal(net.params.weights, w0)               # nothing is applied while accumulating
        net.apply_accumulated()
        o.apply_summed_gradients(shards, 1, False)
        assert not net.accumulated.any() and not torch.equal(net.params.weights, w0)
        net.check_status()
        w = net.params.named_arrays()
        wo = {k.replace("main/q_head/dense", "main/policy_values_head/fc"): v for k, v in o.weights().items()}
        assert set(wo) == set(w)
        for name, towers in wo.items():
            np.testing.assert_allclose(w[name][0], towers[0], err_msg=name, **WEIGHTS)
    assert torch.isfinite(net.params.weights).all()


@pytest.mark.parametrize("A,T", [(16, 63),      # 64 rows, rows * A = 1024: both heads in one launch, forward and backward
                                 (16, 64),      # 65 rows, rows * A = 1040: one launch forward, launches of their own backward
                                 (17, 5)])      # wider than the narrow-dense kernels serve: launches of their own both ways
def test_one_window_update_equals_the_composed_oracle_at_the_head_forks_branch_boundaries(dev, A, T):
    """test_network_update_equals_the_composed_oracle with ONE window (the bootstrap row present) and one Adam step, at
    the shapes where the heads' launches change form — the same oracle, restatement and tolerances."""
    import torch
    from coach_amd.nn.networks import ActorCriticNet
    from oracle import nn as N
    rng = np.random.RandomState(11)
    lr, beta, lam = 5e-4, 0.01, 0.96
    net = ActorCriticNet(dev, (4,), A, learning_rate=lr, optimizer_epsilon=1e-4, beta_entropy=beta, seed=3)
    o = _oracle_for(net, (4,), lr, 1e-4)
    w0 = net.params.weights.clone()
    obs = rng.randn(T + 1, 4).astype(np.float32)
    actions = rng.randint(0, A, size=T)
    rewards = rng.uniform(-1, 2, size=T).astype(np.float32)
    tgt = torch.zeros(T, dtype=torch.float64, device=dev)
    adv = torch.zeros(T, dtype=torch.float64, device=dev)
    loss = net.accumulate_window(_t(obs, dev), T, True, _t(actions.astype(np.int32), dev), tgt, adv, _t(rewards, dev),
                                 _t(np.array([0], np.uint8), dev), 0.99, lam, R.A_VALUE, False)
    feat = o.tower.forward(N.prep_obs(obs, False))
    z, v = o.head.forward(feat).astype(np.float32), o.v_head.forward(feat).astype(np.float32)[:, 0]
    r = R.window_loss(v, z, actions, rewards, False, 0.99, lam, R.A_VALUE, False, beta)
    o.tower.backward(o.head.backward(r["dlogits"]) + o.v_head.backward(r["dV"][:, None]))
    shards = [o.snapshot_grads()]
    print("\n  A %d T %d: V max abs diff %.3e, loss %.6f / %.6f, norm %.6f / %.6f" % (
        A, T, float(np.abs(net.values.cpu().numpy() - v).max()), float(loss.item()), r["loss"], float(net.norm.item()),
        o.global_norm()))
    np.testing.assert_allclose(net.values.cpu().numpy(), v, **OUT)
    np.testing.assert_allclose(tgt.cpu().numpy(), r["targets"], **OUT)
    np.testing.assert_allclose(adv.cpu().numpy(), r["advantages"], rtol=1e-4, atol=4e-6)
    np.testing.assert_allclose(float(loss.item()), r["loss"], **LOSS)
    np.testing.assert_allclose(float(net.value_loss.item()), r["value_loss"], **LOSS)
    np.testing.assert_allclose(float(net.policy_loss.item()), r["policy_loss"], **LOSS)
    np.testing.assert_allclose(float(net.entropy.item()), r["entropy"], **LOSS)
    np.testing.assert_allclose(float(net.norm.item()), o.global_norm(), **LOSS)
    assert o.global_norm() < 40.0                                    # (nothing is clipped in this test)
    assert torch.equal(net.accumulated, net.params.grads) and net.accumulated.abs().sum() > 0
    assert torch.equal(net.params.weights, w0)                       # nothing is applied while accumulating
    net.apply_accumulated()
    o.apply_summed_gradients(shards, 1, False)
    assert not net.accumulated.any() and not torch.equal(net.params.weights, w0)
    net.check_status()
    w = net.params.named_arrays()
    wo = {k.replace("main/q_head/dense", "main/policy_values_head/fc"): v for k, v in o.weights().items()}
    assert set(wo) == set(w)
    for name, towers in wo.items():
        np.testing.assert_allclose(w[name][0], towers[0], err_msg=name, **WEIGHTS)


def test_acting_runs_the_policy_head_alone_and_wide_heads_take_the_separate_launches(dev):
    """policy_values equals predict's logits; A = 18 is wider than the narrow-dense helper serves, so both heads run as
    launches of their own — the same window gives the restatement's losses either way"""
    from coach_amd.nn.networks import ActorCriticNet
    rng = np.random.RandomState(5)
    for A in (2, 18):
        net = ActorCriticNet(dev, (4,), A, beta_entropy=0.01, seed=1)
        obs = rng.randn(6, 4).astype(np.float32)
        z = net.policy_values(_t(obs, dev), 6, tag="act").data.view(6, A).cpu().numpy()
        v, z2 = net.predict(_t(obs, dev), 6)
        np.testing.assert_allclose(z, z2.cpu().numpy(), **OUT)
        import torch
        T = 5
        tgt, adv = (torch.zeros(T, dtype=torch.float64, device=dev) for _ in range(2))
        actions, rewards = rng.randint(0, A, size=T), rng.uniform(-1, 2, size=T).astype(np.float32)
        net.window_gradients(_t(obs, dev), T, True, _t(actions.astype(np.int32), dev), tgt, adv, _t(rewards, dev),
                             _t(np.array([0], np.uint8), dev), 0.99, 0.96, R.GAE, False)
        r = R.window_loss(v.cpu().numpy(), z2.cpu().numpy(), actions, rewards, False, 0.99, 0.96, R.GAE, False, 0.01)
        np.testing.assert_allclose(net.scalars.cpu().numpy(), [r[n] for n in SCALARS], **LOSS)
        net.check_status()
        assert float(net.norm.item()) > 0


def test_backend_interface_serves_the_actor_critic_network(dev):
    """Architecture.predict / accumulate_gradients / apply_gradients through a NetworkWrapper, fed the way
    ActorCriticAgent.learn_from_batch feeds it (actor_critic_agent.py:175-177), against the same network driven
    directly: identical weights after two accumulated windows and one applied step."""
    import torch
    from coach_amd.agents.actor_critic_agent import ActorCriticAgentParameters
    from coach_amd.architectures.hip_architecture import ActorCriticArchitecture
    from coach_amd.architectures.network_wrapper import NetworkWrapper
    from coach_amd.nn.networks import ActorCriticNet, actor_critic_net_kwargs
    from coach_amd.spaces import BoxActionSpace, DiscreteActionSpace, ObservationSpace, SpacesDefinition, StateSpace
    ap = ActorCriticAgentParameters()
    ap.seed = 5
    ap.algorithm.beta_entropy = 0.01
    A = 3
    spaces = SpacesDefinition(StateSpace({"observation": ObservationSpace((6,))}), None, DiscreteActionSpace(A))
    np.random.seed(21)               # the V head's normalized-columns initialiser draws from the global stream
    nw = NetworkWrapper(ap, has_target=False, has_global=False, name="main", spaces=spaces, worker_device=dev)
    online = nw.online_network
    assert isinstance(online, ActorCriticArchitecture) and nw.target_network is None
    np.random.seed(21)
    twin = ActorCriticNet(dev, (6,), A, **actor_critic_net_kwargs(ap.network_wrappers["main"], ap.algorithm, 5))
    assert twin.v_loss_weight == 0.5 and twin.clip_gradients == 40.0
    assert torch.equal(twin.params.weights, online.net.params.weights)
    rng = np.random.RandomState(1)
    obs = rng.randn(4, 6).astype(np.float32)
    values, probs = online.predict({"observation": obs})
    v, z = twin.predict(_t(obs, dev), 4)
    assert values.shape == (4, 1) and probs.shape == (4, A)
    assert np.array_equal(values[:, 0], v.cpu().numpy())
    np.testing.assert_allclose(probs, pg_ref.head_rows(z.cpu().numpy())[0], **OUT)
    w0 = online.net.params.weights.clone()
    for T in (7, 2):
        obs, actions = rng.randn(T, 6).astype(np.float32), rng.randint(0, A, size=T)
        targets, advantages = rng.randn(T, 1), rng.randn(T)        # fp64, as learn_from_batch hands them over
        total_loss, losses, norm = online.accumulate_gradients({"observation": obs, "output_1_0": actions},
                                                               [targets, advantages])[:3]
        twin.accumulate_window(_t(obs, dev), T, False, _t(actions.astype(np.int32), dev), _t(targets.reshape(-1), dev),
                               _t(advantages, dev))
        assert total_loss == float(twin.loss.item()) and norm == float(twin.norm.item())
        assert losses[:2] == [float(twin.value_loss.item()), float(twin.policy_loss.item())] and len(losses) == 3
        np.testing.assert_allclose(sum(losses), total_loss, rtol=1e-6)
        assert torch.equal(online.accumulated_gradients, twin.accumulated)
    assert torch.equal(online.net.params.weights, w0)
    nw.apply_gradients_and_sync_networks()
    twin.apply_accumulated()
    assert torch.equal(online.net.params.weights, twin.params.weights) and not torch.equal(twin.params.weights, w0)
    assert not online.accumulated_gradients.any()
    with pytest.raises(ValueError, match="continuous PolicyHead"):
        box = SpacesDefinition(StateSpace({"observation": ObservationSpace((6,))}), None,
                               BoxActionSpace(2, low=-1.0, high=1.0))
        NetworkWrapper(ap, has_target=False, has_global=False, name="main", spaces=box, worker_device=dev)


def _agent(dev, n_env, t_max, rescaler, gae_lambda=0.96, seed=3):
    from coach_amd.agents.actor_critic_agent import ActorCriticAgent, ActorCriticAgentParameters
    from coach_amd.agents.policy_optimization_agent import PolicyGradientRescaler
    from coach_amd.core_types import RunPhase
    from coach_amd.environments.cartpole_vector_environment import (
        CartPoleVectorEnvironment, CartPoleVectorEnvironmentParameters)
    p = ActorCriticAgentParameters()
    p.seed = seed
    p.algorithm.num_steps_between_gradient_updates = t_max
    p.algorithm.reward_rescale = 1 / 200.
    p.algorithm.beta_entropy = 0.01
    p.algorithm.gae_lambda = gae_lambda
    p.algorithm.policy_gradient_rescaler = PolicyGradientRescaler(rescaler)
    env = CartPoleVectorEnvironment(CartPoleVectorEnvironmentParameters(n_env, "CartPole-v0", seed=11), dev)
    agent = ActorCriticAgent(p, env, dev)
    agent.phase = env.phase = RunPhase.TRAIN
    agent.debug_windows, agent.debug_targets = [], []
    return agent


def _assert_targets_are_the_restatement(agent, rescaler, gae_lambda):
    """every window's fp64 targets and advantages equal the restatement fed the device's own V values, bit for bit; a
    finished episode's last transition is a game over (CartPole reports its limit as one), a running one's is not"""
    reward = np.float32(1.0) * np.float32(1 / 200.)
    assert len(agent.debug_targets) == len(agent.debug_windows) > 0
    for (env, start, end, _, _), (V, tgt, adv, go) in zip(agent.debug_windows, agent.debug_targets):
        T = end - start
        V, go = V.cpu().numpy(), bool(go.item())
        assert V.shape == (T + 1,) and np.isfinite(V).all()
        w = R.window_targets(V[:T], V[T], np.full(T, reward, np.float32), go, 0.99, gae_lambda, rescaler, False)
        assert np.array_equal(BITS64(tgt.cpu().numpy()), BITS64(w["targets"])), (env, start, end)
        assert np.array_equal(BITS64(adv.cpu().numpy()), BITS64(w["advantages"])), (env, start, end)
    return [bool(t[3].item()) for t in agent.debug_targets]


@pytest.mark.parametrize("t_max,rescaler,lam", [(5, R.GAE, 1.0), (5000, R.A_VALUE, 0.96)])
def test_agent_with_one_env_keeps_the_base_cadence_and_restated_targets(dev, t_max, rescaler, lam):
    """windows, pointers, current_episode, training_iteration and the apply cadence are the on-policy base's (pg_ref.run,
    pinned to the reference by PG's fixture); every window's targets are the restatement's on the device's V"""
    from test_pg import _step
    agent = _agent(dev, 1, t_max, rescaler, lam)
    lengths, calls = _step(agent, 12)
    ws = pg_ref.run([np.zeros(L, np.float32) for L in lengths[0]], 0.99, pg_ref.FUTURE_RETURN, 200, t_max, 5)
    got = agent.debug_windows
    assert [(s, e, ce, ap) for _, s, e, ce, ap in got] == \
        [(w["start"], w["end"], w["current_episode"], w["applied"]) for w in ws]
    assert agent.training_iteration == len(ws) == ws[-1]["training_iteration"] and agent.current_episode == 12
    assert any(ap for *_, ap in got) and not all(ap for *_, ap in got)
    assert (t_max == 5) == any(s > 0 for _, s, *_ in got)
    game_overs = _assert_targets_are_the_restatement(agent, rescaler, lam)
    assert game_overs == [w["complete"] for w in ws]
    assert any(c["moved"] for c in calls)
    for c in calls:
        applied = any(ap for *_, ap in c["windows"])
        assert applied == c["moved"]                                 # (a bootstrapped gradient is never exactly zero)
        if c["windows"] and c["windows"][-1][-1]:
            assert not c["accumulated"]
    assert any(c["accumulated"] for c in calls if c["windows"] and not c["windows"][-1][-1])


def test_agent_with_three_envs_processes_windows_in_env_order(dev):
    """each env's windows are what its own single-env run gives for the same episode lengths; windows of one vector step
    come in env order; the envs share the episode counter; the targets of every env's windows are the restatement's"""
    from test_pg import _step
    agent = _agent(dev, 3, 5, R.GAE, 1.0, seed=4)
    lengths, calls = _step(agent, 15)
    got = agent.debug_windows
    for e in range(3):
        eps = lengths[e] + [200]
        ws = pg_ref.run([np.zeros(L, np.float32) for L in eps], 0.99, pg_ref.FUTURE_RETURN, 200, 5, 5)
        mine = [(s, t) for env, s, t, *_ in got if env == e]
        assert mine == [(w["start"], w["end"]) for w in ws][:len(mine)] and len(mine) >= len(lengths[e])
    for c in calls:
        envs = [w[0] for w in c["windows"]]
        assert envs == sorted(envs) and len(set(envs)) == len(envs)
    assert any(len(c["windows"]) > 1 for c in calls)
    ce = [w[3] for w in got]
    assert ce == sorted(ce) and agent.current_episode == sum(len(x) for x in lengths)
    assert agent.training_iteration == len(got)
    game_overs = _assert_targets_are_the_restatement(agent, R.GAE, 1.0)
    assert any(game_overs) and not all(game_overs)


def test_episode_buffer_keeps_the_game_over_byte_and_the_state_before_the_reset(dev):
    """the two columns a bootstrapping agent reads, written by the one copy launch of a step; the rows Policy Gradients
    reads are unchanged"""
    import torch
    from coach_amd.memories.episodic.single_episode_buffer import SingleEpisodeBuffer
    n, L, D = 2, 4, 3
    m = SingleEpisodeBuffer(dev, n, (D,), L)
    rng = np.random.RandomState(0)
    first = rng.randn(n, D).astype(np.float32)
    m.reset(_t(first, dev))
    states = [first]
    for step in range(3):
        nxt, rst = rng.randn(n, D).astype(np.float32), rng.randn(n, D).astype(np.float32)
        done = np.array([step == 1, False])
        go = _t(done.astype(np.uint8), dev)
        m.store(_t(np.array([step, step + 10], np.int32), dev), _t(np.array([0.5, 1.5], np.float32) * (step + 1), dev), go,
                _t(nxt, dev), _t(rst, dev), dones_host=done)
        states.append(np.where(done[:, None], rst, nxt))
        if step == 1:
            # env 0 finished a 2-step episode: its last row holds the game over and the observation BEFORE the reset
            rows, last_next, byte = m.bootstrap_rows(0, 0, 2, True)
            assert rows is None and int(byte.item()) == 1 and np.array_equal(last_next.cpu().numpy(), nxt[0])
            assert not np.array_equal(m.current_states()[0].cpu().numpy(), nxt[0])
            # env 1 runs on, and its last response is not yet visible (one transition): the T + 1 states in place, the
            # last of them the state the step just taken started from
            rows, last_next, byte = m.bootstrap_rows(1, 0, 1, False)
            assert rows.shape == (2, D) and int(byte.item()) == 0
            assert np.array_equal(rows.cpu().numpy(), np.stack([states[0][1], states[1][1]]))
            assert np.array_equal(last_next.cpu().numpy(), states[1][1])
    m.check_status()
    obs, act, rew = m.episode_rows(1, 1, 3)
    assert act.tolist() == [11, 12] and rew.tolist() == [1.5, 3.0, 4.5]
    assert np.array_equal(obs.cpu().numpy(), np.stack([states[1][1], states[2][1]]))
    assert m.steps.tolist() == [1, 3] and m.last_episode_lengths.tolist() == [2, 0]
    assert torch.equal(m.game_over.view(n, L)[1], torch.zeros(L, dtype=torch.uint8, device=dev))


def test_cartpole_a3c_preset_builds_and_runs_200_steps(dev, tmp_path):
    """nothing about learning is asserted (the recorded validation runs are in DESIGN.md): the preset builds, trains
    for 200 vector steps with finite weights, and the four Actor-Critic signals reach the CSV"""
    import importlib
    import torch
    from coach_amd.core_types import EnvironmentSteps, RunPhase
    gm = importlib.import_module("coach_amd.presets.CartPole_A3C").make()
    gm.schedule.improve_steps = EnvironmentSteps(200)
    gm.schedule.steps_between_evaluation_periods = EnvironmentSteps(100)
    gm.device = dev
    gm.logger.__init__(str(tmp_path / "a3c.csv"))
    rows = gm.improve()
    a = gm.agent
    assert type(a).__name__ == "ActorCriticAgent" and gm.total_steps_counters[RunPhase.TRAIN] == 200
    assert a.training_iteration >= 40 and sum(r.get("Evaluation Reward", "") != "" for r in rows) == 2
    gm.environment.check_status()
    a.check_status()
    assert torch.isfinite(a.networks["main"].params.weights).all()
    header = (tmp_path / "a3c.csv").read_text().splitlines()[0].split(",")
    for name in ("Advantages", "Values", "Value Loss", "Policy Loss", "Entropy", "Loss", "Grads (unclipped)",
                 "Discounted Return"):
        assert name + "/Mean" in header, name
        values = [r[name + "/Mean"] for r in rows if r.get(name + "/Mean", "") != ""]
        assert values and np.isfinite(np.asarray(values, dtype=np.float64)).all(), name
