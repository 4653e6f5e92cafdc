"""ACER on the device: rlx_acer_window_loss (csrc/acer.hip) against the numpy restatement (tests/acer_ref.py, itself
pinned to the reference agent by tests/test_acer_ref.py), against the reference agent's own values
(tests/golden/acer.npz) and against rlx_regression_loss fed the aliased target matrix; the network update against the
oracle's layers + TF1 Adam composed with the restatement; the agent's windows, stored behaviour probabilities, replay,
Adam-step count and average network on the device CartPole; the backend interface and the CartPole_ACER preset.

Tolerances.  The launch is compared with the restatement BIT FOR BIT on every output: the window's values are restated
operation by operation with their fp32 / fp64 rounding points and numpy's summation order, the heads' row arithmetic is
pg_ref's plus the operations acer_ref states in order, and the batch sums are restated in the launch's own fixed order
(a3c_ref.tree_sum).  Only the Q loss against rlx_regression_loss's scalar, whose sum has another order, is compared
under tests/tolerances.py's LOSS."""
import numpy as np
import pytest

import acer_ref as R
import pg_ref
from test_acer_ref import _window, fixture_case
from tolerances import LOSS

pytestmark = pytest.mark.gpu

BITS32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
ARRAYS = ("V", "rho", "rho_i", "avg", "q_retrace", "td_targets", "dQ", "dlogits")


def _t(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _padded(x, ld):
    out = np.full((x.shape[0], ld), np.nan, np.float32)
    out[:, :x.shape[1]] = x
    return out


def _launch(rlx, dev, Q, z, za, mu, actions, rewards, game_over, discount=0.99, c=10.0, delta=1.0, beta=0.0,
            q_weight=0.5, trust=False, pad=3, given=None, with_td=True, give_td=True):
    """Q, z [rows, A]; za, mu [T, A] -> every output of one launch.  Every matrix gets a leading dimension of its own
    with NaN padding columns, which the launch must neither read (a NaN would spread) nor write.  given: a dict of a
    computed launch's arrays, handed back in under RLX_ACER_TARGETS_GIVEN (the inputs that mode must not touch are then
    NaN or absent)."""
    import torch
    rows, A = Q.shape
    T = len(actions)
    ld = [A + pad + i for i in range(9)]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    mode = (R.MODE_TRUST_REGION if trust else 0) | (R.MODE_TARGETS_GIVEN if given is not None else 0)
    if given is None:
        V, rho, rho_i, avg, qret, boot = nan(T), nan(T, ld[4]), nan(T), nan(T, ld[5]), nan(T), nan(1)
        td = nan(T, ld[6]) if with_td else None
        za_d, mu_d = _t(_padded(za, ld[2]), dev), _t(_padded(mu, ld[3]), dev)
        rew, go = _t(np.asarray(rewards, np.float32), dev), _t(np.array([int(bool(game_over))], np.uint8), dev)
    else:
        V, rho_i, qret = (_t(given[n], dev) for n in ("V", "rho_i", "q_retrace"))
        rho, avg = _t(_padded(given["rho"], ld[4]), dev), _t(_padded(given["avg"], ld[5]), dev)
        td = _t(_padded(given["td_targets"], ld[6]), dev) if give_td else None
        za_d = mu_d = rew = go = boot = None
    dq, dz, sc = nan(rows, ld[7]), nan(rows, ld[8]), nan(7)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rlx.acer_window_loss(_t(_padded(Q, ld[0]), dev), ld[0], _t(_padded(z, ld[1]), dev), ld[1], rows, za_d, ld[2], mu_d,
                         ld[3], _t(np.asarray(actions, np.int32), dev), rew, go, T, A, float(discount), float(c),
                         float(delta), float(beta), float(q_weight), mode, V, rho, ld[4], rho_i, avg, ld[5], qret, boot,
                         td, ld[6], dq, ld[7], dz, ld[8], sc, status, 0)
    torch.cuda.synchronize()
    st = int(status.item())
    host = lambda v: None if v is None else v.cpu().numpy()
    V, rho, rho_i, avg, qret, boot, td, dq, dz, sc = map(host, (V, rho, rho_i, avg, qret, boot, td, dq, dz, sc))
    if st & R.STATUS_NO_BOOTSTRAP_ROW:
        assert all(np.isnan(v).all() for v in (V, rho, rho_i, avg, qret, boot, dq, dz, sc) if v is not None)
        return dict(status=st)
    assert all(np.isnan(v[:, A:]).all() for v in (rho, avg, td, dq, dz) if v is not None)
    out = dict(V=V, rho=rho[:, :A], rho_i=rho_i, avg=avg[:, :A], q_retrace=qret, dQ=dq[:, :A], dlogits=dz[:, :A],
               td_targets=None if td is None else td[:, :A], boot=None if boot is None else boot[0], status=st)
    out.update(zip(R.SCALARS, sc))
    return out


def _assert_bit_equal(k, r, what=""):
    assert k["status"] == r["status"], what
    for n in ARRAYS:
        if k[n] is not None:
            assert np.array_equal(BITS32(k[n]), BITS32(r[n])), (what, n)
    if k["boot"] is not None:
        assert BITS32(k["boot"]) == BITS32(r["boot"]), (what, "boot")
    for n in R.SCALARS:
        assert BITS32(k[n]) == BITS32(r[n]), (what, n, k[n], r[n])


def _same(a, b, names=ARRAYS + R.SCALARS):
    return all(np.asarray(a[n]).tobytes() == np.asarray(b[n]).tobytes() for n in names)


@pytest.mark.parametrize("A", [1, 2, 7, 8, 18])
@pytest.mark.parametrize("T", [1, 2, 5, 63, 64, 65, 200, 256, 257, 1025])
def test_window_loss_kernel_equals_the_restatement_bit_for_bit(rlx, dev, T, A):
    """T around the wave (64), one row per thread (<= 256), the strided rows and a second and fifth chunk of the
    recurrence (> 256); A around numpy's unrolled sum (8); bootstrapped and terminal, beta 0 and 0.01, the trust-region
    step off and on (delta small enough to adjust some rows), mu equal to the policy (c = 10: neither clip acts) and
    far from it (c = 1.5: rho_bar, the truncation and the bias correction all act); padding in every buffer; a terminal
    window is launched with and without its bootstrap row."""
    adjusted = 0
    for far in (False, True):
        Q, z, za, mu, actions, rewards = _window(T, A, T * 100 + A, far)
        c = 1.5 if far else 10.0
        for game_over, beta, trust in [(g, b, t) for g in (False, True) for b in (0.0, 0.01) for t in (False, True)]:
            what = "T %d A %d far %d game_over %d beta %g trust %d" % (T, A, far, game_over, beta, trust)
            kw = dict(c=c, delta=1e-4, beta=beta, trust=trust)
            k = _launch(rlx, dev, Q, z, za, mu, actions, rewards, game_over, **kw)
            r = R.window_loss(Q, z, za, mu, actions, rewards, game_over, 0.99, **kw)
            assert k["status"] == 0
            _assert_bit_equal(k, r, what)
            assert np.all(k["dQ"][T] == 0) and np.all(k["dlogits"][T] == 0) and np.any(k["dQ"][:T] != 0)
            assert A == 1 or np.any(k["dlogits"][:T] != 0)
            adjusted += int(np.any(r["adj"] > 0))
            if game_over:
                bare = _launch(rlx, dev, Q[:T], z[:T], za, mu, actions, rewards, True, **kw)
                assert bare["status"] == 0 and k["boot"] == 0 == bare["boot"]
                assert all(np.asarray(bare[n]).tobytes() == np.asarray(k[n])[:T].tobytes() for n in ("dQ", "dlogits"))
                assert _same(bare, k, ARRAYS[:6] + R.SCALARS), what
        if far and A > 1 and T >= 63:
            assert np.any(r["rho_i"] > 1) and np.any(r["rho_i"] < 1) and np.any(r["rho"] > c)
    assert A == 1 or T < 63 or adjusted > 0
    # the optional matrix changes nothing else, and a second launch gives the same bits
    again = _launch(rlx, dev, Q, z, za, mu, actions, rewards, True, **kw)
    bare = _launch(rlx, dev, Q, z, za, mu, actions, rewards, True, with_td=False, **kw)
    assert _same(again, k) and _same(bare, k, tuple(n for n in ARRAYS if n != "td_targets") + R.SCALARS)


def test_kernel_on_the_golden_cases_gives_the_reference_agents_values(rlx, dev, golden):
    """what the reference's own ACERAgent._learn_from_batch fed to train_and_sync_networks (and logged as 'Values'),
    bit for bit, from the recorded stand-in networks' Q values and the logits behind their probabilities"""
    z = golden("acer")
    for c in (fixture_case(z, k) for k in range(int(z["n_cases"]))):
        k = _launch(rlx, dev, np.concatenate([c["q_online"], c["q_boot"]]), np.concatenate([c["logits"], c["logits_boot"]]),
                    c["avg_logits"], c["mu"], c["actions"], c["rewards"], c["game_over"], c["discount"])
        assert k["status"] == 0
        for mine, theirs in (("rho", "output_1_1"), ("rho_i", "output_1_2"), ("td_targets", "output_1_3"),
                             ("q_retrace", "output_1_4"), ("avg", "output_1_5"), ("V", "target_1"),
                             ("V", "values_signal")):
            assert np.array_equal(BITS32(k[mine]), BITS32(c[theirs])), (mine, theirs)


@pytest.mark.parametrize("T,A", [(1, 2), (65, 8), (300, 18)])
def test_given_mode_equals_the_computed_mode_bit_for_bit(rlx, dev, T, A):
    """RLX_ACER_TARGETS_GIVEN: the window's arrays are inputs; the average network's logits, mu, the rewards and the
    game-over flag are absent; with and without the aliased matrix; a bootstrap row is carried along with zero rows"""
    Q, z, za, mu, actions, rewards = _window(T, A, 7 * T + A)
    for trust in (False, True):
        kw = dict(c=1.5, delta=1e-4, beta=0.01, trust=trust)
        k = _launch(rlx, dev, Q, z, za, mu, actions, rewards, False, **kw)
        for give_td in (True, False):
            g = _launch(rlx, dev, Q, z, None, None, actions, None, None, given=k, give_td=give_td, **kw)
            assert g["status"] == 0
            assert _same(g, k, tuple(n for n in ARRAYS if give_td or n != "td_targets") + R.SCALARS), (trust, give_td)
            short = _launch(rlx, dev, Q[:T], z[:T], None, None, actions, None, None, given=k, give_td=give_td, **kw)
            assert _same(short, k, R.SCALARS) and short["dlogits"].tobytes() == k["dlogits"][:T].tobytes()


@pytest.mark.parametrize("T,A", [(1, 2), (65, 6), (257, 18), (200, 1)])
def test_q_gradient_is_bit_identical_to_the_regression_loss_on_the_full_matrix(rlx, dev, T, A):
    """rlx_regression_loss fed the aliased target matrix under the Q head's weight: the same dQ bit for bit (the
    untouched columns give exactly zero), whatever the policy head's coefficients are (they are zeroed here: truncation
    0 removes the probability term, beta is 0); the loss scalars differ in the order of their sums only (LOSS)"""
    import torch
    Q, z, za, mu, actions, rewards = _window(T, A, T + A)
    k = _launch(rlx, dev, Q, z, za, mu, actions, rewards, False, c=0.0, pad=0)
    g = torch.full((T, A), float("nan"), dtype=torch.float32, device=dev)
    sc = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    rlx.regression_loss(_t(Q[:T], dev), A, _t(k["td_targets"], dev), A, None, T, A, 0, 0.5, 1.0, g, A, sc, 0)
    assert g.cpu().numpy().tobytes() == k["dQ"][:T].tobytes() and np.any(k["dQ"] != 0)
    np.testing.assert_allclose(float(sc.item()), k["q_loss"], **LOSS)
    assert k["probability_loss"] == 0


def test_out_of_range_actions_missing_bootstrap_row_and_bad_arguments(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    T, A = 5, 3
    Q, z, za, mu, _, rewards = _window(T, A, 2)
    actions = np.array([0, 3, 1, -1, 2])
    k = _launch(rlx, dev, Q, z, za, mu, actions, rewards, False, beta=0.01)
    r = R.window_loss(Q, z, za, mu, actions, rewards, False, 0.99, beta=0.01)
    assert k["status"] == R.STATUS_BAD_ACTION == r["status"]
    _assert_bit_equal(k, r)
    assert np.all(k["dQ"][[1, 3]] == 0) and np.all(k["dlogits"][[1, 3]] == 0) and np.any(k["dlogits"][0] != 0)
    assert np.array_equal(k["td_targets"][[1, 3]], Q[[1, 3]])
    e = (Q[[0, 2, 4], [0, 1, 2]] - k["q_retrace"][[0, 2, 4]]).astype(np.float64)
    np.testing.assert_allclose(k["q_loss"], 0.5 * np.sum(e * e) / 5, **LOSS)      # no term; the mean divides by T
    # the missing bootstrap row: status, and nothing is written (the outputs stay NaN: _launch asserts it)
    ok = [0, 1, 2, 0, 1]
    assert _launch(rlx, dev, Q[:T], z[:T], za, mu, ok, rewards, False)["status"] == R.STATUS_NO_BOOTSTRAP_ROW
    assert _launch(rlx, dev, Q[:T], z[:T], za, mu, ok, rewards, True)["status"] == 0
    f = torch.zeros(8, 32, dtype=torch.float32, device=dev)
    it = torch.zeros(8, dtype=torch.int32, device=dev)
    go = torch.ones(1, dtype=torch.uint8, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(T=4, A=2, rows=5, mode=0, ld=32, ld_q=None, ld_z=None, ld_az=None, ld_mu=None, ld_rho=None, ld_ap=None,
             ld_tt=None, ld_dq=None, ld_dz=None, q=f, z=f, za=f, mu=f, actions=it, rewards=f, game_over=go, V=f,
             rho=f, rho_i=f, avg=f, qret=f, boot=f, td=f, dq=f, dz=f, scalars=f, status=st):
        L = lambda v: ld if v is None else v
        rlx.acer_window_loss(q, L(ld_q), z, L(ld_z), rows, za, L(ld_az), mu, L(ld_mu), actions, rewards, game_over, T, A,
                             0.99, 10.0, 1.0, 0.0, 0.5, mode, V, rho, L(ld_rho), rho_i, avg, L(ld_ap), qret, boot, td,
                             L(ld_tt), dq, L(ld_dq), dz, L(ld_dz), scalars, status, 0)
    call()
    call(rows=4)
    call(td=None, ld_tt=0)
    call(mode=R.MODE_TARGETS_GIVEN | R.MODE_TRUST_REGION, za=None, mu=None, rewards=None, game_over=None, boot=None,
         ld_az=0, ld_mu=0)
    bad = [dict(T=0), dict(T=-1), dict(A=0), dict(A=19), dict(rows=3), dict(rows=6), dict(mode=4), dict(mode=-1)]
    bad += [{n: 1} for n in ("ld_q", "ld_z", "ld_az", "ld_mu", "ld_rho", "ld_ap", "ld_tt", "ld_dq", "ld_dz")]
    bad += [{n: None} for n in ("q", "z", "za", "mu", "actions", "rewards", "game_over", "V", "rho", "rho_i", "avg",
                                "qret", "boot", "dq", "dz", "scalars", "status")]
    for kw in bad:
        with pytest.raises(RlxError):
            call(**kw)
    torch.cuda.synchronize()
    assert int(st.item()) == 0


# ------------------------------------------------------------------------------------ the network
def _oracle_for(net, obs_shape, lr, eps):
    """the oracle's DQN chain (embedder, middleware, one Dense head = the Q head) on the network's weights, with a second
    Dense head (the policy head) on the same torso registered for the norm and the Adam step"""
    from oracle import nn as N
    from oracle.agents import DQNOracle
    arrays = net.params.named_arrays()
    o = DQNOracle(arrays, obs_shape, net.A, lr=lr, eps=eps)
    pn = "main/acer_policy_head/fc"
    o.pi_head = N.Dense(arrays[pn + "/kernel"][0].copy(), arrays[pn + "/bias"][0].copy())
    o.chains.append(("ph", 0, N.Chain([o.pi_head])))
    o.names[("ph", 0)] = [pn]
    return o


def test_network_update_equals_the_composed_oracle(dev):
    """ACERNet.train_window: the online forward on T + 1 rows, the average network's policy head on T, the window launch,
    both heads and the torso backward, the gradients REPLACING the buffer, one Adam step, the average network's move —
    for four windows (bootstrapped and terminal) — against oracle layers + TF1 Adam + the restatement, in the manner and
    at the tolerances of test_a3c.py::test_network_update_equals_the_composed_oracle.  The average network's logits are
    the device's own (its weights are a mix no oracle holds).  After every update the average network equals what the
    existing soft update gives from the old average and the new online weights, and differs from the online one."""
    import torch
    from coach_amd.nn.networks import ACERNet
    from oracle import nn as N
    from tolerances import OUT, WEIGHTS
    rng = np.random.RandomState(7)
    A, lr = 2, 5e-4
    net = ACERNet(dev, (4,), A, learning_rate=lr, optimizer_epsilon=1e-4, importance_weight_truncation=1.5, seed=3)
    names = net.params.entries
    assert "main/acer_policy_head/fc/kernel" in names and "main/q_head/dense/kernel" in names
    assert net.target is not None and net.clip_gradients == 40.0 and torch.equal(net.target, net.params.weights)
    o = _oracle_for(net, (4,), lr, 1e-4)
    for T, game_over in ((9, False), (1, True), (37, False), (6, True)):
        obs = rng.randn(T + 1, 4).astype(np.float32)
        actions = rng.randint(0, A, size=T)
        rewards = rng.uniform(-1, 2, size=T).astype(np.float32)
        mu = pg_ref.head_rows((1.5 * rng.randn(T, A)).astype(np.float32))[0]
        w0, t0, steps0 = net.params.weights.clone(), net.target.clone(), net.adam_steps
        avg_z = net.average_policy_values(_t(obs, dev), T, tag="test_avg").clone().cpu().numpy()
        loss = net.train_window(_t(obs, dev), T, True, _t(actions.astype(np.int32), dev), _t(mu, dev), _t(rewards, dev),
                                _t(np.array([int(game_over)], np.uint8), dev), 0.99, rate=0.01)
        feat = o.tower.forward(N.prep_obs(obs, False))
        q, z = o.head.forward(feat).astype(np.float32), o.pi_head.forward(feat).astype(np.float32)
        r = R.window_loss(q, z, avg_z, mu, actions, rewards, game_over, 0.99, c=1.5)
        o.tower.backward(o.head.backward(r["dQ"]) + o.pi_head.backward(r["dlogits"]))
        np.testing.assert_allclose(net.q_online.cpu().numpy(), q, **OUT)
        np.testing.assert_allclose(net.window["V"].cpu().numpy(), r["V"], **OUT)
        np.testing.assert_allclose(net.window["q_retrace"].cpu().numpy(), r["q_retrace"], **OUT)
        np.testing.assert_allclose(net.scalars.cpu().numpy(), [r[n] for n in R.SCALARS], **LOSS)
        assert float(loss.item()) == float(net.scalars[0].item())
        np.testing.assert_allclose(float(net.norm.item()), o.global_norm(), **LOSS)
        assert o.global_norm() < 40.0                                # (nothing is clipped in this test)
        # the gradients replaced the buffer, were applied at once, and the buffer keeps them
        assert torch.equal(net.accumulated, net.params.grads) and net.accumulated.abs().sum() > 0
        assert net.adam_steps == steps0 + 1 and not torch.equal(net.params.weights, w0)
        o.apply_summed_gradients([o.snapshot_grads()], 1, False)
        w = net.params.named_arrays()
        wo = o.weights()
        assert set(wo) == set(w)
        for name, towers in wo.items():
            np.testing.assert_allclose(w[name][0], towers[0], err_msg=name, **WEIGHTS)
        expect = t0.clone()
        net.lib.mix_weights(expect, net.params.weights, net.params.size, 0.01, net.ctx.stream)
        assert torch.equal(net.target, expect) and not torch.equal(net.target, net.params.weights)
        assert not torch.equal(net.target, t0)
    # the base's apply step: the last window's gradients once more, then cleared
    w1, g = net.params.weights.clone(), net.accumulated.clone()
    net.apply_accumulated()
    assert net.adam_steps == 5 and not net.accumulated.any() and g.any() and not torch.equal(net.params.weights, w1)
    net.check_status()
    assert torch.isfinite(net.params.weights).all()


def test_backend_interface_serves_the_acer_network(dev):
    """Architecture.predict / accumulate_gradients through a NetworkWrapper, fed the way ACERAgent._learn_from_batch
    feeds it (acer_agent.py:157-165), against the same network driven directly in the GIVEN mode"""
    import torch
    from coach_amd.agents.acer_agent import ACERAgentParameters
    from coach_amd.architectures.hip_architecture import ACERArchitecture
    from coach_amd.architectures.network_wrapper import NetworkWrapper
    from coach_amd.nn.networks import ACERNet, acer_net_kwargs
    from coach_amd.spaces import BoxActionSpace, DiscreteActionSpace, ObservationSpace, SpacesDefinition, StateSpace
    from tolerances import OUT
    ap = ACERAgentParameters()
    ap.seed = 5
    A = 3
    spaces = SpacesDefinition(StateSpace({"observation": ObservationSpace((6,))}), None, DiscreteActionSpace(A))
    nw = NetworkWrapper(ap, has_target=True, has_global=False, name="main", spaces=spaces, worker_device=dev)
    online = nw.online_network
    assert isinstance(online, ACERArchitecture) and isinstance(nw.target_network, ACERArchitecture)
    twin = ACERNet(dev, (6,), A, **acer_net_kwargs(ap.network_wrappers["main"], ap.algorithm, 5))
    assert twin.q_loss_weight == 0.5 and twin.clip_gradients == 40.0 and not twin.trust_region
    assert torch.equal(twin.params.weights, online.net.params.weights)
    rng = np.random.RandomState(1)
    T = 7
    obs = rng.randn(T, 6).astype(np.float32)
    q, probs = online.predict({"observation": obs})
    q2, z2 = twin.predict(_t(obs, dev), T)
    assert q.shape == (T, A) and probs.shape == (T, A) and np.array_equal(q, q2.cpu().numpy())
    np.testing.assert_allclose(probs, pg_ref.head_rows(z2.cpu().numpy())[0], **OUT)
    tq, tprobs = nw.target_network.predict({"observation": obs})
    np.testing.assert_allclose(tprobs, probs, **OUT)                  # the average network starts as a copy
    # the agent's arithmetic on the host, as the reference does it
    actions, rewards = rng.randint(0, A, size=T), rng.uniform(-1, 2, size=T).astype(np.float32)
    mu = pg_ref.head_rows(rng.randn(T, A).astype(np.float32))[0]
    w = R.window_values(q, probs, mu, actions, rewards, True, 0.99)
    inputs = {"observation": obs, "output_1_0": actions, "output_1_1": w["rho"], "output_1_2": w["rho_i"],
              "output_1_3": w["td_targets"], "output_1_4": w["q_retrace"], "output_1_5": tprobs}
    heads = online.output_heads[1]
    res = online.accumulate_gradients(inputs, [w["td_targets"], w["V"]], additional_fetches=[
        heads.probability_loss, heads.bias_correction_loss, heads.kl_divergence])
    total_loss, losses, norm, fetched = res[:4]
    given = dict(V=_t(w["V"], dev), rho=_t(w["rho"], dev), rho_i=_t(w["rho_i"], dev), avg_policy=_t(tprobs, dev),
                 q_retrace=_t(w["q_retrace"], dev), td_targets=_t(w["td_targets"], dev))
    twin.window_gradients(_t(obs, dev), T, False, _t(actions.astype(np.int32), dev), given=given)
    assert total_loss == float(twin.loss.item()) and norm == float(twin.norm.item()) and norm > 0
    assert losses == [float(twin.q_loss.item()), float(twin.policy_loss.item())]
    assert fetched == [float(twin.probability_loss.item()), float(twin.bias_correction_loss.item()),
                       float(twin.kl_divergence.item())]
    r = R.head_losses(q, z2.cpu().numpy(), tprobs, w["rho"], w["rho_i"], w["q_retrace"], w["V"], w["td_targets"], actions)
    np.testing.assert_allclose(total_loss, r["loss"], **LOSS)
    with pytest.raises(ValueError, match="aliases"):
        online.accumulate_gradients(inputs, [q, w["V"]])
    with pytest.raises(ValueError, match="only discrete action spaces"):
        box = SpacesDefinition(StateSpace({"observation": ObservationSpace((6,))}), None,
                               BoxActionSpace(2, low=-1.0, high=1.0))
        NetworkWrapper(ap, has_target=True, has_global=False, name="main", spaces=box, worker_device=dev)


# -------------------------------------------------------------------------------------- the agent
def _agent(dev, n_env, t_max, seed=3, start_replay=60, ratio=2):
    from coach_amd.agents.acer_agent import ACERAgent, ACERAgentParameters
    from coach_amd.core_types import RunPhase
    from coach_amd.environments.cartpole_vector_environment import (
        CartPoleVectorEnvironment, CartPoleVectorEnvironmentParameters)
    from coach_amd.memories.memory import MemoryGranularity
    p = ACERAgentParameters()
    p.seed = seed
    p.algorithm.num_steps_between_gradient_updates = t_max
    p.algorithm.reward_rescale = 1 / 200.
    p.algorithm.num_transitions_to_start_replay = start_replay
    p.algorithm.ratio_of_replay = ratio
    p.memory.max_size = (MemoryGranularity.Transitions, 150)
    env = CartPoleVectorEnvironment(CartPoleVectorEnvironmentParameters(n_env, "CartPole-v0", seed=11), dev)
    agent = ACERAgent(p, env, dev)
    agent.phase = env.phase = RunPhase.TRAIN
    agent.debug_windows, agent.debug_targets = [], []
    return agent


def _run(agent, episodes, monkeypatch, limit=4000):
    """act() + train() until `episodes` episodes finished -> per env the finished episodes' lengths; per env and episode
    the acting probabilities of every step; per train() call what it did"""
    net, n = agent.networks["main"], agent.n_env
    lengths, probs, calls, done = [[] for _ in range(n)], [[[]] for _ in range(n)], [], 0
    draws, poisson = [], np.random.poisson

    def recording_poisson(lam):
        draws.append(int(poisson(lam)))
        return draws[-1]
    monkeypatch.setattr(np.random, "poisson", recording_poisson)
    for _ in range(limit):
        agent.act()
        p = agent.action_probabilities.cpu().numpy().copy()
        for e in range(n):
            probs[e][-1].append(p[e])
        if agent._episode_just_ended:
            for e, L in zip(np.nonzero(agent._episode_steps == 0)[0], agent.ended_episode_lengths):
                lengths[e].append(int(L))
                assert len(probs[e][-1]) == int(L)
                probs[e].append([])
                done += 1
        held, n0, t0, s0, d0 = agent.replay.num_transitions(), len(agent.debug_windows), len(agent.debug_targets), \
            net.adam_steps, len(draws)
        agent.train()
        calls.append(dict(windows=agent.debug_windows[n0:], targets=agent.debug_targets[t0:], held=held,
                          adam_steps=net.adam_steps - s0, draws=draws[d0:], accumulated=bool(net.accumulated.any())))
        if done >= episodes:
            break
    agent.check_status()
    return lengths, probs, calls


def _assert_windows_are_the_restatement(agent, calls, probs):
    """every window — replayed ones included — has the restatement's V, rho, q_retrace and aliased matrix, bit for bit,
    fed the device's own network outputs and stored mu; an on-policy window's mu rows are its acting steps' probabilities"""
    reward = np.float32(1.0) * np.float32(1 / 200.)
    threshold, n_on, n_replay = agent.ap.algorithm.num_transitions_to_start_replay, 0, 0
    episode_of = [0] * agent.n_env                   # which of its episodes an env's next window belongs to
    for c in calls:
        on = [t for t in c["targets"] if t["kind"] == "on-policy"]
        rep = [t for t in c["targets"] if t["kind"] == "replay"]
        assert len(on) == len(c["windows"])
        # replay starts only once the memory passes the threshold, and runs exactly the drawn number of windows.  (The
        # memory can only grow within a call: `held` is its size before the call's first window.)
        assert len(rep) == sum(c["draws"]) and len(c["draws"]) <= len(on)
        assert len(c["draws"]) == (len(on) if c["held"] > threshold else 0)
        # the Adam steps: one per window, plus the repeated application of the last window's gradients
        assert c["adam_steps"] == len(on) + len(rep) + sum(1 for w in c["windows"] if w[4])
        if c["windows"]:
            assert c["accumulated"] == (not c["windows"][-1][4])
        for t in c["targets"]:
            T = t["T"]
            q, z, mu = (t[k].cpu().numpy() for k in ("q", "logits", "mu"))
            assert q.shape == (T + 1, agent.A) and np.isfinite(q).all()
            P = pg_ref.head_rows(z)[0]
            go = bool(t["game_over"].item())
            rewards = t["rewards"].cpu().numpy()
            assert np.all(rewards == reward)
            w = R.window_values(q[:T], P[:T], mu, t["actions"].cpu().numpy(), rewards, go, 0.99,
                                R.bootstrap_value(q[T], P[T]))
            for mine, theirs in (("V", "V"), ("rho", "rho"), ("rho_i", "rho_i"), ("q_retrace", "q_retrace"),
                                 ("td_targets", "td_targets")):
                assert np.array_equal(BITS32(t[theirs].cpu().numpy()), BITS32(w[mine])), (t["kind"], mine)
            n_replay += t["kind"] == "replay"
        for (env, start, end, *_), t in zip(c["windows"], on):
            n_on += 1
            want = np.stack(probs[env][episode_of[env]][start:end])
            assert np.array_equal(BITS32(t["mu"].cpu().numpy()), BITS32(want)), (env, start, end)
            if bool(t["game_over"].item()):          # the window ended its episode (CartPole reports its limit as one)
                episode_of[env] += 1
    return n_on, n_replay


@pytest.mark.parametrize("t_max", [5, 5000])
def test_agent_with_one_env_keeps_the_base_cadence_and_replays_the_drawn_windows(dev, monkeypatch, t_max):
    """windows, pointers, current_episode, training_iteration and the apply cadence are the on-policy base's (pg_ref.run,
    pinned to the reference by PG's fixture); replay, Adam steps, mu and every window's values as stated above"""
    agent = _agent(dev, 1, t_max)
    lengths, probs, calls = _run(agent, 12, monkeypatch)
    ws = pg_ref.run([np.zeros(L, np.float32) for L in lengths[0]], 0.99, pg_ref.FUTURE_RETURN, 200, t_max, 5)
    got = agent.debug_windows
    assert [(s, e, ce, ap) for _, s, e, ce, ap in got] == \
        [(w["start"], w["end"], w["current_episode"], w["applied"]) for w in ws]
    assert agent.training_iteration == len(ws) == ws[-1]["training_iteration"] and agent.current_episode == 12
    assert any(ap for *_, ap in got) and not all(ap for *_, ap in got)
    n_on, n_replay = _assert_windows_are_the_restatement(agent, calls, probs)
    assert n_on == len(ws) and n_replay == agent.replayed_windows > 0
    on = [t for c in calls for t in c["targets"] if t["kind"] == "on-policy"]
    assert [bool(t["game_over"].item()) for t in on] == [w["complete"] for w in ws]
    # the replay holds whole episodes, the newest that fit max_size, and evaluation or heat-up wrote nothing else
    keep = len(lengths[0])
    while sum(lengths[0][-keep:]) > 150:
        keep -= 1
    assert [m for _, m in agent.replay.episodes] == lengths[0][len(lengths[0]) - keep:]
    assert any(c["held"] <= 60 and c["windows"] for c in calls) and any(c["draws"] for c in calls)
    replayed = [t for c in calls for t in c["targets"] if t["kind"] == "replay"]
    assert all(t["T"] <= t_max for t in replayed) and (t_max != 5 or any(t["T"] == 5 for t in replayed))


def test_agent_with_three_envs_shares_one_replay_in_completion_order(dev, monkeypatch):
    agent = _agent(dev, 3, 5, seed=4)
    lengths, probs, calls = _run(agent, 15, monkeypatch)
    got = agent.debug_windows
    for e in range(3):
        eps = lengths[e] + [200]
        ws = pg_ref.run([np.zeros(L, np.float32) for L in eps], 0.99, pg_ref.FUTURE_RETURN, 200, 5, 5)
        mine = [(s, t) for env, s, t, *_ in got if env == e]
        assert mine == [(w["start"], w["end"]) for w in ws][:len(mine)] and len(mine) >= len(lengths[e])
    for c in calls:
        envs = [w[0] for w in c["windows"]]
        assert envs == sorted(envs) and len(set(envs)) == len(envs)
    assert agent.training_iteration == len(got) and agent.current_episode == sum(len(x) for x in lengths)
    n_on, n_replay = _assert_windows_are_the_restatement(agent, calls, probs)
    assert n_on == len(got) and n_replay == agent.replayed_windows > 0
    total = sum(sum(x) for x in lengths)
    assert agent.replay.num_transitions() <= 150 < total


def test_cartpole_acer_preset_builds_and_runs_400_steps(dev, tmp_path):
    """nothing about learning is asserted (the recorded validation runs are in DESIGN.md): the preset builds, trains for
    400 vector steps with finite weights, replays once its memory holds enough (the threshold is lowered to 100
    transitions for that), and ACER's signals reach the CSV"""
    import importlib
    import torch
    from coach_amd.core_types import EnvironmentSteps, RunPhase
    gm = importlib.import_module("coach_amd.presets.CartPole_ACER").make()
    gm.agent_params.algorithm.num_transitions_to_start_replay = 100
    gm.schedule.improve_steps = EnvironmentSteps(400)
    gm.schedule.steps_between_evaluation_periods = EnvironmentSteps(200)
    gm.device = dev
    gm.logger.__init__(str(tmp_path / "acer.csv"))
    rows = gm.improve()
    a = gm.agent
    assert type(a).__name__ == "ACERAgent" and gm.total_steps_counters[RunPhase.TRAIN] == 400
    assert a.training_iteration >= 80 and sum(r.get("Evaluation Reward", "") != "" for r in rows) == 2
    assert a.replayed_windows > 0 and a.replay.num_transitions() > 100
    net = a.networks["main"]
    assert net.adam_steps >= a.training_iteration + a.replayed_windows
    gm.environment.check_status()
    a.check_status()
    assert torch.isfinite(net.params.weights).all() and not torch.equal(net.target, net.params.weights)
    header = (tmp_path / "acer.csv").read_text().splitlines()[0].split(",")
    for name in ("Q Loss", "Policy Loss", "Probability Loss", "Bias Correction Loss", "Values", "KL Divergence",
                 "Entropy", "Loss", "Grads (unclipped)", "Discounted Return"):
        assert name + "/Mean" in header, name
        values = [r[name + "/Mean"] for r in rows if r.get(name + "/Mean", "") != ""]
        assert values and np.isfinite(np.asarray(values, dtype=np.float64)).all(), name
