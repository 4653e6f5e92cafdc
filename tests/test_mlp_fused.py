"""rlx_mlp_dqn_update (csrc/mlp_fused.hip): the ONE-launch DQN update of an MLP Q network against (a) the
layer-by-layer device path it replaces and (b) the numpy oracle of DQNAgent.learn_from_batch
(oracle.agents.DQNOracle, pinned to the reference's own learn_from_batch by tests/golden/updates.npz /
loop.npz).  Same weights, same batches: losses, |TD errors|, gradient norms and the weights after several
updates must agree to fp32 accumulation noise (the two device paths sum in different orders)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _net(dev, dims, A, huber, fused):
    from coach_amd.nn.networks import DQNNet
    d0, h1, h2 = dims
    net = DQNNet(dev, (d0,), A, embedder=[h1], middleware=[h2], learning_rate=1e-3,
                 replace_mse_with_huber_loss=huber, seed=4)
    if not fused:
        net._fused = None
    else:
        assert net._fused is not None
    return net


@pytest.mark.parametrize("dims,A,B,huber,ddqn,per", [
    ((4, 256, 512, ), 2, 32, False, False, False),       # BASELINE C1 (CartPole_DQN preset network)
    ((4, 256, 512, ), 2, 32, True, True, True),
    ((8, 96, 96, ), 5, 20, True, False, True),            # ragged batch, 3 workgroups
    ((15, 128, 64, ), 3, 7, False, True, False),          # odd obs dim, 2 workgroups
])
def test_fused_update_matches_layerwise_and_oracle(dev, dims, A, B, huber, ddqn, per):
    import torch
    from oracle.agents import DQNOracle
    fused, plain = _net(dev, dims, A, huber, True), _net(dev, dims, A, huber, False)
    assert torch.equal(fused.params.weights, plain.params.weights)
    orc = DQNOracle(plain.params.named_arrays(), (dims[0],), A, "relu", 1e-3, 0.9, 0.99, 1e-4, huber)
    rng = np.random.RandomState(B + A)
    td = {k: torch.zeros(B, dtype=torch.float64, device=dev) for k in "fp"}
    for it in range(4):
        s = rng.randn(B, dims[0]).astype(np.float32)
        s2 = rng.randn(B, dims[0]).astype(np.float32)
        a = rng.randint(0, A, B).astype(np.int32)
        r = rng.randn(B).astype(np.float32)
        done = (rng.rand(B) < 0.2)
        w = (rng.rand(B) + 0.1) if per else None
        dv = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dt)
        args = (dv(s, torch.float32), dv(s2, torch.float32), B, dv(a, torch.int32), dv(r, torch.float32),
                dv(done.astype(np.uint8), torch.uint8), 0.97)
        res = {}
        for k, net in (("f", fused), ("p", plain)):
            loss = net.learn_from_batch(*args, importance_weights=None if w is None else dv(w, torch.float64),
                                        td_errors=td[k], double_dqn=ddqn)
            net.check_status()
            res[k] = (float(loss.item()), float(net.norm.item()))
        ref = orc.learn_from_batch(s, s2, a, r, done, 0.97, None if w is None else w.astype(np.float32), ddqn)
        np.testing.assert_allclose(res["f"][0], res["p"][0], rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(res["f"][1], res["p"][1], rtol=2e-4)
        np.testing.assert_allclose(td["f"].cpu().numpy(), td["p"].cpu().numpy(), rtol=1e-4, atol=2e-6)
        np.testing.assert_allclose(res["f"][0], ref["loss"], rtol=2e-4, atol=1e-7)
        np.testing.assert_allclose(td["f"].cpu().numpy(), ref["td_errors"], rtol=2e-3, atol=5e-6)
        if it == 1:
            fused.update_target(1.0); plain.update_target(1.0); orc.update_target(1.0)
    wf, wp, wo = fused.params.named_arrays(), plain.params.named_arrays(), orc.weights()
    for name in wf:
        np.testing.assert_allclose(wf[name][0], wp[name][0], rtol=0, atol=2e-5, err_msg=name)
        np.testing.assert_allclose(wf[name][0], wo[name][0], rtol=0, atol=5e-5, err_msg=name)
    assert torch.allclose(fused.adam.state, plain.adam.state)
    assert int(fused._fused["sync"].abs().sum().item()) == 0          # barrier words re-armed


@pytest.mark.parametrize("ddqn", [False, True])
def test_fused_update_selects_a_nan_of_the_target_net_like_the_layerwise_path(dev, ddqn):
    """A NaN in one element (column 1) of the target tower's last bias: Q_target(s', 1) is NaN in every row.  DQN: np.argmax
    takes the first NaN, so every row's target, every |TD error| and the loss are NaN -- a loop that asks `q > best` skips
    the NaN and trains on with finite targets.  DDQN: the online net selects, and exactly the rows it sends to column 1
    are NaN.  The one-launch update and the layer-by-layer path (rlx_dqn_head_loss_backward) agree on which values are
    NaN, and to the usual accumulation noise on the others."""
    import torch
    dims, A, B = (8, 96, 96), 5, 20
    fused, plain = _net(dev, dims, A, True, True), _net(dev, dims, A, True, False)
    for net in (fused, plain):
        name = [n for n in net.params.entries if n.endswith("bias")][-1]
        bias = net.params.w(name, 0, buf=net.target)
        assert tuple(bias.shape) == (A,), (name, bias.shape)
        bias[1] = float("nan")
    rng = np.random.RandomState(3)
    dv = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dt)
    s2 = dv(rng.randn(B, dims[0]).astype(np.float32), torch.float32)
    args = (dv(rng.randn(B, dims[0]).astype(np.float32), torch.float32), s2, B, dv(rng.randint(0, A, B), torch.int32),
            dv(rng.randn(B).astype(np.float32), torch.float32), dv(rng.rand(B) < 0.2, torch.uint8), 0.97)
    to_column_1 = (plain.q_values(s2, B).data.view(B, A).argmax(1) == 1).cpu().numpy() if ddqn else np.ones(B, dtype=bool)
    td, loss = {}, {}
    for k, net in (("f", fused), ("p", plain)):
        td[k] = torch.zeros(B, dtype=torch.float64, device=dev)
        loss[k] = float(net.learn_from_batch(*args, td_errors=td[k], double_dqn=ddqn).item())
        net.check_status()
        td[k] = td[k].cpu().numpy()
        assert np.array_equal(np.isnan(td[k]), to_column_1), (k, td[k])
    assert np.isnan(loss["f"]) == np.isnan(loss["p"]) == bool(to_column_1.any())
    np.testing.assert_allclose(td["f"][~to_column_1], td["p"][~to_column_1], rtol=1e-4, atol=2e-6)
    if not ddqn:                                # every value is NaN: the two paths agree bit for bit in the only sense there is
        assert np.isnan(td["f"]).all() and np.isnan(td["p"]).all() and np.isnan(loss["f"]) and np.isnan(loss["p"])


def _nan_in_b1(net):
    name = [n for n in net.params.entries if n.endswith("bias")][0]
    for buf in (net.params.weights, net.target):
        net.params.w(name, 0, buf=buf)[3] = float("nan")


def test_fused_update_keeps_a_nan_of_the_first_bias_like_the_layerwise_path(dev):
    """A NaN in one element of b1, online and target, at the smallest sizes rlx_mlp_dqn_supported accepts: unit 3 of the
    first layer is NaN in every row after np.maximum(z, 0), so every Q value, every target, every |TD error| and the loss
    are NaN on the layer-by-layer path (rlx_gemm's epilogue).  The one-launch update agrees (v > 0 ? v : 0 made the unit 0 and
    trained on with finite values)."""
    import torch
    from coach_amd import _rlx
    dims, A, B = (1, 32, 32), 1, 1
    lib = _rlx.lib()
    assert lib.rlx_mlp_dqn_supported(B, *dims, A) and not lib.rlx_mlp_dqn_supported(B, dims[0], 31, 32, A) \
        and not lib.rlx_mlp_dqn_supported(B, dims[0], 32, 31, A) and not lib.rlx_mlp_dqn_supported(B - 1, *dims, A)
    fused, plain = _net(dev, dims, A, True, True), _net(dev, dims, A, True, False)
    rng = np.random.RandomState(3)
    dv = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dt)
    args = (dv(rng.randn(B, dims[0]).astype(np.float32), torch.float32), dv(rng.randn(B, dims[0]).astype(np.float32), torch.float32),
            B, dv(rng.randint(0, A, B), torch.int32), dv(rng.randn(B).astype(np.float32), torch.float32),
            dv(np.zeros(B), torch.uint8), 0.97)
    for k, net in (("f", fused), ("p", plain)):
        _nan_in_b1(net)
        td = torch.zeros(B, dtype=torch.float64, device=dev)
        loss = float(net.learn_from_batch(*args, td_errors=td).item())
        print(k, "loss", loss, "|TD|", td.cpu().numpy())
        assert np.isnan(td.cpu().numpy()).all() and np.isnan(loss), k


def test_fused_q_act_keeps_a_nan_of_the_first_bias_like_the_layer_launches(dev):
    """rlx_mlp_q_act at the smallest sizes rlx_mlp_q_act_supported accepts, one NaN in b1: Q(s) is NaN exactly where the
    layer launches' Q(s) is (everywhere: the NaN unit feeds every unit of the second layer)."""
    import torch
    from coach_amd import _rlx
    from coach_amd.nn.networks import DQNNet
    (d0, h1, h2), A, n_env = (1, 4, 4), 1, 1
    lib = _rlx.lib()
    assert not lib.rlx_mlp_q_act_supported(n_env, d0, 3, h2, A) and not lib.rlx_mlp_q_act_supported(n_env, d0, h1, 3, A)
    net = DQNNet(dev, (d0,), A, embedder=[h1], middleware=[h2], learning_rate=1e-3, seed=3)
    assert net.can_act_fused(n_env)
    s = torch.from_numpy(np.random.RandomState(1).randn(n_env, d0).astype(np.float32)).to(dev)
    q = lambda: torch.zeros(n_env, A, dtype=torch.float32, device=dev)
    clean, got = q(), q()
    net.q_act(s, n_env, None, None, None, 0.0, clean, None)
    _nan_in_b1(net)
    net.q_act(s, n_env, None, None, None, 0.0, got, None)
    ref = net.q_values(s, n_env, tag="ref").data.view(n_env, A)
    assert not bool(clean.isnan().any()) and bool(ref.isnan().all())
    assert torch.equal(got.isnan(), ref.isnan())


def test_fused_update_is_reproducible(dev):
    """fixed summation orders: two runs from the same state give bit-identical weights."""
    import torch
    outs = []
    for _ in range(2):
        net = _net(dev, (4, 256, 512), 2, False, True)
        rng = np.random.RandomState(0)
        td = torch.zeros(32, dtype=torch.float64, device=dev)
        for it in range(3):
            t = lambda x, dt: torch.from_numpy(x).to(dev).to(dt)
            net.learn_from_batch(t(rng.randn(32, 4).astype(np.float32), torch.float32),
                                 t(rng.randn(32, 4).astype(np.float32), torch.float32), 32,
                                 t(rng.randint(0, 2, 32).astype(np.int32), torch.int32),
                                 t(rng.randn(32).astype(np.float32), torch.float32),
                                 t((rng.rand(32) < 0.1).astype(np.uint8), torch.uint8), 0.99, td_errors=td)
        outs.append((net.params.weights.clone(), td.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
