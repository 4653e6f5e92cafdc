"""PPOActorNet / PPOCriticNet (coach_amd/nn/networks.py): one value minibatch and policy minibatches — forward, the head
launch of csrc/ppo_kl.hip, backward, one Adam step — against oracle layers + TF1 Adam composed with the restatement
tests/ppo_kl_ref.py, in the manner and at the tolerances (tests/tolerances.py) of
test_pg.py::test_network_update_equals_the_composed_oracle; the running fetch sums and the coefficient update on the
device bit for bit the restatement's on the device's own scalars."""
import numpy as np
import pytest

import head_loss_ref as H
import ppo_kl_ref as R
from tolerances import LOSS, OUT, WEIGHTS

F32 = np.float32
pytestmark = pytest.mark.gpu
SCHEME = dict(embedder=[16], middleware=[16])
B = 64


def _t(x, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _oracle_for(net, head, obs_shape, n_out, lr):
    """the oracle's chain (embedder, middleware, one Dense head) on the network's weights, tanh as the PPO networks"""
    from oracle.agents import DQNOracle
    arrays = {k.replace(head, "main/q_head/dense"): v for k, v in net.params.named_arrays().items()
              if not k.endswith("policy_log_std")}
    return DQNOracle(arrays, obs_shape, n_out, activation="tanh", lr=lr, eps=1e-4)


def _weights_match(net, o, head):
    w = net.params.named_arrays()
    for name, towers in o.weights().items():
        np.testing.assert_allclose(w[name.replace("main/q_head/dense", head)][0], towers[0], err_msg=name, **WEIGHTS)


def _perturbed(rng, probs, scale):
    o = np.exp(np.log(probs.astype(np.float64)) + scale * rng.randn(*probs.shape))
    return (o / o.sum(axis=1, keepdims=True)).astype(F32)


def test_critic_minibatch_equals_the_composed_oracle(dev):
    import torch
    from coach_amd.nn.networks import PPOCriticNet
    rng = np.random.RandomState(11)
    lr = 5e-4
    net = PPOCriticNet(dev, (4,), learning_rate=lr, seed=5, **SCHEME)
    assert "main/v_head/dense/kernel" in net.params.entries and torch.equal(net.target, net.params.weights)
    o = _oracle_for(net, "main/v_head/dense", (4,), 1, lr)
    w0 = net.params.weights.clone()
    for step in range(2):
        obs = rng.randn(B, 4).astype(F32)
        targets = rng.randn(B).astype(F32)
        v = o.q(obs).astype(F32)
        np.testing.assert_allclose(net.values(_t(obs, dev), B).cpu().numpy(), v[:, 0], **OUT)
        ref = H.regression_loss(v, targets[:, None], None, "mse", 1.0, 1.0)
        o.tower.backward(o.head.backward(ref["grad"].astype(F32)))
        norm = o.global_norm()
        o.adam_step(1.0)
        loss = net.train_minibatch(_t(obs, dev), B, _t(targets, dev))
        np.testing.assert_allclose(float(loss.item()), ref["loss"], **LOSS)
        np.testing.assert_allclose(float(net.norm.item()), norm, **LOSS)
        _weights_match(net, o, "main/v_head/dense")
    assert torch.equal(net.target, w0)                                 # the target copy moves only with update_target
    obs = rng.randn(B, 4).astype(F32)
    v_target = net.values(_t(obs, dev), B, use_target=True).clone()
    assert not torch.equal(v_target, net.values(_t(obs, dev), B))
    net.update_target()
    assert torch.equal(net.target, net.params.weights)


def test_discrete_actor_minibatches_equal_the_composed_oracle(dev):
    """minibatch 0: the old policy is the target copy right after a sync (KL ~ 0, below the cutoff); minibatch 1: an old
    policy far from the new one (KL mean above the cutoff: the squared hinge's factor is in the gradient)"""
    import torch
    from coach_amd.nn.networks import PPOActorNet
    rng = np.random.RandomState(12)
    A, lr, beta, klc, target_kl, high = 3, 5e-4, 0.01, 1.0, 0.01, 1000.0
    net = PPOActorNet(dev, (4,), A, learning_rate=lr, beta_entropy=beta, target_kl_divergence=target_kl,
                      initial_kl_coefficient=klc, high_kl_penalty_coefficient=high, seed=6, **SCHEME)
    assert "main/ppo_head/policy_fc/kernel" in net.params.entries
    o = _oracle_for(net, "main/ppo_head/policy_fc", (4,), A, lr)
    sets, sides = [], []
    for step in range(2):
        obs = rng.randn(B, 4).astype(F32)
        actions = rng.randint(0, A, size=B).astype(np.int32)
        adv = rng.randn(B).astype(F32)
        old = net.policy_probs(_t(obs, dev), B, use_target=True).cpu().numpy().copy()
        np.testing.assert_allclose(net.policy_probs(_t(obs, dev), B).cpu().numpy(), H.softmax(o.q(obs).astype(F32))[0], **OUT)
        if step == 1:
            old = _perturbed(rng, old, 1.0)
        logits = o.q(obs).astype(F32)
        ref = R.ppo_kl_discrete_loss(logits, actions, adv, old, beta, klc, 2 * target_kl, high, True, 1.0)
        sides.append(ref["side"])
        o.tower.backward(o.head.backward(ref["dlogits"].astype(F32)))
        norm = o.global_norm()
        o.adam_step(1.0)
        scalars = net.train_minibatch(_t(obs, dev), B, _t(actions, dev), _t(adv, dev), _t(old, dev)).cpu().numpy().copy()
        net.check_status()
        np.testing.assert_allclose(scalars, ref["scalars"], **LOSS)
        np.testing.assert_allclose(float(net.norm.item()), norm, **LOSS)
        _weights_match(net, o, "main/ppo_head/policy_fc")
        sets.append(scalars)
    assert sides == ["below", "above"]
    sums = R.accumulate(sets)
    assert net.epoch_sums.cpu().numpy().tobytes() == sums.tobytes()
    net.update_kl_coefficient()
    want_c, want_kl = R.kl_coefficient_update(sums, target_kl, klc)
    assert net.kl_coefficient.cpu().numpy()[0].tobytes() == want_c.tobytes() and want_c == F32(1.5)
    assert net.kl_mean.cpu().numpy()[0].tobytes() == want_kl.tobytes()
    net.reset_epoch_sums()
    assert not net.epoch_sums.any() and torch.isfinite(net.params.weights).all()


def test_continuous_actor_minibatches_equal_the_composed_oracle(dev):
    """the Gaussian head: the mean layer and the torso through the oracle, the policy_log_std vector through the oracle's
    Adam on the restatement's dlog_std; minibatch 1 has an old policy far away (above the cutoff)"""
    from coach_amd.nn.networks import PPOActorNet
    rng = np.random.RandomState(13)
    A, lr, beta, klc, target_kl, high = 2, 5e-4, 0.01, 1.0, 0.01, 1000.0
    net = PPOActorNet(dev, (5,), A, learning_rate=lr, beta_entropy=beta, target_kl_divergence=target_kl,
                      initial_kl_coefficient=klc, high_kl_penalty_coefficient=high, seed=7, continuous=True, **SCHEME)
    o = _oracle_for(net, "main/ppo_head/policy_mean", (5,), A, lr)
    ls = net.params.named_arrays()["main/ppo_head/policy_log_std"][0].copy()
    assert not ls.any()
    sides = []
    for step in range(2):
        obs = rng.randn(B, 5).astype(F32)
        mean = o.q(obs).astype(F32)
        mu_t, std_t = (x.cpu().numpy().copy() for x in net.policy_mean_std(_t(obs, dev), B, use_target=True))
        np.testing.assert_allclose(net.policy_mean_std(_t(obs, dev), B)[0].cpu().numpy(), mean, **OUT)
        if step == 1:
            mu_t = (mu_t + 0.5 * rng.randn(B, A)).astype(F32)
        actions = (mean + np.exp(ls) * rng.randn(B, A)).astype(F32)
        adv = rng.randn(B).astype(F32)
        ref = R.ppo_kl_continuous_loss(mean, ls, actions, adv, mu_t, std_t, beta, klc, 2 * target_kl, high, True, 1.0)
        sides.append(ref["side"])
        o.tower.backward(o.head.backward(ref["dmean"].astype(F32)))
        dls = ref["dlog_std"].astype(F32)
        norm = np.sqrt(float(o.global_norm()) ** 2 + float((dls.astype(np.float64) ** 2).sum()))
        o.adam_step(1.0)
        o.adam.step("policy_log_std", ls, dls)
        scalars = net.train_minibatch(_t(obs, dev), B, _t(actions, dev), _t(adv, dev),
                                      (_t(mu_t, dev), _t(std_t, dev))).cpu().numpy()
        np.testing.assert_allclose(scalars, ref["scalars"], **LOSS)
        np.testing.assert_allclose(float(net.norm.item()), norm, **LOSS)
        _weights_match(net, o, "main/ppo_head/policy_mean")
        np.testing.assert_allclose(net.params.named_arrays()["main/ppo_head/policy_log_std"][0], ls, **WEIGHTS)
    assert sides == ["below", "above"] and ls.any()


def test_actor_refuses_sizes_the_head_does_not_serve(dev):
    from coach_amd.nn.networks import PPOActorNet
    with pytest.raises(ValueError, match="1 .. 18 actions"):
        PPOActorNet(dev, (4,), 19, **SCHEME)
    with pytest.raises(ValueError, match="1 .. 32 action dimensions"):
        PPOActorNet(dev, (4,), 33, continuous=True, **SCHEME)


def test_captured_actor_minibatch_follows_the_coefficient(dev):
    """a policy minibatch + the coefficient update captured as a graph (forward, head launch, backward, Adam, update)
    and replayed gives the weights, scalars, running sums and coefficient of the same steps launched eagerly on a twin
    network, bit for bit — the coefficient changes between the replays (x 1.5 each time) and the captured head launch
    reads the new value"""
    import torch
    from coach_amd.nn.networks import PPOActorNet
    rng = np.random.RandomState(14)
    A = 3
    kw = dict(learning_rate=5e-4, beta_entropy=0.01, target_kl_divergence=0.01, initial_kl_coefficient=1.0, seed=8, **SCHEME)
    eager, captured = PPOActorNet(dev, (4,), A, **kw), PPOActorNet(dev, (4,), A, **kw)
    assert torch.equal(eager.params.weights, captured.params.weights)
    obs, adv = _t(rng.randn(B, 4).astype(F32), dev), _t(rng.randn(B).astype(F32), dev)
    actions = _t(rng.randint(0, A, size=B).astype(np.int32), dev)
    old = _t(_perturbed(rng, np.full((B, A), 1.0 / A), 1.0), dev)                # far from the new policy: KL above 1.3 target

    def step(net):
        net.reset_epoch_sums()
        net.train_minibatch(obs, B, actions, adv, old)
        net.update_kl_coefficient()
    from coach_amd.agents.vector_agent import capture
    step(captured)                                                               # step 1, eager: every buffer exists
    graph = capture(lambda: step(captured))                                      # (a capture launches nothing)
    torch.cuda.synchronize()
    step(eager)
    assert torch.equal(eager.params.weights, captured.params.weights)
    for k in range(2, 4):
        graph.replay()
        step(eager)
        torch.cuda.synchronize()
        assert torch.equal(eager.params.weights, captured.params.weights), k
        assert torch.equal(eager.scalars, captured.scalars) and torch.equal(eager.epoch_sums, captured.epoch_sums)
        assert torch.equal(eager.kl_coefficient, captured.kl_coefficient)
        assert float(eager.kl_coefficient.item()) == 1.5 ** k
