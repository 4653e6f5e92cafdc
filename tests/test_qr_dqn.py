"""Quantile-Regression DQN on the device: rlx_qr_dqn_head_loss and rlx_quantile_egreedy (csrc/qr_dqn.hip) against the
numpy restatement (tests/qr_dqn_ref.py, itself pinned to the reference agent by tests/test_qr_dqn_ref.py), the network
update against the oracle's layers + TF1 Adam composed with that restatement, the staged-record step graph against
act() + train(), and the reference's golden bar for CartPole_QR_DQN."""
import random

import numpy as np
import pytest

import qr_dqn_ref as R
from tolerances import LOSS, OUT, WEIGHTS

pytestmark = pytest.mark.gpu


def _t(x, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t if dtype is None else t.to(dtype)


def _launch(rlx, dev, theta, theta_next, actions, rewards, go, discount, kappa, ws, ticket):
    import torch
    B, A, N = theta.shape
    d = torch.full((B, A * N), float("nan"), dtype=torch.float32, device=dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    T = torch.zeros(B, N, dtype=torch.float32, device=dev)
    tau = torch.zeros(B, N, dtype=torch.float32, device=dev)
    a_star = torch.zeros(B, dtype=torch.int32, device=dev)
    rlx.qr_dqn_head_loss(_t(theta.reshape(B, A * N), dev), A * N, _t(theta_next.reshape(B, A * N), dev), A * N,
                         _t(actions.astype(np.int32), dev), _t(rewards.astype(np.float32), dev),
                         _t(go.astype(np.uint8), dev), discount, kappa, N, A, B, 1.0, d, A * N, ws, ticket, loss,
                         status, T, tau, a_star, 0)
    torch.cuda.synchronize()
    return (a_star.cpu().numpy(), T.cpu().numpy(), tau.cpu().numpy(), loss.cpu().numpy()[0],
            d.cpu().numpy().reshape(B, A, N), int(status.item()))


@pytest.mark.parametrize("kappa", [1.0, 0.5])
@pytest.mark.parametrize("N", [1, 50, 200])
@pytest.mark.parametrize("A", [2, 6, 18])
@pytest.mark.parametrize("B", [1, 32, 37])
def test_loss_kernel_equals_the_restatement(rlx, dev, B, A, N, kappa):
    import torch
    rng = np.random.RandomState(B * 1000 + A * 10 + N)
    theta = rng.randn(B, A, N).astype(np.float32)
    theta_next = rng.randn(B, A, N).astype(np.float32)
    actions = rng.randint(0, A, size=B)
    rewards = rng.randn(B).astype(np.float32)
    go = rng.rand(B) < 0.3
    go[0] = False
    if B > 1:
        go[1] = True
    ws = torch.zeros(256, dtype=torch.float32, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    a_star, T, tau, loss, d, status = _launch(rlx, dev, theta, theta_next, actions, rewards, go, 0.99, kappa, ws, ticket)
    ra, rT, rtau, rloss, rd = R.update(theta, theta_next, actions, rewards, go, 0.99, kappa)
    assert status == 0 and int(ticket.item()) == 0
    assert np.array_equal(a_star, ra)
    assert np.array_equal(T.view(np.uint32), rT.view(np.uint32))
    assert np.array_equal(tau.view(np.uint32), rtau.view(np.uint32))
    np.testing.assert_allclose(loss, rloss, **LOSS)
    np.testing.assert_allclose(d, rd, **OUT)
    off = np.ones((B, A), bool)
    off[np.arange(B), actions] = False
    assert np.all(d[off] == 0.0)
    again = _launch(rlx, dev, theta, theta_next, actions, rewards, go, 0.99, kappa, ws, ticket)
    assert again[3].tobytes() == loss.tobytes() and again[4].tobytes() == d.tobytes()


def test_loss_kernel_flags_an_action_out_of_range_and_refuses_large_shapes(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    rng = np.random.RandomState(2)
    theta = rng.randn(4, 3, 8).astype(np.float32)
    actions = np.array([0, 3, 1, 2])
    ws = torch.zeros(256, dtype=torch.float32, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    *_, d, status = _launch(rlx, dev, theta, theta, actions, np.zeros(4), np.zeros(4, bool), 0.99, 1.0, ws, ticket)
    assert status == 1 and int(ticket.item()) == 0 and np.all(d[1] == 0)
    big = torch.zeros(1, 19 * 4, dtype=torch.float32, device=dev)
    with pytest.raises(RlxError):
        rlx.qr_dqn_head_loss(big, 76, big, 76, ticket, big, ticket, 0.99, 1.0, 4, 19, 1, 1.0, big, 76, ws, ticket,
                             ws, ticket, None, None, None, 0)


def test_quantile_egreedy_equals_the_reference_formula(rlx, dev):
    import torch
    rng = np.random.RandomState(11)
    for n_env, A, N in ((5, 2, 50), (9, 6, 200), (4, 18, 1), (3, 4, 7)):
        x = rng.randn(n_env, A, N).astype(np.float32)
        x[0, 1] = x[0, 0]                                  # exact ties: the tie uniforms decide
        x[1, :] = x[1, 0]
        q_ref = R.q_values(x)
        u = rng.rand(n_env)
        u[:3] = 0.9                                       # greedy rows include the tied ones
        ra = rng.randint(0, A, size=n_env).astype(np.int32)
        tie = rng.rand(n_env, A)
        q_out = torch.zeros(n_env, A, dtype=torch.float64, device=dev)
        acts = torch.zeros(n_env, dtype=torch.int32, device=dev)
        rlx.quantile_egreedy(_t(x.reshape(n_env, A * N), dev), A * N, N, _t(u, dev), _t(ra, dev), _t(tie, dev), 0.5,
                             n_env, A, q_out, acts, 0)
        q = q_out.cpu().numpy()
        assert np.all(np.abs(q - q_ref) <= 4 * np.spacing(np.abs(x.astype(np.float64)).mean(-1)))
        assert np.array_equal(q, R.q_values_device_order(x))
        assert acts.cpu().numpy().tolist() == R.egreedy(q_ref, u, ra, tie, 0.5).tolist()
        if A > 1:
            assert q[1, 0] == q[1, A - 1]


def _oracle_for(net, obs_shape, lr, eps):
    from oracle.agents import DQNOracle
    return DQNOracle(net.params.named_arrays(), obs_shape, net.AN, lr=lr, eps=eps)


def _oracle_update(o, obs, next_obs, actions, rewards, go, A, N, kappa, discount=0.99):
    B = obs.shape[0]
    q_next = o.q(next_obs, target=True).reshape(B, A, N)
    q = o.q(obs).reshape(B, A, N)
    _, _, _, loss, d = R.update(q, q_next, actions, rewards, go, discount, kappa)
    o.tower.backward(o.head.backward(d.reshape(B, A * N)))
    o.adam_step(1.0)
    return loss


@pytest.mark.parametrize("kind", ["vector", "image"])
def test_network_update_equals_the_composed_oracle(dev, kind):
    """QRDQNNet.learn_from_batch against oracle layers + TF1 Adam + the restatement, fed the same batches: CartPole's
    shape (4 -> Medium MLP, A 2, N 50, B 32) for 20 updates with target copies between them; one image update
    (84 x 84 x 4, A 6, N 200)."""
    import torch
    from coach_amd.nn.networks import QRDQNNet
    rng = np.random.RandomState(7)
    if kind == "vector":
        shape, A, N, B, updates, lr = (4,), 2, 50, 32, 20, 5e-4
    else:
        shape, A, N, B, updates, lr = (84, 84, 4), 6, 200, 8, 1, 5e-5
    net = QRDQNNet(dev, shape, A, N, huber_loss_interval=1.0, learning_rate=lr, optimizer_epsilon=0.01 / 32, seed=3)
    o = _oracle_for(net, shape, lr, 0.01 / 32)
    for u in range(updates):
        if kind == "vector":
            obs, nxt = rng.randn(B, 4).astype(np.float32), rng.randn(B, 4).astype(np.float32)
        else:
            obs = rng.randint(0, 256, size=(B,) + shape).astype(np.uint8)
            nxt = rng.randint(0, 256, size=(B,) + shape).astype(np.uint8)
        actions = rng.randint(0, A, size=B)
        rewards = rng.choice([0.0, 1.0], size=B).astype(np.float32)
        go = rng.rand(B) < 0.1
        loss = net.learn_from_batch(_t(obs, dev), _t(nxt, dev), B, _t(actions.astype(np.int32), dev), _t(rewards, dev),
                                    _t(go.astype(np.uint8), dev), 0.99)
        ref = _oracle_update(o, obs, nxt, actions, rewards, go, A, N, 1.0)
        np.testing.assert_allclose(float(loss.item()), ref, **LOSS)
        if u % 5 == 4:
            net.update_target(1.0)
            o.update_target(1.0)
    net.check_status()
    w, wo = net.params.named_arrays(), o.weights()
    worst = max(float(np.abs(w[n][0] - t[0]).max()) for n, t in wo.items())
    print("\n  %s: %d updates, weights max abs diff %.3e" % (kind, updates, worst))
    for name, towers in wo.items():
        np.testing.assert_allclose(w[name][0], towers[0], err_msg=name, **WEIGHTS)
    assert torch.isfinite(net.params.weights).all()


def test_prioritized_memory_is_refused(dev):
    from coach_amd.agents.qr_dqn_agent import QuantileRegressionDQNAgent, QuantileRegressionDQNAgentParameters
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    from coach_amd.memories.non_episodic.prioritized_experience_replay import PrioritizedExperienceReplayParameters
    p = QuantileRegressionDQNAgentParameters()
    p.algorithm.atoms = 8
    p.memory = PrioritizedExperienceReplayParameters()
    env = SyntheticVectorEnvironment(SyntheticVectorEnvironmentParameters("vector", 1, (4,), 2, episode_length=5, seed=3),
                                     dev)
    with pytest.raises(ValueError):
        QuantileRegressionDQNAgent(p, env, dev)


def test_qr_dqn_whole_step_graph_equals_act_plus_train(dev):
    """step_and_train (one staged record + one hipGraph per env-step) against act() + train(): bit-identical weights,
    target, Adam state, replay contents and counters, with target copies inside the run."""
    import torch
    from coach_amd.agents.qr_dqn_agent import QuantileRegressionDQNAgent, QuantileRegressionDQNAgentParameters
    from coach_amd.core_types import EnvironmentSteps, RunPhase
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    from coach_amd.memories.memory import MemoryGranularity
    agents = []
    for fused in (True, False):
        p = QuantileRegressionDQNAgentParameters()
        p.seed = 5
        p.algorithm.atoms = 10
        p.network_wrappers["main"].batch_size = 16
        p.memory.max_size = (MemoryGranularity.Transitions, 64)
        p.algorithm.num_consecutive_playing_steps = EnvironmentSteps(1)
        p.algorithm.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(7)
        env = SyntheticVectorEnvironment(SyntheticVectorEnvironmentParameters("vector", 1, (6,), 3, episode_length=5,
                                                                              seed=3), dev)
        a = QuantileRegressionDQNAgent(p, env, dev)
        random.seed(9); np.random.seed(9)
        a.phase = RunPhase.HEATUP
        for _ in range(20):
            a.act()
        a.phase = RunPhase.TRAIN
        for _ in range(45):
            if fused:
                a.step_and_train()
            else:
                a.act(); a.train()
        a.check_status()
        agents.append(a)
    f, s = agents
    assert f._step_graph_ok() and any(k[0] == "step" for k in f._graphs)
    net_f, net_s = f.networks["main"], s.networks["main"]
    assert torch.equal(net_f.params.weights, net_s.params.weights)
    assert torch.equal(net_f.target, net_s.target)
    assert torch.equal(net_f.adam.v, net_s.adam.v)
    assert not torch.equal(net_f.params.weights, net_f.target)          # it did train
    for col in ("obs", "next_obs", "action", "reward", "game_over"):
        assert torch.equal(getattr(f.memory, col), getattr(s.memory, col)), col
    assert (f.training_iteration, f.total_steps_counter, f.memory.count, f.memory.cursor, f.memory.pending) == \
        (s.training_iteration, s.total_steps_counter, s.memory.count, s.memory.cursor, s.memory.pending)
    assert f.episode_statistics() == s.episode_statistics()


def test_cartpole_qr_dqn_preset_reaches_the_golden_threshold(dev, tmp_path):
    """presets/CartPole_QR_DQN.py of the reference: min_reward_threshold 150 within max_episodes_to_achieve_reward 250,
    with the agent seed 0 the reference's golden tests use."""
    from test_cartpole import _golden
    st = _golden(dev, "CartPole_QR_DQN", tmp_path)
    assert st["passed"], st
