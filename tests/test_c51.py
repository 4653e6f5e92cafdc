"""Categorical DQN (C51) on the device: rlx_c51_head_loss and rlx_categorical_egreedy (csrc/c51.hip) against the numpy
restatement (tests/c51_ref.py, itself pinned to the reference agent by tests/test_c51_ref.py), the network update against
the oracle's layers + TF1 Adam composed with that restatement, the staged-record step graph against act() + train(),
prioritized replay driven by the kernel's error buffer, and the golden bar for CartPole_C51.

Tolerances: a*, m, the zero pattern of dlogits, the Q values and the chosen actions are compared exactly (the kernels'
softmax and their fp64 sums are restated operation by operation).  The loss, the per-action losses and the PER errors
differ from the restatement by fp32 summation order and the device's logf: tests/tolerances.py's LOSS (minibatch losses)
fits them, OUT (action probabilities) fits the gradient p - m."""
import random

import numpy as np
import pytest

import c51_ref as R
from test_c51_ref import expectation_ulp_bound
from tolerances import LOSS, OUT, WEIGHTS

pytestmark = pytest.mark.gpu

SUPPORTS = {"c51": (-10.0, 10.0), "wide": (0.0, 200.0)}


def _t(x, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t if dtype is None else t.to(dtype)


def _launch(rlx, dev, logits, logits_next, z, actions, rewards, go, discount, ws, ticket, with_errors=True):
    import torch
    B, A, N = logits.shape
    d = torch.full((B, A * N), float("nan"), dtype=torch.float32, device=dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    m = torch.zeros(B, N, dtype=torch.float32, device=dev)
    a_star = torch.zeros(B, dtype=torch.int32, device=dev)
    ce = torch.zeros(B, A, dtype=torch.float32, device=dev)
    err = torch.full((B,), float("nan"), dtype=torch.float64, device=dev) if with_errors else None
    rlx.c51_head_loss(_t(logits.reshape(B, A * N), dev), A * N, _t(logits_next.reshape(B, A * N), dev), A * N,
                      _t(z, dev), _t(actions.astype(np.int32), dev), _t(rewards.astype(np.float32), dev),
                      _t(go.astype(np.uint8), dev), discount, N, A, B, 1.0, d, A * N, err, ws, ticket, loss, status,
                      m, a_star, ce, 0)
    torch.cuda.synchronize()
    return dict(a_star=a_star.cpu().numpy(), m=m.cpu().numpy(), loss=loss.cpu().numpy()[0],
                dlogits=d.cpu().numpy().reshape(B, A, N), action_losses=ce.cpu().numpy(),
                errors=None if err is None else err.cpu().numpy(), status=int(status.item()))


def _inputs(rng, B, A, N, support):
    z = R.support(*SUPPORTS[support], N)
    logits = (rng.randn(B, A, N) * 2).astype(np.float32)
    logits_next = (rng.randn(B, A, N) * 2).astype(np.float32)
    actions = rng.randint(0, A, size=B)
    # rewards on the support's scale; the wide support gets reward 1, as CartPole gives
    rewards = np.ones(B, np.float32) if support == "wide" else rng.randn(B).astype(np.float32)
    go = rng.rand(B) < 0.3
    go[0] = False
    if B > 1:
        go[1] = True
    return z, logits, logits_next, actions, rewards, go


@pytest.mark.parametrize("support", sorted(SUPPORTS))
@pytest.mark.parametrize("N", [2, 51, 256])
@pytest.mark.parametrize("A", [2, 6, 18])
@pytest.mark.parametrize("B", [1, 32, 37])
def test_loss_kernel_equals_the_restatement(rlx, dev, B, A, N, support):
    import torch
    rng = np.random.RandomState(B * 1000 + A * 10 + N)
    z, logits, logits_next, actions, rewards, go = _inputs(rng, B, A, N, support)
    ws = torch.zeros(256, dtype=torch.float32, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    k = _launch(rlx, dev, logits, logits_next, z, actions, rewards, go, 0.99, ws, ticket)
    # np.linspace(-10, 10, 256) is a support on which the reference itself raises IndexError for an atom clipped at
    # v_max (c51_ref.overhangs): there the kernel is compared with the restatement that leaves that contribution out
    assert R.overhangs(z) == (N == 256 and support == "c51")
    r = R.update(logits, logits_next, z, actions, rewards, go, 0.99, overhang="drop" if R.overhangs(z) else "raise")
    rows = np.arange(B)
    print("\n  B %d A %d N %d %s: loss %.6g (twin %.6g, rel %.2e), max |dlogits - twin| %.2e, max rel error diff %.2e, "
          "m bits equal %s" % (B, A, N, support, k["loss"], r["loss"], abs(k["loss"] - r["loss"]) / abs(r["loss"]),
                               np.abs(k["dlogits"] - r["dlogits"]).max(),
                               (np.abs(k["errors"] - r["errors"]) / np.maximum(np.abs(r["errors"]), 1e-30)).max(),
                               np.array_equal(k["m"].view(np.uint32), r["m"].view(np.uint32))))
    assert k["status"] == 0 and int(ticket.item()) == 0
    assert np.array_equal(k["a_star"], r["a_star"])
    assert np.array_equal(k["m"].view(np.uint32), r["m"].view(np.uint32))
    off = np.ones((B, A), bool)
    off[rows, actions] = False
    assert np.all(k["dlogits"][off] == 0.0) and not np.isnan(k["dlogits"]).any()
    assert np.any(k["dlogits"][rows, actions] != 0.0)
    np.testing.assert_allclose(k["loss"], r["loss"], **LOSS)
    np.testing.assert_allclose(k["action_losses"], r["action_losses"], **LOSS)
    np.testing.assert_allclose(k["dlogits"], r["dlogits"], **OUT)
    assert k["errors"].dtype == np.float64
    np.testing.assert_allclose(k["errors"], r["errors"], **LOSS)
    # the error buffer is the taken action's cross entropy, widened
    assert np.array_equal(k["errors"], k["action_losses"][rows, actions].astype(np.float64))
    again = _launch(rlx, dev, logits, logits_next, z, actions, rewards, go, 0.99, ws, ticket, with_errors=False)
    assert again["loss"].tobytes() == k["loss"].tobytes() and again["dlogits"].tobytes() == k["dlogits"].tobytes()


def test_loss_kernel_keeps_the_dropped_mass(rlx, dev):
    """N = 2 on [0, 1] with reward 1 and no game-over: every atom is clipped at v_max, bj is an integer, m is all zero."""
    import torch
    rng = np.random.RandomState(4)
    z = R.support(0.0, 1.0, 2)
    logits = rng.randn(3, 2, 2).astype(np.float32)
    ws = torch.zeros(256, dtype=torch.float32, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    k = _launch(rlx, dev, logits, logits, z, np.array([0, 1, 0]), np.ones(3), np.zeros(3, bool), 0.99, ws, ticket)
    assert np.all(k["m"] == 0.0)
    p = R.softmax(logits)
    assert np.array_equal(k["dlogits"][np.arange(3), [0, 1, 0]], p[np.arange(3), [0, 1, 0]])     # p - 0
    assert np.all(k["errors"] == 0.0)


def test_loss_kernel_flags_an_action_out_of_range_and_refuses_large_shapes(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    rng = np.random.RandomState(2)
    logits = rng.randn(4, 3, 8).astype(np.float32)
    z = R.support(-10.0, 10.0, 8)
    actions = np.array([0, 3, 1, 2])
    ws = torch.zeros(256, dtype=torch.float32, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    k = _launch(rlx, dev, logits, logits, z, actions, np.zeros(4), np.zeros(4, bool), 0.99, ws, ticket)
    assert k["status"] == 1 and int(ticket.item()) == 0 and np.all(k["dlogits"][1] == 0) and k["errors"][1] == 0.0
    assert np.any(k["dlogits"][0] != 0)
    zd = _t(R.support(-10.0, 10.0, 4), dev)
    for n_atoms, n_actions, batch in ((4, 19, 1), (257, 1, 1), (1, 2, 1), (4, 2, 257)):
        big = torch.zeros(max(batch, 1), 19 * 257, dtype=torch.float32, device=dev)
        ld = 19 * 257
        with pytest.raises(RlxError):
            rlx.c51_head_loss(big, ld, big, ld, zd, ticket, big, ticket, 0.99, n_atoms, n_actions, batch, 1.0, big, ld,
                              None, ws, ticket, ws, ticket, None, None, None, 0)
    with pytest.raises(RlxError):
        rlx.categorical_egreedy(big, ld, zd, 4, zd, ticket, zd, 0.5, 1, 19, None, ticket, 0)


def test_categorical_egreedy_equals_the_reference_formula(rlx, dev):
    import torch
    rng = np.random.RandomState(11)
    for n_env, A, N, support in ((5, 2, 51, "c51"), (9, 6, 51, "wide"), (4, 18, 2, "c51"), (3, 4, 256, "c51"),
                                 (3, 18, 256, "wide")):
        z = R.support(*SUPPORTS[support], N)
        x = (rng.randn(n_env, A, N) * 2).astype(np.float32)
        x[0, 1] = x[0, 0]                                  # exact ties: the tie uniforms decide
        x[1, :] = x[1, 0]
        p = R.softmax(x)
        q_ref = R.q_values(p, z)
        u = rng.rand(n_env)
        u[:3] = 0.9                                       # greedy rows include the tied ones
        ra = rng.randint(0, A, size=n_env).astype(np.int32)
        tie = rng.rand(n_env, A)
        q_out = torch.zeros(n_env, A, dtype=torch.float64, device=dev)
        acts = torch.zeros(n_env, dtype=torch.int32, device=dev)
        rlx.categorical_egreedy(_t(x.reshape(n_env, A * N), dev), A * N, _t(z, dev), N, _t(u, dev), _t(ra, dev),
                                _t(tie, dev), 0.5, n_env, A, q_out, acts, 0)
        q = q_out.cpu().numpy()
        mag = (p.astype(np.float64) * np.abs(z)).sum(-1)
        assert np.all(np.abs(q - q_ref) <= expectation_ulp_bound(N) * np.spacing(mag))
        assert np.array_equal(q, R.q_values_device_order(p, z))
        assert acts.cpu().numpy().tolist() == R.egreedy(q, u, ra, tie, 0.5).tolist()
        assert q[1, 0] == q[1, A - 1] and q[0, 0] == q[0, 1]
        # without the optional output
        acts2 = torch.zeros(n_env, dtype=torch.int32, device=dev)
        rlx.categorical_egreedy(_t(x.reshape(n_env, A * N), dev), A * N, _t(z, dev), N, _t(u, dev), _t(ra, dev),
                                _t(tie, dev), 0.5, n_env, A, None, acts2, 0)
        assert torch.equal(acts, acts2)


def _oracle_for(net, obs_shape, lr, eps):
    from oracle.agents import DQNOracle
    return DQNOracle(net.params.named_arrays(), obs_shape, net.AN, lr=lr, eps=eps)


def _oracle_update(o, obs, next_obs, actions, rewards, go, A, N, z, discount=0.99):
    B = obs.shape[0]
    x_next = o.q(next_obs, target=True).reshape(B, A, N)
    x = o.q(obs).reshape(B, A, N)
    r = R.update(x.astype(np.float32), x_next.astype(np.float32), z, actions, rewards, go, discount)
    o.tower.backward(o.head.backward(r["dlogits"].reshape(B, A * N)))
    o.adam_step(1.0)
    return r["loss"]


@pytest.mark.parametrize("kind", ["vector", "image"])
def test_network_update_equals_the_composed_oracle(dev, kind):
    """C51Net.learn_from_batch against oracle layers + TF1 Adam + the restatement, fed the same batches, with the agent's
    default support and optimizer (51 atoms on [-10, 10], lr 2.5e-4, Adam epsilon 1e-4): CartPole's shape (4 -> Medium
    MLP, A 2, B 32) for 20 updates with target copies between them; one image update (84 x 84 x 4, A 6).

    Measured on the MI355X while this test was written, and kept here because it decides what a failure means: with
    the support [0, 100], lr 5e-4 and these batches every loss of the 20 updates agreed with the oracle's to 1.3e-7
    relative and the weights to 1.5e-8 up to the third update, where 18 weights of the first layer (a few nearly dead
    units) began to drift, by 4e-5 in that update and by a decaying amount in each later one, to 3e-4 at the end — the
    momentum tail of one sample whose pre-activation lies on the other side of the ReLU's zero in fp32; with Adam
    epsilon 0.01 / 32 or with the support [-10, 10] the same run stayed at 2.2e-8.  A difference of that shape is not a
    wrong update; a loss outside LOSS in any update is."""
    import torch
    from coach_amd.nn.networks import C51Net
    rng = np.random.RandomState(7)
    if kind == "vector":
        shape, A, N, B, updates, lr, v = (4,), 2, 51, 32, 20, 2.5e-4, (-10.0, 10.0)
    else:
        shape, A, N, B, updates, lr, v = (84, 84, 4), 6, 51, 8, 1, 2.5e-4, (-10.0, 10.0)
    net = C51Net(dev, shape, A, N, v_min=v[0], v_max=v[1], learning_rate=lr, optimizer_epsilon=1e-4, seed=3)
    assert np.array_equal(net.z.cpu().numpy(), R.support(v[0], v[1], N))
    o = _oracle_for(net, shape, lr, 1e-4)
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
        ref = _oracle_update(o, obs, nxt, actions, rewards, go, A, N, net.z_values)
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


def _agent(dev, per=False, seed=5, atoms=11, B=16, cap=64, use_graphs=None):
    from coach_amd.agents.categorical_dqn_agent import CategoricalDQNAgent, CategoricalDQNAgentParameters
    from coach_amd.core_types import EnvironmentSteps
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    from coach_amd.memories.memory import MemoryGranularity
    from coach_amd.memories.non_episodic.prioritized_experience_replay import PrioritizedExperienceReplayParameters
    p = CategoricalDQNAgentParameters()
    p.seed = seed
    p.algorithm.atoms, p.algorithm.v_min, p.algorithm.v_max = atoms, -2.0, 8.0
    p.network_wrappers["main"].batch_size = B
    if per:
        p.memory = PrioritizedExperienceReplayParameters()
    p.memory.max_size = (MemoryGranularity.Transitions, cap)
    p.algorithm.num_consecutive_playing_steps = EnvironmentSteps(1)
    p.algorithm.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(7)
    env = SyntheticVectorEnvironment(SyntheticVectorEnvironmentParameters("vector", 1, (6,), 3, episode_length=5,
                                                                          seed=3), dev)
    return CategoricalDQNAgent(p, env, dev, use_graphs=use_graphs)


def test_c51_whole_step_graph_equals_act_plus_train(dev):
    """step_and_train (one staged record + one hipGraph per env-step) against act() + train(): bit-identical weights,
    target, Adam state, replay contents and counters, with target copies inside the run."""
    import torch
    from coach_amd.core_types import RunPhase
    agents = []
    for fused in (True, False):
        a = _agent(dev)
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


def _one_prioritized_update(dev, weight_factor=None):
    """heat up, then ONE update from a PrioritizedExperienceReplay; returns what the update saw and what it left."""
    import torch
    from coach_amd.core_types import RunPhase
    a = _agent(dev, per=True, use_graphs=False)
    random.seed(9); np.random.seed(9)
    a.phase = RunPhase.HEATUP
    for _ in range(30):
        a.act()
    a.phase = RunPhase.TRAIN
    mem, net = a.memory, a.networks["main"]
    seen = {}
    inner = a.learn_from_batch

    def spy(batch):
        B = a.batch_size
        if weight_factor is not None:
            batch._info["weight"].mul_(weight_factor)
        seen["weight"] = batch.info("weight").cpu().numpy().copy()
        seen["idx"] = batch.info("idx").clone()
        seen["trees"] = [t.clone() for t in (mem.sum_tree, mem.min_tree, mem.max_tree, mem.max_priority)]
        seen["x"] = net.distribution_logits(batch._states["observation"], B, tag="spy").data.view(
            B, a.A, a.N).cpu().numpy().copy()
        seen["x_next"] = net.distribution_logits(batch._next_states["observation"], B, use_target=True,
                                                 tag="spy_t").data.view(B, a.A, a.N).cpu().numpy().copy()
        seen["actions"] = batch.actions().cpu().numpy().astype(np.int64)
        seen["rewards"] = batch.rewards().cpu().numpy().copy()
        seen["go"] = batch.game_overs().cpu().numpy().astype(bool)
        seen["w0"] = net.params.weights.clone()
        return inner(batch)
    a.learn_from_batch = spy
    a.act()
    a.train()
    a.check_status()
    mem.check_status()
    torch.cuda.synchronize()
    assert a.training_iteration >= 1 and "idx" in seen
    return a, seen


def test_prioritized_replay_gets_the_taken_actions_cross_entropy(dev):
    """categorical_dqn_agent.py:162-165: errors = losses[0][arange(B), actions] -> update_priorities.  After one update
    the three trees equal those that update_priorities builds from the restatement's errors (to the tolerance of the
    errors themselves, LOSS: the leaves are (error + epsilon) ** alpha), and bit for bit those it builds from the
    kernel's own error buffer."""
    import torch
    a, seen = _one_prioritized_update(dev)
    mem, net = a.memory, a.networks["main"]
    r = R.update(seen["x"], seen["x_next"], net.z_values, seen["actions"], seen["rewards"], seen["go"],
                 a.ap.algorithm.discount)
    np.testing.assert_allclose(a.td_errors.cpu().numpy(), r["errors"], **LOSS)
    assert np.all(r["errors"] > 0)
    after = [t.clone() for t in (mem.sum_tree, mem.min_tree, mem.max_tree, mem.max_priority)]
    assert not torch.equal(after[0], seen["trees"][0])                    # priorities were updated
    for errors, exact in ((_t(r["errors"], dev), False), (a.td_errors.clone(), True)):
        for t, t0 in zip((mem.sum_tree, mem.min_tree, mem.max_tree, mem.max_priority), seen["trees"]):
            t.copy_(t0)
        mem.update_priorities(seen["idx"], errors)
        mem.check_status()
        for t, ta in zip((mem.sum_tree, mem.min_tree, mem.max_tree, mem.max_priority), after):
            if exact:
                assert torch.equal(t, ta)
            else:
                np.testing.assert_allclose(t.cpu().numpy(), ta.cpu().numpy(), **LOSS)
    assert not torch.equal(net.params.weights, seen["w0"])


def test_importance_weights_have_no_effect_on_the_update(dev):
    """The reference's head has an empty loss_type: the importance-weight placeholder exists and is never multiplied
    in (heads/head.py:141-180).  Scaling the sampled weights changes nothing: weights, Adam state, loss, priorities."""
    import torch
    a, sa = _one_prioritized_update(dev)
    b, sb = _one_prioritized_update(dev, weight_factor=7.0)
    np.testing.assert_array_equal(sb["weight"], sa["weight"] * 7.0)
    assert sa["weight"].min() > 0
    assert torch.equal(sa["idx"], sb["idx"])
    na, nb = a.networks["main"], b.networks["main"]
    assert torch.equal(na.params.weights, nb.params.weights) and not torch.equal(na.params.weights, sa["w0"])
    assert torch.equal(na.adam.v, nb.adam.v) and torch.equal(na.loss, nb.loss)
    assert torch.equal(a.td_errors, b.td_errors)
    assert torch.equal(a.memory.sum_tree, b.memory.sum_tree)


def test_cartpole_c51_preset_reaches_the_golden_threshold(dev, tmp_path):
    """CartPole_C51 with the bar of the reference's CartPole_QR_DQN: min_reward_threshold 150 within
    max_episodes_to_achieve_reward 250, with the agent seed 0 the reference's golden tests use."""
    from test_cartpole import _golden
    st = _golden(dev, "CartPole_C51", tmp_path)
    assert st["passed"], st
