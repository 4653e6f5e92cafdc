"""Bootstrapped DQN on the device: rlx_bootstrapped_dqn_head_loss and rlx_bootstrapped_egreedy
(csrc/bootstrapped_dqn.hip) against the numpy restatement (tests/bootstrapped_ref.py, itself pinned to the reference
agent by tests/test_bootstrapped_dqn_ref.py) and against rlx_dqn_head_loss head by head; the replay's mask column; the
network update against the oracle's layers + TF1 Adam composed with the restatement; graph replay, checkpoints and the
agent's host draws."""
import os
import random

import numpy as np
import pytest

import bootstrapped_ref as R
from test_bootstrapped_dqn_ref import ACT_CASES, CASES, acting_draws, case
from tolerances import LOSS, WEIGHTS

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "bootstrapped_dqn.npz"))


def _t(x, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t if dtype is None else t.to(dtype)


def _launch(rlx, dev, q_online, q_next, q_sel, actions, rewards, go, masks, huber, discount=0.99):
    import torch
    K, B, A = q_online.shape
    KA = K * A
    dq = torch.full((B, KA), float("nan"), dtype=torch.float32, device=dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(K * B, dtype=torch.float32, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    heads = torch.zeros(K, dtype=torch.float32, device=dev)
    td = torch.zeros(B, K, dtype=torch.float32, device=dev)
    a_star = torch.zeros(B, K, dtype=torch.int32, device=dev)
    words = R.mask_words(masks).view(np.int32)
    rlx.bootstrapped_dqn_head_loss(_t(R.columns(q_online), dev), KA, _t(R.columns(q_next), dev),
                                   _t(R.columns(q_sel), dev), KA, _t(actions.astype(np.int32), dev),
                                   _t(rewards.astype(np.float32), dev), _t(go.astype(np.uint8), dev), _t(words, dev),
                                   discount, B, K, A, int(huber), 1.0, dq, KA, ws, ticket, loss, status, heads, td, a_star, 0)
    torch.cuda.synchronize()
    return dict(dq=dq.cpu().numpy().reshape(B, K, A).transpose(1, 0, 2), loss=loss.cpu().numpy()[0],
                head_losses=heads.cpu().numpy(), td=td.cpu().numpy(), a_star=a_star.cpu().numpy(),
                status=int(status.item()), ticket=int(ticket.item()))


@pytest.mark.parametrize("huber", [True, False])
@pytest.mark.parametrize("s", range(len(CASES)))
def test_loss_kernel_equals_the_restatement_on_the_golden_cases(rlx, dev, gold, s, huber):
    c = case(gold, s)
    B, A, K, _ = CASES[s]
    args = (c["q_online"], c["q_next"], c["q_sel"], c["actions"], c["rewards"], c["go"], c["masks"])
    d = _launch(rlx, dev, *args, huber)
    u = R.update(*args, 0.99, huber)
    assert d["status"] == 0 and d["ticket"] == 0
    assert np.array_equal(d["a_star"], u["a_star"])
    taken = u["td_targets"][:, np.arange(B), c["actions"]].T                   # [B, K]; the golden's own entries
    assert np.array_equal(taken.view(np.uint32), c["targets"][:, np.arange(B), c["actions"]].T.view(np.uint32))
    assert np.array_equal(d["td"].view(np.uint32), np.ascontiguousarray(taken).view(np.uint32))
    np.testing.assert_allclose(d["dq"], u["dq"], **LOSS)
    np.testing.assert_allclose(d["head_losses"], u["head_losses"], **LOSS)
    np.testing.assert_allclose(d["loss"], u["loss"], **LOSS)
    # a cleared bit: exact zeros; and everything off the taken action
    assert np.all(d["dq"][c["masks"].T == 0] == 0.0)
    off = np.ones((B, A), bool)
    off[np.arange(B), c["actions"]] = False
    assert np.all(d["dq"][:, off] == 0.0)
    again = _launch(rlx, dev, *args, huber)
    for k in ("dq", "loss", "head_losses", "td"):
        assert again[k].tobytes() == d[k].tobytes(), k


@pytest.mark.parametrize("B,A,K", [(32, 6, 10), (37, 2, 32), (256, 18, 32), (1, 3, 1), (100, 18, 7)])
def test_all_bits_set_equals_dqn_head_loss_head_by_head_bit_for_bit(rlx, dev, B, A, K):
    import torch
    rng = np.random.RandomState(B + A + K)
    q, qn, qs = [(rng.randn(K, B, A) * 2).astype(np.float32) for _ in range(3)]
    actions = rng.randint(0, A, size=B)
    rewards = rng.randn(B).astype(np.float32)
    go = rng.rand(B) < 0.3
    for huber in (True, False):
        d = _launch(rlx, dev, q, qn, qs, actions, rewards, go, np.ones((B, K), np.int64), huber)
        for h in range(K):
            dq = torch.full((B, A), float("nan"), dtype=torch.float32, device=dev)
            loss = torch.zeros(1, dtype=torch.float32, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            rlx.dqn_head_loss(_t(q[h], dev), A, _t(qn[h], dev), _t(qs[h], dev), A, _t(actions.astype(np.int32), dev),
                              _t(rewards, dev), _t(go.astype(np.uint8), dev), None, 0.99, B, A, int(huber), 1.0, dq, A,
                              None, None, A, loss, status, 0)
            assert dq.cpu().numpy().tobytes() == np.ascontiguousarray(d["dq"][h]).tobytes(), (h, huber)
            assert loss.cpu().numpy().tobytes() == d["head_losses"][h:h + 1].tobytes(), (h, huber)
        total = np.float32(0)
        for h in range(K):
            total = np.float32(total + d["head_losses"][h])
        assert total.tobytes() == d["loss"].tobytes()


@pytest.mark.parametrize("huber", [True, False])
def test_a_nan_in_a_selector_row_wins_that_heads_selection(rlx, dev, huber):
    """np.argmax (bootstrapped_ref.update): the first NaN of a head's selector row is that head's greedy action.  The target
    net is finite, so the targets stay finite and are read at the NaN's column"""
    B, A, K = 37, 3, 4
    rng = np.random.RandomState(5)
    q, qn, qs = [(rng.randn(K, B, A) * 2).astype(np.float32) for _ in range(3)]
    qs[0, 5], qs[1, 5], qs[3, 6], qs[2, 36] = [1, np.nan, 3], [np.nan, 3, np.nan], [2, 2, np.nan], [3, np.nan, np.nan]
    actions, rewards, go = rng.randint(0, A, size=B), rng.randn(B).astype(np.float32), rng.rand(B) < 0.3
    masks = np.ones((B, K), np.int64)
    d = _launch(rlx, dev, q, qn, qs, actions, rewards, go, masks, huber)
    u = R.update(q, qn, qs, actions, rewards, go, masks, 0.99, huber)
    assert u["a_star"][5, 0] == 1 and u["a_star"][5, 1] == 0 and u["a_star"][6, 3] == 2 and u["a_star"][36, 2] == 1
    assert d["status"] == 0 and np.array_equal(d["a_star"], u["a_star"])
    taken = np.ascontiguousarray(u["td_targets"][:, np.arange(B), actions].T)
    assert np.isfinite(taken).all() and np.array_equal(d["td"].view(np.uint32), taken.view(np.uint32))
    np.testing.assert_allclose(d["dq"], u["dq"], **LOSS)
    np.testing.assert_allclose(d["loss"], u["loss"], **LOSS)


def test_loss_kernel_flags_an_action_out_of_range_and_refuses_large_shapes(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    rng = np.random.RandomState(2)
    q = rng.randn(4, 5, 3).astype(np.float32)
    d = _launch(rlx, dev, q, q, q, np.array([0, 3, 1, 2, -1]), np.zeros(5), np.zeros(5, bool), np.ones((5, 4)), True)
    assert d["status"] == 1 and d["ticket"] == 0 and np.all(d["dq"][:, [1, 4]] == 0) and np.isfinite(d["dq"]).all()
    z = torch.zeros(4096, dtype=torch.float32, device=dev)
    i = torch.zeros(4096, dtype=torch.int32, device=dev)
    for B, K, A in ((1, 33, 2), (1, 2, 19), (257, 2, 2)):
        with pytest.raises(RlxError):
            rlx.bootstrapped_dqn_head_loss(z, K * A, z, z, K * A, i, z, i, i, 0.99, B, K, A, 1, 1.0, z, K * A, z, i, z, i,
                                           None, None, None, 0)


def _act(rlx, dev, q, heads, vote, u, ra, tie, eps):
    import torch
    n, K, A = q.shape
    vals = torch.full((n, A), float("nan"), dtype=torch.float32, device=dev)
    acts = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rlx.bootstrapped_egreedy(_t(q.reshape(n, K * A), dev), K * A, K, _t(np.asarray(heads, np.int32), dev), int(vote),
                             _t(np.asarray(u, np.float64), dev), _t(np.asarray(ra, np.int32), dev),
                             _t(np.asarray(tie, np.float64), dev), float(eps), n, A, vals, acts, 0)
    return acts.cpu().numpy(), vals.cpu().numpy()


@pytest.mark.parametrize("s", range(len(ACT_CASES)))
def test_acting_kernel_gives_the_golden_actions(rlx, dev, gold, s):
    q, heads = gold["act%d_q" % s], gold["act%d_heads" % s]
    for name, vote in (("train", False), ("test", True)):
        u, ra, tie = acting_draws(gold, s, vote)
        acts, vals = _act(rlx, dev, q, heads, vote, u, ra, tie, 0.5)
        assert acts.tolist() == gold["act%d_%s_actions" % (s, name)].tolist()
        assert np.array_equal(vals.astype(np.float64), gold["act%d_%s_values" % (s, name)])


def test_acting_kernel_equals_the_restatement_on_random_cases(rlx, dev):
    rng = np.random.RandomState(5)
    for n, A, K in ((1, 2, 1), (7, 6, 10), (64, 18, 32), (130, 3, 5), (9, 4, 32)):
        q = rng.randint(-2, 3, size=(n, K, A)).astype(np.float32) if n % 2 else rng.randn(n, K, A).astype(np.float32)
        heads = rng.randint(0, K, size=n)
        u, ra, tie = rng.rand(n), rng.randint(0, A, size=n), rng.rand(n, A)
        for vote in (False, True):
            acts, vals = _act(rlx, dev, q, heads, vote, u, ra, tie, 0.3)
            ref = R.action_values(q, heads, vote)
            assert np.array_equal(vals, ref)
            assert acts.tolist() == R.egreedy(ref, u, ra, tie, 0.3).tolist()


@pytest.mark.parametrize("kind", ["vector", "image"])
def test_mask_column_round_trip_through_store_wrap_around_and_gather(dev, kind):
    import torch
    from coach_amd.memories.memory import MemoryGranularity
    from coach_amd.memories.non_episodic.experience_replay import ExperienceReplay
    n_env, cap = 2, 12
    rng = np.random.RandomState(4)
    if kind == "vector":
        kw, shape, dt = dict(observation_shape=(3,)), (3,), np.float32
    else:
        kw, shape, dt = dict(observation_shape=(84, 84), stack=4, min_episode_length=1), (84, 84), np.uint8
    mem = ExperienceReplay((MemoryGranularity.Transitions, cap), device=dev, n_env=n_env, mask_column=True, **kw)
    plain = ExperienceReplay((MemoryGranularity.Transitions, cap), device=dev, n_env=n_env, **kw)
    assert plain.mask is None and "mask" not in plain._batch_buffers(4)
    obs = lambda: _t((rng.rand(n_env, *shape) * 200).astype(dt), dev)
    mem.reset(obs())
    with pytest.raises(ValueError):
        mem.store(_t(np.zeros(n_env, np.int32), dev), _t(np.zeros(n_env, np.float32), dev),
                  _t(np.zeros(n_env, np.uint8), dev), obs(), obs())
    written = []                                           # (word, reward) per stored row, in store order
    for step in range(11):                                 # 22 rows through a 12 (+2) row ring
        words = rng.randint(0, 2 ** 32, size=n_env, dtype=np.uint64).astype(np.uint32)
        rew = rng.randn(n_env).astype(np.float32)
        mem.store(_t(rng.randint(0, 2, n_env).astype(np.int32), dev), _t(rew, dev), _t(np.zeros(n_env, np.uint8), dev),
                  obs(), obs(), masks=_t(words.view(np.int32), dev), episode_end=False)
        written += list(zip(words.tolist(), rew.tolist()))
    assert mem.num_transitions() == cap
    alive = written[-cap:]
    idx = np.array([0, 11, 5, 5, 3, 10, 1])
    b = mem.collate(idx, len(idx))
    got = b.info("mask").cpu().numpy().view(np.uint32)
    assert got.tolist() == [alive[i][0] for i in idx]
    assert b.rewards().cpu().numpy().tolist() == [alive[i][1] for i in idx]       # the same rows as the other columns
    # set_masks rewrites words of rows already written
    rows = mem.physical_rows(np.array([2, 7]))
    mem.set_masks(_t(rows, dev), _t(np.array([7, 0x80000001], np.uint32).view(np.int32), dev), 2)
    got = mem.collate(np.array([2, 7, 0]), 3).info("mask").cpu().numpy().view(np.uint32)
    assert got.tolist() == [7, 0x80000001, alive[0][0]]
    mem.check_status()


def _oracle_update(o, net, K, A, obs, actions, rewards, go, masks, huber):
    """the restatement on the DEVICE's own head outputs (the Double-DQN selection is a discrete decision on values that
    agree to rounding only), then the oracle's backward pass and TF1 Adam on its gradient."""
    B = obs.shape[0]
    split = lambda t: np.ascontiguousarray(t.cpu().numpy().reshape(B, K, A).transpose(1, 0, 2))
    u = R.update(split(net.last_q), split(net.last_q_next), split(net.last_q_sel), actions, rewards, go, masks, 0.99,
                 huber)
    np.testing.assert_allclose(o.q(obs), net.last_q.cpu().numpy().reshape(B, K * A), rtol=2e-4, atol=2e-5)
    o.tower.backward(o.head.backward(R.columns(u["dq"])) * np.float32(o.head_gradient_rescale))
    o.adam_step(1.0)
    return u["loss"]


@pytest.mark.parametrize("kind", ["vector", "image"])
def test_network_update_equals_the_composed_oracle(dev, kind):
    import torch
    from coach_amd.nn.networks import BootstrappedDQNNet
    from oracle.agents import DQNOracle
    rng = np.random.RandomState(7)
    if kind == "vector":
        shape, A, K, B, updates, lr = (4,), 2, 10, 32, 12, 2.5e-4
    else:
        shape, A, K, B, updates, lr = (84, 84, 4), 6, 10, 8, 1, 2.5e-4
    net = BootstrappedDQNNet(dev, shape, A, K, learning_rate=lr, seed=3, head_gradient_rescale=1.0 / K)
    o = DQNOracle(net.params.named_arrays(), shape, K * A, lr=lr, head_gradient_rescale=1.0 / K)
    # every head's block was initialised with its own fan-out
    w = net.params.named_arrays()["main/q_head/dense/kernel"][0]
    limit = np.sqrt(6.0 / (w.shape[0] + A))
    assert w.shape[1] == K * A and np.abs(w).max() <= limit and np.abs(w).max() > np.sqrt(6.0 / (w.shape[0] + K * A))
    for u in range(updates):
        if kind == "vector":
            obs, nxt = rng.randn(B, 4).astype(np.float32), rng.randn(B, 4).astype(np.float32)
        else:
            obs = rng.randint(0, 256, size=(B,) + shape).astype(np.uint8)
            nxt = rng.randint(0, 256, size=(B,) + shape).astype(np.uint8)
        actions = rng.randint(0, A, size=B)
        rewards = rng.choice([0.0, 1.0], size=B).astype(np.float32)
        go = rng.rand(B) < 0.1
        masks = (rng.rand(B, K) < 0.6).astype(np.int64)
        loss = net.learn_from_batch(_t(obs, dev), _t(nxt, dev), B, _t(actions.astype(np.int32), dev), _t(rewards, dev),
                                    _t(go.astype(np.uint8), dev), _t(R.mask_words(masks).view(np.int32), dev), 0.99)
        ref = _oracle_update(o, net, K, A, obs, actions, rewards, go, masks, True)
        np.testing.assert_allclose(float(loss.item()), ref, **LOSS)
        if u % 5 == 4:
            net.update_target(1.0)
            o.update_target(1.0)
    net.check_status()
    wd, wo = net.params.named_arrays(), o.weights()
    print("\n  %s: %d updates, weights max abs diff %.3e" % (
        kind, updates, max(float(np.abs(wd[n][0] - t[0]).max()) for n, t in wo.items())))
    for name, towers in wo.items():
        np.testing.assert_allclose(wd[name][0], towers[0], err_msg=name, **WEIGHTS)
    assert torch.isfinite(net.params.weights).all()


def test_torso_gets_one_kth_of_the_head_gradients_and_the_heads_all_of_theirs(dev):
    import torch
    from coach_amd.nn.networks import BootstrappedDQNNet
    A, K, B = 3, 8, 32                                      # 1 / 8: the scaling is exact in binary
    rng = np.random.RandomState(1)
    obs, nxt = rng.randn(B, 4).astype(np.float32), rng.randn(B, 4).astype(np.float32)
    args = (_t(obs, dev), _t(nxt, dev), B, _t(rng.randint(0, A, size=B).astype(np.int32), dev),
            _t(rng.randn(B).astype(np.float32), dev), _t((rng.rand(B) < 0.2).astype(np.uint8), dev),
            _t(R.mask_words(rng.rand(B, K) < 0.5).view(np.int32), dev), 0.99)
    grads = []
    for scale in (1.0, 1.0 / K):
        net = BootstrappedDQNNet(dev, (4,), A, K, seed=3, head_gradient_rescale=scale)
        net.learn_from_batch(*args)
        grads.append({n: v[0] for n, v in net.params.named_arrays(net.params.grads).items()})
    full, scaled = grads
    for name in full:
        if "q_head" in name:
            assert np.array_equal(full[name], scaled[name]), name
        else:
            assert np.abs(full[name]).max() > 0
            assert np.array_equal(full[name] * np.float32(1.0 / K), scaled[name]), name


def _agent(dev, n_env=1, p=1.0, K=4, use_graphs=None, seed=5, image=False, L=5):
    from coach_amd.agents.bootstrapped_dqn_agent import BootstrappedDQNAgent, BootstrappedDQNAgentParameters
    from coach_amd.core_types import EnvironmentSteps
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    from coach_amd.memories.memory import MemoryGranularity
    ap = BootstrappedDQNAgentParameters()
    ap.seed = seed
    net = ap.network_wrappers["main"]
    net.batch_size = 16
    net.heads_parameters[0].num_output_head_copies = K
    net.heads_parameters[0].rescale_gradient_from_head_by_factor = 1.0 / K
    ap.exploration.architecture_num_q_heads = K
    ap.exploration.bootstrapped_data_sharing_probability = p
    ap.memory.max_size = (MemoryGranularity.Transitions, 60)
    ap.algorithm.num_consecutive_playing_steps = EnvironmentSteps(1)
    ap.algorithm.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(7)
    env = SyntheticVectorEnvironment(SyntheticVectorEnvironmentParameters(
        "image" if image else "vector", n_env, (84, 84) if image else (6,), 3, episode_length=L, seed=3), dev)
    return BootstrappedDQNAgent(ap, env, dev, use_graphs=use_graphs)


def _run(a, heatup, train):
    from coach_amd.core_types import RunPhase
    random.seed(9); np.random.seed(9)
    a.phase = RunPhase.HEATUP
    for _ in range(heatup):
        a.act()
    a.phase = RunPhase.TRAIN
    for _ in range(train):
        a.step_and_train()
    a.check_status()


def test_prioritized_memory_is_refused(dev):
    from coach_amd.agents.bootstrapped_dqn_agent import BootstrappedDQNAgent, BootstrappedDQNAgentParameters
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    from coach_amd.memories.non_episodic.prioritized_experience_replay import PrioritizedExperienceReplayParameters
    p = BootstrappedDQNAgentParameters()
    p.memory = PrioritizedExperienceReplayParameters()
    env = SyntheticVectorEnvironment(SyntheticVectorEnvironmentParameters("vector", 1, (4,), 2, episode_length=5, seed=3),
                                     dev)
    with pytest.raises(ValueError, match="priorities"):
        BootstrappedDQNAgent(p, env, dev)


def test_graph_replay_equals_eager(dev):
    import torch
    g, e = _agent(dev, n_env=2, p=0.6, use_graphs=True), _agent(dev, n_env=2, p=0.6, use_graphs=False)
    for a in (g, e):
        _run(a, 12, 40)
    assert any(k[0] == "learn" for k in g._graphs) and not e._graphs and not g._step_graph_ok()
    ng, ne = g.networks["main"], e.networks["main"]
    assert torch.equal(ng.params.weights, ne.params.weights) and torch.equal(ng.target, ne.target)
    assert torch.equal(ng.adam.v, ne.adam.v) and not torch.equal(ng.params.weights, ng.target)
    for col in ("obs", "next_obs", "action", "reward", "game_over", "mask"):
        assert torch.equal(getattr(g.memory, col), getattr(e.memory, col)), col
    assert torch.equal(ng.loss, ne.loss) and torch.equal(g.actions, e.actions)
    assert set(g.signals) == {"Loss", "Grads (unclipped)", "Q"} and g.signals["Q"].numel() == 16 * 4 * 3


def test_checkpoint_round_trip(dev, tmp_path):
    import torch
    from coach_amd.checkpoint import restore_checkpoint, save_checkpoint
    from coach_amd.core_types import RunPhase
    a = _agent(dev, n_env=2, p=0.6)
    _run(a, 12, 17)
    save_checkpoint(a, str(tmp_path))
    b = _agent(dev, n_env=2, p=0.6, seed=99)
    restore_checkpoint(b, str(tmp_path))
    assert b.exploration_policy.selected_head.tolist() == a.exploration_policy.selected_head.tolist()
    assert torch.equal(a.memory.mask, b.memory.mask)
    assert b._needs_head.tolist() == a._needs_head.tolist() and (b._open_rows is None) == (a._open_rows is None)
    host = (random.getstate(), np.random.get_state())       # both continue from the host streams the checkpoint holds
    for x in (a, b):
        random.setstate(host[0]); np.random.set_state(host[1])
        for _ in range(15):
            x.step_and_train()
    assert torch.equal(a.networks["main"].params.weights, b.networks["main"].params.weights)
    assert torch.equal(a.memory.mask, b.memory.mask) and torch.equal(a.memory.action, b.memory.action)
    assert a.exploration_policy.selected_head.tolist() == b.exploration_policy.selected_head.tolist()
    assert b.phase == RunPhase.TRAIN


@pytest.mark.parametrize("p", [1.0, 0.5])
def test_stored_masks_equal_the_hosts_draws_in_a_multi_env_loop(dev, p):
    a = _agent(dev, n_env=3, p=p, K=5)
    a.debug_masks = []
    _run(a, 9, 30)
    drawn = {}                                            # (the last step's rows wait for their draw: not visible yet)
    for row, word in a.debug_masks:                       # later writes of a ring row replace earlier ones
        drawn[row] = word
    mem = a.memory
    stored = mem.mask.cpu().numpy().view(np.uint32)
    rows = mem.physical_rows(np.arange(mem.num_transitions()))
    assert len(rows) > 30 and all(int(r) in drawn for r in rows)
    assert [int(stored[r]) for r in rows] == [drawn[int(r)] for r in rows]
    assert (p < 1.0) == (len(set(drawn.values())) > 1) and max(drawn.values()) < 2 ** 5
    # what an update reads is those words
    b = mem.collate(np.arange(16), 16)
    assert b.info("mask").cpu().numpy().view(np.uint32).tolist() == [drawn[int(r)] for r in rows[:16]]
    ev = a.evaluate_episodes(1)                            # the vote; nothing stored, heads re-selected afterwards
    assert np.isfinite(ev) and mem.num_transitions() == len(rows)
