"""Batch RL on the GPU above the kernels: the episodic replay as a frozen dataset (split, shuffled epochs, refusals)
against the reference memory's recording, and the kNN action mask (coach_amd/agents/ddqn_bcq_agent.py: key sets,
average_dist, select_actions up to the argmax) against the reference agent's recording (tests/golden/bcq.npz)."""
import os
import random

import numpy as np
import pytest

import bcq_ref as R
from test_bcq_ref import CASES, MEMORIES, case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "bcq.npz"))


def _filled_memory(dev, lengths, ratio, n_env=1):
    """the device memory holding episodes of `lengths` in that (completion) order; every transition's reward is its
    index in the reference's transitions list.  n_env = 2 is for equal-length episodes (the envs end together: ties
    complete in env order)."""
    import torch
    from coach_amd.memories.episodic.episodic_experience_replay import EpisodicExperienceReplay
    from coach_amd.memories.memory import MemoryGranularity
    m = EpisodicExperienceReplay((MemoryGranularity.Transitions, 1000), max_episode_length=max(lengths), device=dev,
                                 n_env=n_env, observation_shape=(1,), min_episode_length=1, train_to_eval_ratio=ratio)
    m.reset(torch.zeros(n_env, 1, device=dev))
    assert len(lengths) % n_env == 0
    start = 0
    for g in range(0, len(lengths), n_env):
        group = lengths[g:g + n_env]
        assert len(set(group)) == 1
        firsts = start + np.concatenate([[0], np.cumsum(group)[:-1]])
        for j in range(group[0]):
            done = j == group[0] - 1
            m.store(torch.zeros(n_env, dtype=torch.int32, device=dev),
                    torch.tensor(firsts + j, dtype=torch.float32, device=dev),
                    torch.full((n_env,), int(done), dtype=torch.uint8, device=dev),
                    torch.zeros(n_env, 1, device=dev), torch.zeros(n_env, 1, device=dev),
                    dones_host=np.full(n_env, done))
        start += sum(group)
    assert m.episode_lengths() == list(lengths) and m.num_transitions_in_complete_episodes() == sum(lengths)
    return m


@pytest.mark.parametrize("i,n_env", [(0, 1), (1, 1), (2, 1), (1, 2)])
def test_memory_split_and_epochs_equal_the_reference_memory(dev, gold, i, n_env):
    lengths, ratio = MEMORIES[i]
    p = "mem%d_" % i
    m = _filled_memory(dev, lengths, ratio, n_env)
    with pytest.raises(TypeError):
        next(m.get_shuffled_training_data_generator(4))                    # range(None): no split yet, as in the reference
    m.freeze()
    m.prepare_evaluation_dataset()
    assert m.get_last_training_set_episode_id() == int(gold[p + "episode_id"])
    assert m.last_training_set_transition_id == int(gold[p + "transition_id"])
    assert [b - a for a, b in m.evaluation_dataset_as_episodes] == gold[p + "eval_lengths"].tolist()
    first, end = m.evaluation_dataset_as_transitions
    assert list(range(first, end)) == gold[p + "eval_transitions"].tolist()
    ev = m.gather(m.physical_rows(np.arange(first, end)), end - first)["reward"].cpu().numpy()
    assert ev.tolist() == gold[p + "eval_transitions"].tolist()            # the ranges name the reference's transitions
    m._split_training_and_evaluation_datasets()                            # a second call changes nothing
    assert m.last_training_set_transition_id == int(gold[p + "transition_id"])
    random.seed(7)
    size = int(gold[p + "size"])
    for epoch in range(2):
        flat, sizes = [], []
        for batch in m.get_shuffled_training_data_generator(size):
            got = batch.rewards().cpu().numpy()
            assert got.shape == (batch.size,)
            sizes.append(batch.size)
            flat += got.astype(np.int64).tolist()
        assert sizes == gold[p + "epoch%d_sizes" % epoch].tolist()
        assert flat == gold[p + "epoch%d_flat" % epoch].tolist()
    m.check_status()


def test_a_frozen_memory_refuses_stores_and_the_split_keeps_the_reference_errors(dev, gold):
    import torch
    m = _filled_memory(dev, [3, 3], 1)
    with pytest.raises(ValueError) as e:
        m.prepare_evaluation_dataset()
    assert str(e.value) == str(gold["mem_error_ratio_1"])
    m.train_to_eval_ratio = 0.9                                              # round(5.4) = 5: the last episode trains too
    with pytest.raises(ValueError, match="train_to_eval_ratio is too high causing the evaluation set to be empty"):
        m.prepare_evaluation_dataset()
    assert (m.get_last_training_set_episode_id(), m.last_training_set_transition_id) == (1, 6)
    assert m.frozen is False
    m.assert_not_frozen()
    m.freeze()
    args = (torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, device=dev),
            torch.zeros(1, dtype=torch.uint8, device=dev), torch.zeros(1, 1, device=dev), torch.zeros(1, 1, device=dev))
    with pytest.raises(AssertionError) as e:
        m.store(*args, dones_host=np.array([False]))
    assert str(e.value) == str(gold["mem_frozen_error"])
    m.store(*args, record=False)                                             # acting during evaluation stores nothing
    assert m.num_transitions() == 6 and m.open_transitions() == 0
    batches = list(m.shuffled_training_index_batches(4))
    assert [len(b) for b in batches] == [4, 2] and sorted(sum(batches, [])) == list(range(6))


@pytest.mark.parametrize("name", sorted(CASES))
def test_action_mask_equals_the_reference_agent(dev, gold, name):
    import torch
    from coach_amd.agents.ddqn_bcq_agent import KNNActionMask, KNNParameters
    c = case(gold, name)
    B, A, W, counts, n_zero = CASES[name]
    p = KNNParameters()
    p.average_dist_coefficient = float(c["coefficient"])
    mask = KNNActionMask(dev, A, p, seed=3, rank=1)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    avg = mask.build(t(c["emb"]), t(c["data_actions"].astype(np.int32)))
    assert mask.counts == counts and sum(counts) == mask.keys.shape[0]      # every stored transition once
    assert np.array_equal(mask.keys.cpu().numpy(), c["keys"]) and mask.set_offsets.cpu().numpy().tolist() == \
        c["set_offsets"].tolist()
    assert avg == float(c["average_dist"]) or (np.isinf(avg) and np.isinf(float(c["average_dist"])))
    if name.endswith("f"):
        mask.average_dist = float(c["threshold"]) / float(c["coefficient"])  # the recording's finite stand-in
    assert mask.threshold == float(c["threshold"]) or np.isinf(mask.threshold)
    event = torch.tensor([5], dtype=torch.int64, device=dev)
    fam = torch.empty(B, A, dtype=torch.float32, device=dev)
    sel = mask.selector(t(c["q_sel"]), t(c["emb_next"]), event, familiarity=fam).cpu().numpy()
    assert np.array_equal(fam.cpu().numpy().view(np.uint32), c["familiarity"].view(np.uint32))
    want, m, zero = R.masked_selector(c["q_sel"], c["familiarity"], float(c["threshold"]), seed=3, rank=1, event=5)
    assert np.array_equal(sel.view(np.uint32), want.view(np.uint32)) and int(mask.zero_rows.item()) == n_zero
    assert np.array_equal(np.isneginf(sel) | zero[:, None], c["mask"]) and np.array_equal(zero, c["zero_rows"])
    assert np.array_equal(np.argmax(sel, axis=1)[~zero], c["selected"][~zero])
    # a captured graph follows the event: the same replay draws other uniforms after the counter moved
    if n_zero:
        q, e = t(c["q_sel"]), t(c["emb_next"])
        out = torch.empty(B, A, dtype=torch.float32, device=dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mask.selector(q, e, event, familiarity=fam, out=out)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                mask.selector(q, e, event, familiarity=fam, out=out)
        torch.cuda.current_stream().wait_stream(side)
        for ev in (5, 6):
            event.fill_(ev)
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32),
                                  R.masked_selector(c["q_sel"], c["familiarity"], float(c["threshold"]), 3, 1, ev)[0]
                                  .view(np.uint32))


def test_action_mask_refusals(dev):
    import torch
    from coach_amd.agents.ddqn_bcq_agent import KNNActionMask, KNNParameters, NNImitationModelParameters
    with pytest.raises(ValueError, match="NNImitationModelParameters is not served yet"):
        KNNActionMask(dev, 2, NNImitationModelParameters())
    with pytest.raises(ValueError, match="1 to 18 actions"):
        KNNActionMask(dev, 19)
    p = KNNParameters()
    p.knn_size = 3
    mask = KNNActionMask(dev, 2, p)
    emb = torch.zeros(6, 4, device=dev)
    with pytest.raises(RuntimeError, match="built first"):
        mask.distances(emb)
    with pytest.raises(ValueError, match="action 1 has 4 keys, knn_size is 3"):
        mask.build(emb, np.array([0, 1, 1, 0, 1, 1]))
    with pytest.raises(ValueError, match="an action outside"):
        mask.build(emb, np.array([0, 1, 2, 0, 1, 1]))
    assert mask.build(emb, np.array([0, 1, 1, 0, 1, 0])) == 0.0             # identical states: every distance is 0


def test_network_update_with_a_given_selector(dev):
    """DQNNet.learn_from_batch(selector=): the network's own online Q values on s' as the selector give Double DQN's
    update bit for bit — also on a network whose default path is the one-launch small-MLP update, which a selector
    bypasses; a masked selector's -inf entries are never chosen."""
    import torch
    from coach_amd.nn.networks import DQNNet

    class LayerByLayerDQNNet(DQNNet):
        FUSED_MLP = False
    A, B = 3, 32
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ddqn, own, fusable = LayerByLayerDQNNet(dev, (4,), A, seed=3), LayerByLayerDQNNet(dev, (4,), A, seed=3), \
        DQNNet(dev, (4,), A, seed=3)
    masked, floored = LayerByLayerDQNNet(dev, (4,), A, seed=3), LayerByLayerDQNNet(dev, (4,), A, seed=3)
    assert ddqn._fused is None and fusable._fused is not None
    rng = np.random.RandomState(11)
    for u in range(6):
        size = B if u < 5 else 7                                             # an epoch's last batch is smaller
        common = (t(rng.randn(size, 4).astype(np.float32)), t(rng.randn(size, 4).astype(np.float32)), size,
                  t(rng.randint(0, A, size=size).astype(np.int32)), t(rng.choice([0.0, 1.0], size=size).astype(np.float32)),
                  t((rng.rand(size) < 0.1).astype(np.uint8)))
        la = ddqn.learn_from_batch(*common, 0.99, double_dqn=True).clone()
        for net in (own, fusable):
            sel = net.q_values(common[1], size, tag="next_o", noise_pass="online_next").data.view(size, A).clone()
            assert torch.equal(la, net.learn_from_batch(*common, 0.99, selector=sel)), u
        drop = t(rng.rand(size, A) < 0.4)
        drop[:, 0] &= ~drop.all(dim=1)                                       # every row keeps an action
        for net, low in ((masked, float("-inf")), (floored, -1e30)):
            sel = net.q_values(common[1], size, tag="next_o", noise_pass="online_next").data.view(size, A).clone()
            sel[drop] = low
            net.learn_from_batch(*common, 0.99, selector=sel)
        if u == 2:
            for net in (ddqn, own, fusable, masked, floored):
                net.update_target(1.0)
    for net in (ddqn, own, fusable, masked, floored):
        net.check_status()
    for net in (own, fusable):
        assert torch.equal(ddqn.params.weights, net.params.weights) and torch.equal(ddqn.adam.m, net.adam.m)
    assert torch.equal(masked.params.weights, floored.params.weights)
    assert not torch.equal(masked.params.weights, ddqn.params.weights) and torch.isfinite(masked.params.weights).all()
    with pytest.raises(ValueError, match="selector is a contiguous fp32"):
        ddqn.learn_from_batch(*common, 0.99, selector=torch.zeros(size, A + 1, device=dev))


# ------------------------------------------------------------------------------ the agent and the graph manager
def _tiny_run(dev, use_graphs, **kw):
    from coach_amd.core_types import TrainingSteps
    from coach_amd.presets.CartPole_DDQN_BCQ_BatchRL import make
    gm = make(dataset_size=600, heatup_steps=200, reward_model_num_epochs=2, improve_epochs=2, batch_size=32,
              evaluation_episodes=1, **kw)
    gm.device, gm.use_graphs = dev, use_graphs
    gm.agent_params.algorithm.num_steps_between_copying_online_weights_to_target = TrainingSteps(5)
    gm.create_graph()
    gm.improve()
    return gm


def test_the_reference_presets_parameters_run(dev):
    """the graph manager whose parameters equal the reference preset text's dump (tests/golden/bcq_preset.json, checked
    on the CPU by test_bcq_ref.py) — imitation-model wrapper and softmax_temperature included — builds and trains: a
    smaller dataset, one reward epoch, one epoch"""
    from test_bcq_ref import reference_equivalent_manager
    gm = reference_equivalent_manager(dataset_size=1500, heatup_steps=500, reward_model_num_epochs=1, improve_epochs=1,
                                      evaluation_episodes=1)
    gm.device = dev
    gm.create_graph()
    gm.improve()
    a = gm.trained_agent
    assert set(a.networks) == {"main", "reward_model"} and a.training_epoch == 1 and a.training_iteration > 0
    assert a.networks["main"].l2_regularization == 0.0001 and a.networks["reward_model"].l2_regularization == 0
    assert a.ap.algorithm.reward_rescale == 1 / 200. and gm.experience_generating_agent.ap.algorithm.reward_rescale == 1 / 200.
    assert int(a.zero_rows_total.item()) >= int(a.zero_row_updates.item()) >= 0


def test_tiny_batch_rl_run_end_to_end(dev):
    import torch
    runs = [_tiny_run(dev, g) for g in (True, False)]
    a, b = (gm.trained_agent for gm in runs)
    for name in ("main", "reward_model"):                                    # graphs on and off: identical weights
        assert torch.equal(a.networks[name].params.weights, b.networks[name].params.weights), name
    assert torch.equal(a.networks["main"].target, b.networks["main"].target)
    gm, mem = runs[0], a.memory
    assert mem is gm.experience_generating_agent.memory and mem.frozen
    n, train = mem.num_transitions_in_complete_episodes(), mem.last_training_set_transition_id
    assert 0 < train < n <= 600 and mem.num_transitions() == n               # evaluation stored nothing
    assert sum(a.mask.counts) == n == a.mask.keys.shape[0]                   # every stored transition is a key once
    acts = mem.gather(mem.physical_rows(np.arange(n)), n)["action"].cpu().numpy()
    assert a.mask.counts == [int((acts == k).sum()) for k in range(2)]
    updates = 2 * -(-train // 32)
    assert a.training_epoch == 2 == gm.epochs and a.training_iteration == updates == gm.training_steps
    assert a.target_copies == updates // 5 and a.ap.algorithm.num_consecutive_playing_steps.num_steps == 0
    assert np.isfinite(a.mask.average_dist) and a.mask.average_dist > 0
    assert torch.isfinite(a.networks["main"].params.weights).all() and len(a.reward_model_losses) == 2
    assert 0 <= int(a.zero_row_updates.item()) <= updates == int(b.training_iteration)
    evals = [r for r in gm.logger.rows if r.get("Evaluation Reward", "") != ""]
    assert [int(r["Episode #"]) for r in evals] == [1, 2]                    # time is counted in epochs; only the trained
    assert gm.dataset_training_steps == gm.experience_generating_agent.training_iteration > 0   # agent's rows are logged
    with pytest.raises(AssertionError, match="Memory is frozen"):
        gm.heatup(type(gm.schedule.heatup_steps)(1))


def test_three_updates_follow_the_float64_restatement(dev):
    """Loss, gradient norm and weights of three whole updates — online Q on s', the kNN mask, the masked selector, the
    Double-DQN targets, the Q head's MSE, the L2 term (lambda * w on the gradient before Adam, lambda * sum w^2 / 2 on
    the loss), TF1 Adam, a target copy in between, the last batch smaller — against tests/bcq_ref.MLP64 under the
    project's tolerances.  The selection is a discrete decision on values that agree to rounding only, so it is taken
    from the device's selector, which is first checked against the restatement bit for bit."""
    import torch
    from coach_amd.agents.ddqn_bcq_agent import KNNActionMask
    from coach_amd.nn.networks import DQNNet
    from tolerances import LOSS, WEIGHTS
    A, W, lr, l2, discount = 3, 16, 1e-3, 0.01, 0.98
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rng = np.random.RandomState(21)
    net = DQNNet(dev, (4,), A, learning_rate=lr, seed=5, replace_mse_with_huber_loss=False)
    net.l2_regularization = l2
    ref = R.MLP64(net.params.named_arrays(), lr)
    assert [w.shape for w in ref.W] == [(4, 256), (256, 512), (512, A)] and "embedder" in ref.names[0]
    keys, key_actions = rng.randn(90, W).astype(np.float32), rng.randint(0, A, size=90)
    mask = KNNActionMask(dev, A, seed=2)
    mask.build(t(keys), key_actions)
    ks, off = R.key_sets(keys, key_actions, A)
    masked = differs = 0
    for u, B in enumerate((32, 32, 7)):
        obs, nxt = rng.randn(B, 4).astype(np.float32), rng.randn(B, 4).astype(np.float32)
        actions, rewards = rng.randint(0, A, size=B), rng.randn(B).astype(np.float32)
        go = rng.rand(B) < 0.2
        emb = (keys[rng.randint(90, size=B)] + rng.randn(B, W).astype(np.float32) * rng.uniform(0, 4.0, (B, 1))
               .astype(np.float32)).astype(np.float32)
        emb[0] += 100.0                                                       # a zero-confidence row
        q_sel = net.q_values(t(nxt), B, tag="next_o", noise_pass="online_next").data.view(B, A).clone()
        np.testing.assert_allclose(q_sel.cpu().numpy(), ref.forward(nxt), rtol=1e-4, atol=2e-6)
        event = torch.tensor([u], dtype=torch.int64, device=dev)
        sel = mask.selector(q_sel, t(emb), event)
        want, m, zero = R.masked_selector(q_sel.cpu().numpy(), R.nn_min_distance(emb, ks, off), mask.threshold, 2, 0, u)
        assert np.array_equal(sel.cpu().numpy().view(np.uint32), want.view(np.uint32)) and zero[0]
        masked += int(m.sum())
        chosen = np.argmax(want, axis=1)
        differs += int((chosen[~zero] != np.argmax(q_sel.cpu().numpy(), axis=1)[~zero]).sum())
        loss = net.learn_from_batch(t(obs), t(nxt), B, t(actions.astype(np.int32)), t(rewards), t(go.astype(np.uint8)),
                                    discount, selector=sel)
        r = ref.update(obs, nxt, actions, rewards, go, discount, chosen, l2)
        print("\n  update %d (B=%d): loss %.6f vs %.6f (head %.6f), gradient norm %.6f vs %.6f"
              % (u, B, float(loss.item()), r["loss"], r["head_loss"], float(net.norm.item()), r["norm"]))
        assert r["loss"] - r["head_loss"] > 10 * LOSS["rtol"] * r["loss"]    # the L2 term is visible at this tolerance
        np.testing.assert_allclose(float(loss.item()), r["loss"], **LOSS)
        np.testing.assert_allclose(float(net.norm.item()), r["norm"], **LOSS)
        if u == 0:
            net.update_target(1.0)
            ref.copy_to_target()
    assert masked > 9 + 10 and differs > 0      # more than the three zero-confidence rows' entries; the mask changed choices
    net.check_status()
    w = net.params.named_arrays()
    worst = 0.0
    for i, name in enumerate(ref.names):
        for kind, arr in (("kernel", ref.W[i]), ("bias", ref.b[i])):
            worst = max(worst, float(np.abs(w[name + "/" + kind][0] - arr).max()))
            np.testing.assert_allclose(w[name + "/" + kind][0], arr, err_msg=name, **WEIGHTS)
    print("  weights max abs diff %.3e" % worst)
