"""The imitation model above the launches, on the GPU: ClassificationNet (predict, train_on_batch), ImitationActionMask
and the DDQN-BCQ agent with NNImitationModelParameters, in a tiny Batch RL run."""
import numpy as np
import pytest

import imitation_ref as R

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _t(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


# ------------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize("B,A", [(1, 2), (37, 3), (128, 18)])
def test_predict_equals_the_selectors_familiarity(rlx, dev, B, A):
    import torch
    from coach_amd.agents.ddqn_bcq_agent import ImitationActionMask, NNImitationModelParameters
    from coach_amd.nn.networks import ClassificationNet
    rng = np.random.RandomState(B)
    net = ClassificationNet(dev, (4,), A, embedder=[32], middleware=[16], seed=2)
    obs = _t((rng.randn(B, 4) * 3).astype(np.float32), dev)
    probs = net.predict(obs, B).cpu().numpy()
    z = net.logits(obs, B).data.view(B, A).cpu().numpy()
    assert np.array_equal(bits(probs), bits(R.softmax_parts(z)[0]))          # the one softmax, on the device's logits
    mask = ImitationActionMask(dev, A, NNImitationModelParameters(), net, seed=3, rank=1)
    q = _t(rng.randn(B, A).astype(np.float32), dev)
    fam = torch.empty(B, A, dtype=torch.float32, device=dev)
    event = torch.tensor([5], dtype=torch.int64, device=dev)
    sel = mask.selector(q, obs, event, familiarity=fam).cpu().numpy()
    assert np.array_equal(bits(fam.cpu().numpy()), bits(probs))              # bit for bit the network's predict
    want, _, m, zero = R.imitation_selector(q.cpu().numpy(), z, 0.35, seed=3, rank=1, event=5)
    assert np.array_equal(bits(sel), bits(want)) and int(mask.zero_rows.item()) == int(zero.sum())
    assert mask.threshold == float(np.float32(0.35)) != 0.35
    net.check_status()


def test_mask_and_network_refusals(dev):
    import torch
    from coach_amd.agents.ddqn_bcq_agent import ImitationActionMask, KNNParameters, NNImitationModelParameters
    from coach_amd.nn.networks import ClassificationNet
    net = ClassificationNet(dev, (4,), 3, embedder=[8], middleware=[8])
    with pytest.raises(ValueError, match="Unsupported action drop method"):
        ImitationActionMask(dev, 3, KNNParameters(), net)
    with pytest.raises(ValueError, match="1 to 18 actions"):
        ImitationActionMask(dev, 2, NNImitationModelParameters(), net)
    obs = torch.zeros(4, 4, device=dev)
    with pytest.raises(ValueError, match="exactly one of actions and labels"):
        net.train_on_batch(obs, 4)
    with pytest.raises(ValueError, match="contiguous fp32"):
        net.train_on_batch(obs, 4, labels=torch.zeros(4, 2, device=dev))
    with pytest.raises(ValueError, match="1 .. 18 actions"):
        ClassificationNet(dev, (4,), 19)
    big = torch.zeros(1025, 4, device=dev)
    with pytest.raises(ValueError, match="1 to 1024 rows"):
        net.train_on_batch(big, 1025, actions=torch.zeros(1025, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("mode", ["actions", "labels"])
def test_three_updates_follow_the_float64_restatement(dev, mode):
    """Loss (the SUM over the batch), gradient norm and weights of three train_on_batch calls — the last batch smaller,
    an L2 term — against tests/imitation_ref.MLP64 under tests/tolerances.py's LOSS and WEIGHTS: the tolerances of the
    existing network-parity test of a DQNNet regression update of the same widths (4-256-512-A,
    tests/test_bcq_agent.py::test_three_updates_follow_the_float64_restatement)."""
    from coach_amd.nn.networks import ClassificationNet
    from tolerances import LOSS, WEIGHTS
    A, lr, l2 = 3, 1e-3, 0.01
    rng = np.random.RandomState(21)
    net = ClassificationNet(dev, (4,), A, learning_rate=lr, l2_regularization=l2, seed=5)
    ref = R.MLP64(net.params.named_arrays(), "main/classification_head/output", lr)
    assert [w.shape for w in ref.W] == [(4, 256), (256, 512), (512, A)] and "embedder" in ref.names[0]
    for u, B in enumerate((32, 32, 7)):
        obs, actions = rng.randn(B, 4).astype(np.float32), rng.randint(0, A, size=B)
        labels = R.one_hot(actions, A).astype(np.float32)
        if mode == "labels" and u == 1:
            labels = (rng.rand(B, A) * 0.7).astype(np.float32)                # soft rows too
        if mode == "actions":
            loss = net.train_on_batch(_t(obs, dev), B, actions=_t(actions.astype(np.int32), dev))
        else:
            loss = net.train_on_batch(_t(obs, dev), B, labels=_t(labels, dev))
        r = ref.classification_update(obs, labels, l2)
        print("\n  update %d (B=%d): loss %.6f vs %.6f (head %.6f), gradient norm %.6f vs %.6f"
              % (u, B, float(loss.item()), r["loss"], r["head_loss"], float(net.norm.item()), r["norm"]))
        assert r["head_loss"] > 0.5 * B * np.log(A) * 0.5                     # a sum over the batch, not a mean
        np.testing.assert_allclose(float(loss.item()), r["loss"], **LOSS)
        np.testing.assert_allclose(float(net.norm.item()), r["norm"], **LOSS)
    net.check_status()
    w = net.params.named_arrays()
    for i, name in enumerate(ref.names):
        for kind, arr in (("kernel", ref.W[i]), ("bias", ref.b[i])):
            np.testing.assert_allclose(w[name + "/" + kind][0], arr, err_msg=name, **WEIGHTS)


# ------------------------------------------------------------------------------ the agent and the graph manager
def _tiny_run(dev, use_graphs=True, reward_epochs=2, **kw):
    from coach_amd.core_types import TrainingSteps
    from coach_amd.presets.CartPole_DDQN_BCQ_BatchRL import make
    gm = make(dataset_size=600, heatup_steps=200, reward_model_num_epochs=reward_epochs, improve_epochs=2, batch_size=32,
              evaluation_episodes=1, **kw)
    gm.device, gm.use_graphs = dev, use_graphs
    gm.agent_params.algorithm.num_steps_between_copying_online_weights_to_target = TrainingSteps(5)
    return gm


def test_batch_rl_run_with_the_imitation_models_mask(dev, rlx, monkeypatch):
    import torch
    calls = {"nn_min_distance": 0}
    inner = rlx.nn_min_distance

    def counted(*a):
        calls["nn_min_distance"] += 1
        return inner(*a)
    monkeypatch.setattr(rlx, "nn_min_distance", counted)
    runs = []
    for graphs in (True, False):
        gm = _tiny_run(dev, graphs, action_drop="nn")
        drop = gm.agent_params.algorithm.action_drop_method_parameters
        drop.imitation_model_num_epochs = 3
        drop.mask_out_actions_threshold = 0.6        # two actions: the less likely one is always masked, often both
        gm.create_graph()
        gm.improve()
        runs.append(gm)
    a, b = (gm.trained_agent for gm in runs)
    assert calls["nn_min_distance"] == 0                                     # no key sets, no distances
    assert set(a.networks) == {"main", "reward_model", "imitation_model"} and a.imitation
    for name in a.networks:                                                  # graphs on and off: identical weights
        assert torch.equal(a.networks[name].params.weights, b.networks[name].params.weights), name
    train = a.memory.last_training_set_transition_id
    batches = -(-train // 32)
    assert a.model_updates == R.reward_model_schedule(2, 3, batches)         # the restated interleaving
    assert len(a.reward_model_losses) == 2 and len(a.imitation_model_losses) == 3
    im = [float(x.item()) for x in a.imitation_model_losses]
    assert all(np.isfinite(im)) and im[-1] < im[0]                           # the classifier fits the logged actions
    assert a.training_epoch == 2 and a.training_iteration == 2 * batches
    assert int(a.zero_rows_total.item()) >= int(a.zero_row_updates.item()) > 0          # it counts zero rows
    assert torch.isfinite(a.networks["main"].params.weights).all()
    evals = [r for r in runs[0].logger.rows if r.get("Evaluation Reward", "") != ""]
    assert [int(r["Episode #"]) for r in evals] == [1, 2]
    for gm in runs:
        gm.check_status()


def test_the_knn_run_does_not_see_an_imitation_wrapper(dev):
    """KNNParameters with an imitation_model wrapper in the parameters: the wrapper is not built and the run's weights
    equal those of the run without it, bit for bit (the kNN path is untouched)."""
    import torch
    from copy import deepcopy
    from coach_amd.architectures.head_parameters import ClassificationHeadParameters
    plain, with_wrapper = _tiny_run(dev), _tiny_run(dev)
    w = with_wrapper.agent_params.network_wrappers
    w['imitation_model'] = deepcopy(w['main'])
    w['imitation_model'].heads_parameters = [ClassificationHeadParameters()]
    for gm in (plain, with_wrapper):
        gm.create_graph()
        gm.improve()
    a, b = plain.trained_agent, with_wrapper.trained_agent
    assert set(b.networks) == {"main", "reward_model"} and not b.imitation
    for name in a.networks:
        assert torch.equal(a.networks[name].params.weights, b.networks[name].params.weights), name
    assert a.mask.average_dist == b.mask.average_dist and a.model_updates == R.reward_model_schedule(2, 0, len(
        a.model_updates) // 2)


# ------------------------------------------------------------------------------------------------ Behavioral Cloning
def _bc_agent(dev, use_graphs, batch_size=32, seed=5, dataset=None, lr=1e-3):
    from coach_amd.agents.bc_agent import BCAgent, BCAgentParameters
    from coach_amd.core_types import CsvDataset, RunPhase
    from coach_amd.environments.cartpole_vector_environment import (
        CartPoleVectorEnvironment, CartPoleVectorEnvironmentParameters)
    from coach_amd.memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters
    p = BCAgentParameters()
    p.seed = seed
    p.network_wrappers["main"].batch_size = batch_size
    p.network_wrappers["main"].learning_rate = lr
    if dataset is not None:
        p.memory = EpisodicExperienceReplayParameters()
        p.memory.load_memory_from_file_path = CsvDataset(dataset)
    env = CartPoleVectorEnvironment(CartPoleVectorEnvironmentParameters(1, "CartPole-v0", seed=11), dev)
    agent = BCAgent(p, env, dev, use_graphs=use_graphs)
    agent.phase = env.phase = RunPhase.TRAIN
    return agent


@pytest.mark.parametrize("B", [1, 32])
def test_bc_updates_follow_the_float64_restatement(dev, B):
    """three BCAgent updates (targets of ones, no entropy term, one Adam step each), graphs on and off, against
    tests/imitation_ref.MLP64.bc_update under tests/tolerances.py's LOSS and WEIGHTS (the tolerances of
    tests/test_bcq_agent.py::test_three_updates_follow_the_float64_restatement, the same widths 4-256-512-A)."""
    import torch
    from coach_amd.core_types import DeviceBatch
    from tolerances import LOSS, WEIGHTS
    agents = [_bc_agent(dev, g, batch_size=B) for g in (True, False)]
    assert agents[0].imitation and not agents[0].is_on_policy and agents[0].networks["main"].beta_entropy == 0
    ref = R.MLP64(agents[0].networks["main"].params.named_arrays(), "main/policy_values_head/fc", 1e-3)
    assert [w.shape for w in ref.W] == [(4, 256), (256, 512), (512, 2)]
    rng = np.random.RandomState(B)
    obs_d = torch.zeros(B, 4, device=dev)
    act_d = torch.zeros(B, dtype=torch.int32, device=dev)
    for u in range(3):                               # the third replays the captured graph on new data in the same buffers
        obs, actions = rng.randn(B, 4).astype(np.float32), rng.randint(0, 2, size=B)
        obs_d.copy_(_t(obs, dev))
        act_d.copy_(_t(actions.astype(np.int32), dev))
        batch = DeviceBatch(B, {"observation": obs_d}, {"observation": obs_d}, act_d, None, None, info={})
        losses = [float(a.learn_from_batch(batch).item()) for a in agents]
        r = ref.bc_update(obs, actions)
        print("\n  update %d (B=%d): loss %.6f / %.6f vs %.6f, gradient norm %.6f vs %.6f"
              % (u, B, losses[0], losses[1], r["loss"], float(agents[0].networks["main"].norm.item()), r["norm"]))
        assert losses[0] == losses[1]                                        # graphs on and off: the same bits
        np.testing.assert_allclose(losses[0], r["loss"], **LOSS)
        np.testing.assert_allclose(float(agents[0].networks["main"].norm.item()), r["norm"], **LOSS)
    assert torch.equal(agents[0].networks["main"].params.weights, agents[1].networks["main"].params.weights)
    assert not agents[0].networks["main"].accumulated.any()                  # a non-accumulating update
    w = agents[0].networks["main"].params.named_arrays()
    for i, name in enumerate(ref.names):
        for kind, arr in (("kernel", ref.W[i]), ("bias", ref.b[i])):
            np.testing.assert_allclose(w[name + "/" + kind][0], arr, err_msg=name, **WEIGHTS)
    for a in agents:
        a.check_status()
    with pytest.raises(NotImplementedError, match="ImitationAgent is an abstract agent. Not to be used directly."):
        from coach_amd.agents.imitation_agent import ImitationAgent
        ImitationAgent.learn_from_batch(agents[0], batch)


def test_bc_acting_is_egreedy_over_the_probabilities_in_the_forced_test_phase(dev):
    from coach_amd.core_types import RunPhase
    agent = _bc_agent(dev, True)
    agent.ap.exploration.evaluation_epsilon = agent.exploration_policy.evaluation_epsilon = 0.0
    steps_before = agent.exploration_policy.epsilon_schedule.current_value
    states = agent.memory.current_states()
    a = agent.choose_action(states).cpu().numpy().copy()
    assert agent.phase == RunPhase.TRAIN and agent.exploration_policy.phase == RunPhase.TEST
    assert agent.exploration_policy.epsilon_schedule.current_value == steps_before      # the schedule is not stepped
    probs = agent._q_act.cpu().numpy()
    z = agent.networks["main"].policy_values(states, 1, tag="act").data.view(1, 2).cpu().numpy()
    assert np.array_equal(bits(probs), bits(R.softmax_parts(z)[0])) and a[0] == int(np.argmax(probs[0]))
    agent.check_status()


RULE = np.array([0.05, 0.1, 1.0, 0.5])              # action 1 (push right) iff RULE . (x, x_dot, theta, theta_dot) > 0


def _cartpole_rollouts(seed, episodes, max_len=60):
    """CartPole-v0's dynamics on the host (gym's cartpole.py: Euler, force 10, tau 0.02) under the linear rule above, from
    initial states uniform in [-0.15, 0.15]^4 -> write_csv_dataset's episode dicts"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(episodes):
        s = rng.uniform(-0.15, 0.15, size=4)
        obs, nxt, act = [], [], []
        for _ in range(max_len):
            a = int(RULE @ s > 0)
            x, xd, th, thd = s
            force = 10.0 if a else -10.0
            temp = (force + 0.05 * thd * thd * np.sin(th)) / 1.1
            tha = (9.8 * np.sin(th) - np.cos(th) * temp) / (0.5 * (4.0 / 3.0 - 0.1 * np.cos(th) ** 2 / 1.1))
            xa = temp - 0.05 * tha * np.cos(th) / 1.1
            n = np.array([x + 0.02 * xd, xd + 0.02 * xa, th + 0.02 * thd, thd + 0.02 * tha])
            obs.append(s.astype(np.float32)), nxt.append(n.astype(np.float32)), act.append(a)
            s = n
            if abs(s[0]) > 2.4 or abs(s[2]) > 0.2095:
                break
        out.append(dict(obs=np.array(obs), next_obs=np.array(nxt), action=np.array(act),
                        reward=np.ones(len(act), dtype=np.float32), probabilities=None))
    return out


def test_bc_run_on_cartpole_from_a_csv_dataset(dev, tmp_path):
    """BC from rollouts labelled by RULE: the last period's mean loss is below the first's, and on held-out rows the
    greedy action agrees with the rule more often than the majority class does.  The agreement and the evaluation reward
    are printed (DESIGN §8 records them), not asserted against a number."""
    import torch
    from coach_amd.core_types import EnvironmentEpisodes, TrainingSteps
    from coach_amd.memories.episodic.csv_dataset import write_csv_dataset
    from coach_amd.presets.CartPole_BC import make
    path = str(tmp_path / "rule.csv")
    train = _cartpole_rollouts(1, 10)
    write_csv_dataset(path, train, None)
    gm = make(path, improve_steps=300, steps_between_evaluation_periods=100, evaluation_episodes=2, learning_rate=1e-3)
    gm.device = dev
    gm.create_graph()
    agent = gm.agent
    n = sum(len(e["action"]) for e in train)
    assert agent.memory.num_transitions() == n and agent.memory.frozen
    losses, inner = [], agent.learn_from_batch

    def recording(batch):
        loss = inner(batch)
        losses.append(loss.clone())
        return loss
    agent.learn_from_batch = recording
    env_steps = gm.environment.total_steps
    gm.train_and_act(TrainingSteps(100))
    assert gm.environment.total_steps == env_steps                           # the training phase never steps the environment
    gm.improve()
    assert agent.training_iteration == 400 == gm.training_steps and len(losses) == 400
    per = [float(torch.stack(losses[i:i + 100]).mean().item()) for i in range(0, 400, 100)]
    assert per[-1] < per[0]
    held = _cartpole_rollouts(2, 8)
    obs = np.concatenate([e["obs"] for e in held])[:512]
    want = (obs.astype(np.float64) @ RULE > 0).astype(np.int64)
    greedy = np.argmax(agent._predict(_t(obs, dev), len(obs)).cpu().numpy(), axis=1)
    agreement, majority = float((greedy == want).mean()), float(max(want.mean(), 1 - want.mean()))
    evals = [float(r["Evaluation Reward"]) for r in gm.logger.rows if r.get("Evaluation Reward", "") != ""]
    print("\n  BC on %d logged transitions, 400 updates of 32: mean loss per 100 updates %s; held-out agreement %.4f "
          "(majority class %.4f, %d rows); evaluation rewards %s" % (n, np.round(per, 4).tolist(), agreement, majority,
                                                                     len(obs), evals))
    assert agreement > majority and len(evals) == 3
    with pytest.raises(ValueError, match="TrainingSteps"):
        gm.train_and_act(EnvironmentEpisodes(1))
    gm.check_status()


def test_classification_architecture_takes_the_one_hot_target_matrix(dev):
    """the backend interface: predict -> probabilities, train_on_batch / accumulate_gradients on the dense [B, A] targets
    the reference passes, equal to the network driven directly"""
    import torch
    from coach_amd.architectures.hip_architecture import ClassificationArchitecture, HipArchitecture, PolicyGradientArchitecture
    from coach_amd.agents.bc_agent import BCAgentParameters
    from coach_amd.nn.networks import ClassificationNet, classification_net_kwargs
    from coach_amd.presets.CartPole_DDQN_BCQ_BatchRL import make
    from coach_amd.spaces import DiscreteActionSpace, ObservationSpace, SpacesDefinition, StateSpace
    spaces = SpacesDefinition(StateSpace({"observation": ObservationSpace(4)}), None, DiscreteActionSpace(2))
    ap = make(action_drop="nn").agent_params
    ap.seed = 5
    w = ap.network_wrappers["imitation_model"]
    w.input_embedders_parameters['observation'].scheme, w.middleware_parameters.scheme = w.input_embedders_parameters[
        'observation'].scheme[-1:], w.middleware_parameters.scheme[-1:]         # Dense(256), Dense(64): a quick network
    arch = HipArchitecture.construct("imitation_model/online", [dev], ap, spaces, "imitation_model/online")
    assert isinstance(arch, ClassificationArchitecture)
    twin = ClassificationNet(dev, (4,), 2, **classification_net_kwargs(w, 5))
    assert torch.equal(twin.params.weights, arch.net.params.weights)
    rng = np.random.RandomState(1)
    obs, actions = rng.randn(9, 4).astype(np.float32), rng.randint(0, 2, size=9)
    probs = arch.predict({"observation": obs})
    assert probs.shape == (9, 2) and np.array_equal(bits(probs), bits(twin.predict(_t(obs, dev), 9).cpu().numpy()))
    total, losses, norm, fetched = arch.train_on_batch({"observation": obs}, R.one_hot(actions, 2))
    want = twin.train_on_batch(_t(obs, dev), 9, actions=_t(actions.astype(np.int32), dev))
    assert total == float(want.item()) == losses[0] and norm == float(twin.norm.item()) and fetched == []
    assert torch.equal(twin.params.weights, arch.net.params.weights)
    with pytest.raises(ValueError, match="targets shape"):
        arch.accumulate_gradients({"observation": obs}, np.zeros((9, 3)))
    bc = HipArchitecture.construct("main/online", [dev], BCAgentParameters(), spaces, "main/online")
    assert isinstance(bc, PolicyGradientArchitecture) and bc.net.beta_entropy == 0
