"""ParameterNoise on the DQN-family agents, on the MI355X: noisy networks are built, every tensor of a noisy layer
trains and reaches the target copy, acting is np.argmax of the device's own action values with no host draw, and a
checkpoint carries the noise counters so that a restored agent continues bit-identically."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
KINDS = ["dqn", "ddqn", "qr", "c51", "c51_per", "dqn_image_per", "dqn_dueling", "dqn_dueling_image_per"]


def _agent(dev, kind, seed=5, use_graphs=None, noisy=True):
    from coach_amd.core_types import EnvironmentSteps
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    from coach_amd.exploration_policies.parameter_noise import ParameterNoiseParameters
    from coach_amd.memories.memory import MemoryGranularity
    from coach_amd.memories.non_episodic.prioritized_experience_replay import PrioritizedExperienceReplayParameters
    if kind.startswith("dqn"):
        from coach_amd.agents.dqn_agent import DQNAgent as A, DQNAgentParameters as P
    elif kind == "ddqn":
        from coach_amd.agents.ddqn_agent import DDQNAgent as A, DDQNAgentParameters as P
    elif kind == "qr":
        from coach_amd.agents.qr_dqn_agent import QuantileRegressionDQNAgent as A, \
            QuantileRegressionDQNAgentParameters as P
    else:
        from coach_amd.agents.categorical_dqn_agent import CategoricalDQNAgent as A, CategoricalDQNAgentParameters as P
    p = P()
    p.seed = seed
    if "dueling" in kind:
        from coach_amd.architectures.head_parameters import DuelingQHeadParameters
        p.network_wrappers["main"].heads_parameters = [DuelingQHeadParameters()]
    if kind in ("qr", "c51", "c51_per"):
        p.algorithm.atoms = 11
    if kind.startswith("c51"):
        p.algorithm.v_min, p.algorithm.v_max = -2.0, 8.0
    p.network_wrappers["main"].batch_size = 16
    if kind.endswith("_per"):
        p.memory = PrioritizedExperienceReplayParameters()
    p.memory.max_size = (MemoryGranularity.Transitions, 64)
    p.algorithm.num_consecutive_playing_steps = EnvironmentSteps(1)
    p.algorithm.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(7)
    if noisy:
        p.exploration = ParameterNoiseParameters(p)
    if "image" in kind:
        envp = SyntheticVectorEnvironmentParameters("image", 1, (84, 84), 3, episode_length=5, seed=3)
    else:
        envp = SyntheticVectorEnvironmentParameters("vector", 1, (6,), 3, episode_length=5, seed=3)
    return A(p, SyntheticVectorEnvironment(envp, dev), dev, use_graphs=use_graphs)


def _run(a, heatup=20, steps=12):
    from coach_amd.core_types import RunPhase
    random.seed(9); np.random.seed(9)
    a.phase = RunPhase.HEATUP
    for _ in range(heatup):
        a.act()
    a.phase = RunPhase.TRAIN
    for _ in range(steps):
        a.step_and_train()
    a.check_status()


@pytest.mark.parametrize("kind", KINDS)
def test_noisy_agent_trains_all_four_tensors_and_copies_them_to_the_target(dev, kind):
    import torch
    from coach_amd.nn import graph as G
    a = _agent(dev, kind)
    net = a.networks["main"]
    assert net.noisy and net._fused is None and net._act is None and not a._step_graph_ok()
    dense = [l for m in net.modules for l in (m.layers if isinstance(m, G.Sequential) else [m])
             if not isinstance(l, G.Conv2d)]
    assert dense and all(isinstance(l, G.NoisyDense) for l in dense) and len(net.noisy_layers) == len(dense)
    assert not any(n.endswith("/kernel") and "conv" not in n for n in net.params.entries)
    before = net.params.named_arrays()
    _run(a)
    after, target = net.params.named_arrays(), net.params.named_arrays(net.target)
    assert np.isfinite(float(net.loss.item()))
    for l in net.noisy_layers:
        for name in (l.wmname, l.bmname, l.wsname, l.bsname):
            assert not np.array_equal(before[name][0], after[name][0]), name          # it moved (the stddevs too)
            assert np.isfinite(after[name][0]).all(), name
    # the target copy carries all four tensors of every noisy layer
    a.update_target_networks(1.0)
    target = net.params.named_arrays(net.target)
    after = net.params.named_arrays()
    for l in net.noisy_layers:
        for name in (l.wmname, l.bmname, l.wsname, l.bsname):
            assert np.array_equal(target[name][0], after[name][0]), name
    # every pass counted on its own: acting, online, target (and Double DQN's selection pass)
    c = net.noise_counters.cpu().numpy().reshape(-1, 4)
    assert (c == c[0]).all() and c[0][0] > 0 and c[0][1] == a.training_iteration == c[0][2]
    assert c[0][3] == (a.training_iteration if kind == "ddqn" else 0)


@pytest.mark.parametrize("kind", ["dqn", "qr", "c51"])
def test_actions_are_the_first_argmax_and_consume_no_host_draw(dev, kind):
    import torch
    from coach_amd.core_types import RunPhase
    a = _agent(dev, kind, use_graphs=False)
    _run(a, steps=3)
    a.phase = RunPhase.TRAIN
    state, pystate = np.random.get_state(), random.getstate()
    for _ in range(6):
        a.act()
        q = a._q_act.cpu().numpy()
        assert np.array_equal(a.actions.cpu().numpy(), np.argmax(q, axis=1).astype(np.int32))
    after = np.random.get_state()
    # k acting steps with no exploration draw at all leave both host generators where they were: act() itself draws nothing
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert random.getstate() == pystate


def test_epsilon_greedy_acting_does_consume_host_draws(dev):
    """the control for the test above: the same steps under the default policy move np.random"""
    from coach_amd.core_types import RunPhase
    a = _agent(dev, "dqn", use_graphs=False, noisy=False)
    _run(a, steps=3)
    a.phase = RunPhase.TRAIN
    state = np.random.get_state()
    a.act()
    after = np.random.get_state()
    assert not (np.array_equal(state[1], after[1]) and state[2:] == after[2:])


def test_constructed_ties_take_the_first_maximum(dev, rlx):
    import torch
    from coach_amd import _rlx
    s = _rlx.current_stream()
    q = torch.tensor([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0], [0.0, -1.0, 0.0], [-5.0, -4.0, -4.0]], dtype=torch.float32,
                     device=dev)
    out = torch.full((4,), -1, dtype=torch.int32, device=dev)
    rlx.argmax_rows(q, 3, 4, 3, out, s)
    assert out.cpu().tolist() == np.argmax(q.cpu().numpy(), axis=1).tolist() == [1, 0, 0, 1]
    # quantiles [env][A = 3][N = 2]: actions 1 and 2 tie exactly in their fp64 means
    quant = torch.tensor([[0.0, 1.0, 2.0, 4.0, 3.0, 3.0], [5.0, 5.0, 1.0, 1.0, 4.0, 6.0]], dtype=torch.float32, device=dev)
    qv = torch.zeros(2, 3, dtype=torch.float64, device=dev)
    act = torch.full((2,), -1, dtype=torch.int32, device=dev)
    rlx.quantile_argmax(quant, 6, 2, 2, 3, qv, act, s)
    assert qv.cpu().tolist() == [[0.5, 3.0, 3.0], [5.0, 1.0, 5.0]]
    assert act.cpu().tolist() == np.argmax(qv.cpu().numpy(), axis=1).tolist() == [1, 0]
    # equal logits in two actions: identical softmaxes, identical expectations
    z = torch.linspace(-1.0, 1.0, 3, dtype=torch.float64, device=dev)
    logits = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 2.0]], dtype=torch.float32, device=dev)
    qv = torch.zeros(1, 3, dtype=torch.float64, device=dev)
    act = torch.full((1,), -1, dtype=torch.int32, device=dev)
    rlx.categorical_argmax(logits, 9, z, 3, 1, 3, qv, act, s)
    v = qv.cpu().numpy()
    assert v[0, 1] == v[0, 2] > v[0, 0]
    assert act.cpu().tolist() == np.argmax(v, axis=1).tolist() == [1]


@pytest.mark.parametrize("kind", ["dqn", "c51_per"])
def test_checkpoint_round_trip_continues_bit_identically(dev, kind, tmp_path):
    import torch
    from coach_amd.checkpoint import restore_checkpoint, save_checkpoint
    a = _agent(dev, kind)
    _run(a)
    save_checkpoint(a, str(tmp_path))
    b = _agent(dev, kind)
    restore_checkpoint(b, str(tmp_path))      # (also puts the host generators, reseeded by b's constructor, back)
    assert torch.equal(a.networks["main"].noise_counters, b.networks["main"].noise_counters)
    outs = []
    for agent in (a, b):
        agent.act()
        q = agent._q_act.clone()
        agent.train()
        outs.append((q, agent.networks["main"].loss.clone(), agent.networks["main"].params.weights.clone()))
        if agent is a:
            restore_checkpoint(b, str(tmp_path))             # (the host generators go back to the checkpoint's state)
    (qa, la, wa), (qb, lb, wb) = outs
    assert torch.equal(qa, qb) and torch.equal(la, lb) and torch.equal(wa, wb)


def test_default_agents_keep_their_plain_networks(dev):
    from coach_amd.nn import graph as G
    a = _agent(dev, "dqn", noisy=False)
    net = a.networks["main"]
    assert not net.noisy and net.noise_counters is None and not net.noisy_layers
    assert sorted(net.params.entries) == sorted(
        ["main/embedder/dense0/kernel", "main/embedder/dense0/bias", "main/middleware/dense0/kernel",
         "main/middleware/dense0/bias", "main/q_head/dense/kernel", "main/q_head/dense/bias"])
    assert net._fused is not None and net._act is not None


def test_default_networks_equal_the_recorded_parameter_lists(dev):
    """names, offsets in the flat buffer, shapes, towers, tower strides and buffer sizes of the networks the default
    (epsilon-greedy) agents build, against tests/golden/default_param_lists.json — written by
    tests/golden/make_default_param_lists.py from the commit before the noisy layers existed"""
    import importlib.util
    import json
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_default_param_lists",
                                                  os.path.join(here, "golden", "make_default_param_lists.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(here, "golden", "default_param_lists.json")) as f:
        recorded = json.load(f)
    built = mod.describe(dev)
    assert set(built) == set(recorded) and len(recorded) == 7
    for case in recorded:
        assert built[case] == recorded[case], case


def test_restored_agent_takes_the_checkpoints_noise_key(dev, tmp_path):
    """the key of the noisy layers' generator is the SAVED one after a restore, in the agent and in its network — a
    fresh agent built with another seed (or with none: a random key) continues the saved agent's noise sequence"""
    import torch
    from coach_amd.checkpoint import restore_checkpoint, save_checkpoint
    a = _agent(dev, "dqn", seed=5)
    _run(a)
    save_checkpoint(a, str(tmp_path))
    for other in (77, None):
        b = _agent(dev, "dqn", seed=other)
        assert b.networks["main"].noise_seed != a.networks["main"].noise_seed
        restore_checkpoint(b, str(tmp_path))
        net_a, net_b = a.networks["main"], b.networks["main"]
        assert (b._noise_seed, net_b.noise_seed, net_b.noise_rank) == (a._noise_seed, net_a.noise_seed, net_a.noise_rank)
        states = a.memory.current_states()
        saved = net_b.noise_counters.clone()                     # (what the checkpoint holds)
        net_a.noise_counters.copy_(saved)                        # (an earlier probe advanced a's acting counters)
        qa = net_a.q_values(states, a.n_env, tag="probe").data.clone()
        qb = net_b.q_values(states, b.n_env, tag="probe").data.clone()
        assert torch.equal(qa, qb)


RESTATED = ["dqn", "ddqn", "dqn_per", "dqn_image_per", "dqn_dueling", "dqn_dueling_image_per", "qr", "c51", "c51_per"]


@pytest.mark.parametrize("kind", RESTATED)
def test_update_equals_the_host_restatement(dev, kind):
    """three learn_from_batch updates of the agent's noisy network against tests/noisy_agent_ref.py (twin layers fed the
    device's noise, the oracle's convolutions and DQN targets, c51_ref / qr_dqn_ref, TF1 Adam): the first update's loss
    within LOSS, every parameter after the three Adam steps within WEIGHTS — all four tensors of every noisy layer."""
    import torch
    from noisy_agent_ref import NoisyUpdateRef
    from tolerances import LOSS, WEIGHTS
    a = _agent(dev, "ddqn" if kind == "ddqn" else kind, use_graphs=False)
    net = a.networks["main"]
    family = "qr" if kind == "qr" else "c51" if kind.startswith("c51") else "dqn"
    ref = NoisyUpdateRef(net, family, (a._noise_seed, a._noise_rank), double_dqn=kind == "ddqn",
                         kappa=getattr(net, "kappa", 1.0), z=getattr(net, "z_values", None))
    start = {k: v.copy() for k, v in ref.online.items()}
    rng = np.random.RandomState(17)
    B, A, discount = a.batch_size, a.A, 0.9
    per = kind.endswith("_per")
    errors = torch.zeros(B, dtype=torch.float64, device=dev)
    for step in range(3):
        if net.image:
            obs, nxt = (rng.randint(0, 256, size=(B,) + net.obs_shape).astype(np.uint8) for _ in range(2))
        else:
            obs, nxt = (rng.randn(B, net.obs_shape[0]).astype(np.float32) for _ in range(2))
        actions = rng.randint(0, A, size=B).astype(np.int32)
        rewards = rng.randn(B).astype(np.float32)
        overs = (rng.rand(B) < 0.25).astype(np.uint8)
        w = rng.uniform(0.2, 1.0, size=B) if per and family == "dqn" else None
        d = lambda x: torch.from_numpy(x).to(dev)
        if family == "dqn":
            loss = net.learn_from_batch(d(obs), d(nxt), B, d(actions), d(rewards), d(overs), discount,
                                        importance_weights=None if w is None else d(w), td_errors=errors,
                                        double_dqn=kind == "ddqn")
        else:
            kw = {"per_errors": errors} if family == "c51" else {}
            loss = net.learn_from_batch(d(obs), d(nxt), B, d(actions), d(rewards), d(overs), discount, **kw)
        net.check_status()
        ref_loss = ref.update(obs, nxt, actions, rewards, overs.astype(bool), discount, w)
        print("%s update %d: loss %.7g, restated %.7g" % (kind, step, float(loss.item()), ref_loss))
        if step == 0:
            np.testing.assert_allclose(float(loss.item()), ref_loss, **LOSS)
            if kind == "dqn":
                a.update_target_networks(1.0)                     # the later updates see a target that differs ...
                ref.target = {k: v.copy() for k, v in ref.online.items()}      # ... from the initial copy
    got = net.params.named_arrays()
    assert set(got) == set(ref.online)
    for l in net.noisy_layers:
        for name in (l.wmname, l.bmname, l.wsname, l.bsname):
            assert not np.array_equal(start[name], got[name][0]), name
    for name, arr in ref.online.items():
        err = np.abs(got[name][0].astype(np.float64) - arr)
        bound = WEIGHTS["atol"] + WEIGHTS["rtol"] * np.abs(arr)
        print("  %-50s worst |error| %.3e, worst error / bound %.3f" % (name, err.max(), (err / bound).max()))
    for name, arr in ref.online.items():
        np.testing.assert_allclose(got[name][0], arr, err_msg=name, **WEIGHTS)
