"""The layers over csrc/dnd.hip: one NECNet update against an fp64 restatement with torch autograd for the trunk, the
bootstrapped n-step returns against a numpy copy of Episode.update_discounted_rewards (core_types.py:780-798), the
CartPole_NEC preset (the reference's text through the import layer; a short run on the device) and the refusals by name."""
import numpy as np
import pytest

from test_dnd import dist2, nearest
from tolerances import LOSS, WEIGHTS


def _net(dev, **kw):
    from coach_amd.nn.networks import NECNet
    args = dict(dnd_size=256, number_of_knn=8, embedder=[32], middleware=[64], seed=3)
    args.update(kw)
    return NECNet(dev, (4,), 2, **args)


@pytest.mark.gpu
def test_necnet_update_equals_fp64_autograd(dev):
    import torch
    rng = np.random.RandomState(0)
    net, B, k, A = _net(dev), 16, 8, 2
    stored = torch.from_numpy(rng.randn(200, 4).astype(np.float32)).to(dev)  # the tables: embeddings of 200 states
    acts = torch.from_numpy((np.arange(200) % A).astype(np.int32)).to(dev)
    net.dnd.add(net.state_embedding(stored, 200, tag="fill").clone(), acts,
                torch.from_numpy(rng.randn(200).astype(np.float32)).to(dev))
    assert net.dnd.has_enough_entries()
    obs = rng.randn(B, 4).astype(np.float32)
    actions, targets = rng.randint(0, A, size=B).astype(np.int32), rng.randn(B).astype(np.float32)
    keys, values = net.dnd.keys.cpu().numpy(), net.dnd.values.cpu().numpy()
    names = list(net.params.entries)
    before = {n: a[0] for n, a in net.params.named_arrays().items()}

    w = {n: torch.from_numpy(before[n]).double().requires_grad_(True) for n in names}
    x = torch.from_numpy(obs).double()
    for layer in ("main/embedder/dense0", "main/middleware/dense0"):
        x = torch.relu(x @ w[layer + "/kernel"] + w[layer + "/bias"])
    e32 = x.detach().numpy().astype(np.float32)
    q = []
    for b in range(B):                       # the neighbours of the fp32 embedding, then the head in fp64
        a = int(actions[b])
        j = (nearest(dist2(e32[b:b + 1], keys[a, :100]), k)[0] & np.uint64(0xffffffff)).astype(np.int64)
        d = ((torch.from_numpy(keys[a, j]).double() - x[b]) ** 2).sum(1) + float(np.float32(0.001))
        q.append((torch.from_numpy(values[a, j]).double() / d).sum() / (1.0 / d).sum())
    loss = ((torch.stack(q) - torch.from_numpy(targets).double()) ** 2).sum() / B
    loss.backward()

    dobs = torch.from_numpy(obs).to(dev)
    dact, dtar = torch.from_numpy(actions).to(dev), torch.from_numpy(targets).to(dev)
    got = net.accumulate_gradients(dobs, B, dact, dtar)
    np.testing.assert_allclose(got.item(), loss.item(), **LOSS)
    norm = np.sqrt(sum((w[n].grad ** 2).sum().item() for n in names))
    np.testing.assert_allclose(net.norm.item(), norm, **LOSS)
    for n in names:
        np.testing.assert_allclose(net.params.g(n).cpu().numpy(), w[n].grad.numpy(), err_msg=n, **WEIGHTS)
    net.learn_from_batch(dobs, B, dact, dtar)                                 # and Adam moves every tensor
    assert all((net.params.w(n).cpu().numpy() != before[n]).any() for n in names)


@pytest.mark.gpu
@pytest.mark.parametrize("n_step", [1, 3, 40])
def test_bootstrapped_nstep_returns(rlx, dev, n_step):
    import torch
    rng = np.random.RandomState(n_step)
    T, n_env, env, ring, first, discount = 23, 3, 1, 32, 20, 0.99             # the episode wraps around the ring
    rewards, mav = rng.randn(ring * n_env).astype(np.float32), rng.randn(ring * n_env).astype(np.float32)
    rows = ((first + np.arange(T)) % ring) * n_env + env
    out = torch.full((ring * n_env,), -7.0, dtype=torch.float64, device=dev)
    compact = torch.zeros(T, dtype=torch.float64, device=dev)
    rlx.episode_nstep_returns_bootstrapped(torch.from_numpy(rewards).to(dev), torch.from_numpy(mav).to(dev), out, compact,
                                           first, T, env, n_env, ring, discount, n_step, 0)
    r, n = rewards[rows].astype("float"), min(n_step, T)                      # core_types.py:780-798
    want, current_discount = r.copy(), discount
    for i in range(1, n):
        want += current_discount * np.pad(r[i:], (0, i), "constant", constant_values=0)
        current_discount *= discount
    want = want + current_discount * np.pad(mav[rows].astype("float")[n:], (0, n), "constant", constant_values=0)
    assert np.array_equal(compact.cpu().numpy(), want)
    got = out.cpu().numpy()
    assert np.array_equal(got[rows], want) and (np.delete(got, rows) == -7.0).all()


def test_parameters_carry_the_references_names_and_defaults():
    """rl_coach/agents/nec_agent.py:36-110, served under the reference's module path by coach_amd.compat"""
    import coach_amd.compat
    coach_amd.compat.install()
    try:
        from rl_coach.agents.nec_agent import NECAgentParameters
        from rl_coach.architectures.head_parameters import DNDQHeadParameters
        from rl_coach.memories.memory import MemoryGranularity
        p = NECAgentParameters()
    finally:
        coach_amd.compat.uninstall()
    alg, net = p.algorithm, p.network_wrappers["main"]
    assert (alg.dnd_size, alg.l2_norm_added_delta, alg.new_value_shift_coefficient, alg.number_of_knn,
            alg.DND_key_error_threshold, alg.propagate_updates_to_DND, alg.n_step,
            alg.bootstrap_total_return_from_old_policy) == (500000, 0.001, 0.1, 50, 0, False, 100, True)
    assert alg.num_consecutive_playing_steps.num_steps == 4 and p.memory.max_size == (MemoryGranularity.Transitions, 100000)
    assert isinstance(net.heads_parameters[0], DNDQHeadParameters) and net.middleware_scheme == "Medium"
    assert p.exploration.evaluation_epsilon == 0.01 and p.exploration.epsilon_schedule.current_value == 0.1
    assert p.path == "coach_amd.agents.nec_agent:NECAgent"


REF = "/root/reference/rl_coach/presets/CartPole_NEC.py"


@pytest.mark.skipif(not __import__("os").path.isfile(REF), reason="needs the reference's preset text (build container)")
def test_the_references_preset_text_executes_through_the_import_layer():
    import coach_amd.compat
    coach_amd.compat.install()
    try:
        ns = {}
        exec(compile(open(REF).read(), REF, "exec"), ns)
    finally:
        coach_amd.compat.uninstall()
    gm, ours = ns["graph_manager"], __import__("importlib").import_module("coach_amd.presets.CartPole_NEC").make()
    from coach_amd.compat import resolve_reference_style
    resolve_reference_style(gm.agent_params, gm.env_params)
    a, b = gm.agent_params, ours.agent_params
    assert a.path == b.path == "coach_amd.agents.nec_agent:NECAgent"
    assert vars(a.algorithm).keys() == vars(b.algorithm).keys()
    for k, v in vars(b.algorithm).items():
        assert getattr(v, "num_steps", v) == getattr(getattr(a.algorithm, k), "num_steps", getattr(a.algorithm, k)), k
    assert a.memory.max_size == b.memory.max_size and a.exploration.evaluation_epsilon == b.exploration.evaluation_epsilon
    assert vars(a.exploration.epsilon_schedule) == vars(b.exploration.epsilon_schedule)
    assert a.network_wrappers["main"].learning_rate == b.network_wrappers["main"].learning_rate
    assert gm.schedule.heatup_steps.num_steps == ours.schedule.heatup_steps.num_steps == 1300


@pytest.mark.gpu
def test_cartpole_nec_preset_fills_the_tables_then_trains(dev):
    """heat-up plus 200 TRAIN steps on 2 envs: every table passes k entries, training starts only then, no status bit"""
    import importlib
    from coach_amd.core_types import EnvironmentSteps, RunPhase
    gm = importlib.import_module("coach_amd.presets.CartPole_NEC").make(num_envs=2, heatup_steps=100, dnd_size=4096)
    gm.schedule.improve_steps = EnvironmentSteps(200)
    gm.schedule.steps_between_evaluation_periods = EnvironmentSteps(100)
    gm.device = dev
    gm.create_graph()
    a = gm.agent
    started = []                             # (tables ready, training had started before) at every update
    learn = a.learn_from_batch
    a.learn_from_batch = lambda batch: (started.append((a.networks["main"].dnd.has_enough_entries(), a.training_started)),
                                        learn(batch))[1]
    rows = gm.improve()
    dnd, mem = a.networks["main"].dnd, a.memory
    assert gm.total_steps_counters[RunPhase.TRAIN] == 200 and a.training_started and started
    assert all(ready or not before for ready, before in started)             # never trained on a table of <= k entries
    assert (dnd.size.cpu().numpy() > dnd.k).all() and a.training_iteration > 0
    assert int(dnd.size.sum().item()) <= mem._gstep * 2 and mem.embedding.abs().sum().item() > 0
    assert mem.max_action_value.abs().sum().item() > 0                        # acting steps after heat-up carried max_a Q
    gm.environment.check_status()
    a.check_status()
    print("CartPole_NEC, 2 envs, 100 heat-up + 200 TRAIN steps: evaluation rewards",
          [r["Evaluation Reward"] for r in rows if r.get("Evaluation Reward", "") != ""])


@pytest.mark.gpu
def test_necagent_refuses_by_name(dev):
    from coach_amd.agents.nec_agent import NECAgent, NECAgentParameters
    from coach_amd.environments.synthetic_vector_environment import (SyntheticVectorEnvironment,
                                                                     SyntheticVectorEnvironmentParameters)
    image = SyntheticVectorEnvironment(SyntheticVectorEnvironmentParameters("image", 1, (84, 84), 2, episode_length=8), dev)
    with pytest.raises(NotImplementedError, match="image observations"):
        NECAgent(NECAgentParameters(), image, dev)
    vector = SyntheticVectorEnvironment(SyntheticVectorEnvironmentParameters("vector", 1, (4,), 2, episode_length=8), dev)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        NECAgent(NECAgentParameters(), vector, dev, dist=__import__("types").SimpleNamespace(enabled=True))


def test_the_backend_interface_refuses_the_dictionary_head_by_name():
    from coach_amd.agents.nec_agent import NECNetworkParameters
    from coach_amd.architectures.hip_architecture import _family_of
    with pytest.raises(NotImplementedError, match="backend interface does not serve a DNDQHead"):
        _family_of(NECNetworkParameters())


@pytest.mark.gpu
def test_necnet_from_the_parameter_objects(dev):
    """the defaults give the 512-float key of FCMiddlewareParameters; the acting pass gives zeros while the tables are empty"""
    import torch
    from coach_amd.agents.nec_agent import NECAgentParameters
    from coach_amd.nn.networks import NECNet, nec_net_kwargs
    p = NECAgentParameters()
    p.algorithm.dnd_size = 64
    net = NECNet(dev, (4,), 2, **nec_net_kwargs(p.network_wrappers["main"], p.algorithm, seed=1))
    q, e = net.q_values(torch.zeros(3, 4, device=dev), 3)
    assert tuple(e.shape) == (3, 512) and tuple(q.shape) == (3, 2) and (q == 0).all() and not net.dnd.has_enough_entries()


def test_necnet_refuses_by_name():
    from coach_amd.nn.networks import NECNet
    with pytest.raises(NotImplementedError, match="image observations"):
        NECNet("cpu", (84, 84, 4), 2)


@pytest.mark.gpu
def test_necnet_refuses_data_parallel_and_dnd_updates_by_name(dev):
    with pytest.raises(NotImplementedError, match="data-parallel"):
        _net(dev).learn_from_batch(None, 1, None, None, sync=object())
    with pytest.raises(NotImplementedError, match="propagate_updates_to_DND"):
        _net(dev, propagate_updates_to_DND=True)
