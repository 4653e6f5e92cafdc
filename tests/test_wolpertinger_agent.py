"""The Wolpertinger agent, its output filter and its preset: parameter plumbing on the CPU; acting, the update and a
short BasicRLGraphManager run on the GPU (the synthetic InvertedPendulum-v2 spaces, 4 envs, 33 bins, k = 3)."""
import csv
import importlib
import json
import os
import random
from collections import OrderedDict

import numpy as np
import pytest

import wolpertinger_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRESET = "Mujoco_Wolpertinger"


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("low, high, bins", [([-1.0], [1.0], 5), ([-2.0], [3.0], 64), ([0.0, -1.0], [10.0, 1.0], [5, 3]),
                                             ([-3.0], [3.0], 1000)])
def test_box_discretization_tables_against_numpy(low, high, bins):
    from itertools import product
    from coach_amd.filters.action import BoxDiscretization
    low, high = np.array(low, dtype=np.float32), np.array(high, dtype=np.float32)
    f = BoxDiscretization(bins)
    n = f.get_unfiltered_action_space(low, high)
    per_dim = [bins] * len(low) if isinstance(bins, int) else bins
    want = np.array(list(product(*[np.linspace(low[i], high[i], per_dim[i]) for i in range(len(low))])))
    assert n == int(np.prod(per_dim)) and f.target_actions.shape == (n, len(low))
    assert f.target_actions.dtype == want.dtype and f.target_actions.tobytes() == want.tobytes()
    assert f.target_actions.tobytes() == R.target_actions(low, high, bins).tobytes()
    assert np.array_equal(f.filter(n - 1), want[-1])
    with pytest.raises(ValueError, match="does not match the action space"):
        f.filter(n)


def test_box_discretization_integer_bins_and_bin_lists():
    from coach_amd.filters.action import BoxDiscretization
    f = BoxDiscretization(5, force_int_bins=True)
    assert f.get_unfiltered_action_space(np.array([0.0]), np.array([10.0])) == 5
    assert f.target_actions[:, 0].tolist() == [0, 2, 5, 7, 10]            # box_discretization.py's own example
    with pytest.raises(ValueError, match="does not match the number of dimensions"):
        BoxDiscretization([3, 4]).get_unfiltered_action_space(np.array([0.0]), np.array([1.0]))


def test_output_filter_accepts_one_box_discretization_and_nothing_else():
    from coach_amd.filters import NoOutputFilter, OutputFilter
    from coach_amd.filters.action import BoxDiscretization
    disc = BoxDiscretization(7)
    f = OutputFilter(action_filters=OrderedDict([("discretization", disc)]), is_a_reference_filter=False)
    assert list(f.action_filters.values()) == [disc] and f.i_am_a_reference_filter is False
    assert not NoOutputFilter().action_filters and not OutputFilter().action_filters
    for bad in ({"rescale": object()}, OrderedDict([("a", BoxDiscretization(3)), ("b", BoxDiscretization(3))]),
                OrderedDict([("a", BoxDiscretization(3)), ("rescale", object())])):
        with pytest.raises(ValueError, match="no device implementation"):
            OutputFilter(action_filters=bad)


def _params(bins=33, k=3, width=1, with_filter=True):
    from coach_amd.agents.wolpertinger_agent import WolpertingerAgentParameters
    from coach_amd.filters import OutputFilter
    from coach_amd.filters.action import BoxDiscretization
    ap = WolpertingerAgentParameters()
    ap.algorithm.k, ap.algorithm.action_embedding_width = k, width
    if with_filter:
        ap.output_filter = OutputFilter(action_filters=OrderedDict([("discretization", BoxDiscretization(bins))]))
    return ap


def _env_stub(kind="vector", action_dim=1):
    return _Obj(p=_Obj(kind=kind, num_envs=2, observation_shape=(4,), action_dim=action_dim, action_low=-1.0,
                       action_high=1.0, episode_length=5, num_actions=None))


@pytest.mark.parametrize("params, env, message", [
    (dict(with_filter=False), dict(), "WolpertingerAgent works only for discrete control problems"),
    (dict(), dict(action_dim=None), "WolpertingerAgent works only for discrete control problems"),
    (dict(width=2), dict(), "action_embedding_width = 1 and a one-dimensional box"),
    (dict(), dict(action_dim=2), "action_embedding_width = 1 and a one-dimensional box"),
    (dict(bins=4, k=5), dict(), r"k = 5 outside \[1, min\(number of actions = 4, 64\)\]"),
    (dict(bins=100, k=65), dict(), "k = 65 outside"),
    (dict(bins=1, k=1), dict(), "at least 2 discrete actions"),
    (dict(), dict(kind="image"), "only for vector observations"),
])
def test_agent_refusals_come_before_anything_touches_the_device(params, env, message):
    from coach_amd.agents.wolpertinger_agent import WolpertingerAgent
    with pytest.raises(ValueError, match=message):
        WolpertingerAgent(_params(**params), _env_stub(**env))


def test_keys_are_the_reference_expression():
    from coach_amd.agents.wolpertinger_agent import knn_keys
    scale = np.array([3.0], dtype=np.float32)
    keys = knn_keys(33, scale)
    want = np.expand_dims((np.arange(33) / (33 - 1) - 0.5) * 2, 1) * scale
    assert keys.dtype == np.float64 and keys.shape == (33, 1) and keys.tobytes() == want.tobytes()
    assert keys.tobytes() == R.knn_keys(33, scale).tobytes() and keys[0, 0] == -3.0 and keys[-1, 0] == 3.0


def test_package_preset_equals_the_unchanged_reference_preset_text():
    """tests/golden/wolpertinger_preset.json holds what the reference's preset text, executed unchanged through the import
    layer, sets (make_wolpertinger_preset_dump.py): the package's preset must equal it field by field."""
    from coach_amd.compat import resolve_reference_style
    from test_cartpole import _dump
    with open(os.path.join(GOLDEN, "wolpertinger_preset.json")) as f:
        ref = json.load(f)[PRESET]
    mine = importlib.import_module("coach_amd.presets." + PRESET).make()
    resolve_reference_style(mine.agent_params, mine.env_params)      # what create_graph does first
    for part in ("agent_params", "env_params", "schedule", "preset_validation_params"):
        assert ref[part] == _dump(getattr(mine, part)), part
    filters = mine.agent_params.output_filter.action_filters
    assert ref["action_filters"] == {name: _dump(f) for name, f in filters.items()}
    assert filters["discretization"].num_bins_per_dimension == 1000000
    assert mine.schedule.heatup_steps.num_steps == 3000 and mine.agent_params.algorithm.k == 1
    small = importlib.import_module("coach_amd.presets." + PRESET).make(level="inverted_pendulum", num_envs=4,
                                                                        agent_seed=3, num_bins=33, k=3)
    assert small.agent_params.output_filter.action_filters["discretization"].num_bins_per_dimension == 33
    assert (small.agent_params.algorithm.k, small.agent_params.seed, small.env_params.num_envs) == (3, 3, 4)


def test_import_layer_serves_the_reference_module_paths():
    import coach_amd.compat as compat
    compat.install()
    import coach_amd.agents.wolpertinger_agent as mine
    import coach_amd.filters.action as action
    mod = importlib.import_module("rl_coach.agents.wolpertinger_agent")
    assert mod.WolpertingerAgentParameters is mine.WolpertingerAgentParameters and mod.WolpertingerAgent is mine.WolpertingerAgent
    assert importlib.import_module("rl_coach.filters.action").BoxDiscretization is action.BoxDiscretization
    assert importlib.import_module("rl_coach.filters.action.box_discretization").BoxDiscretization is action.BoxDiscretization
    heads = importlib.import_module("rl_coach.architectures.head_parameters")
    head = heads.WolpertingerActorHeadParameters()
    assert (head.activation_function, head.batchnorm, head.head_type) == ("tanh", True, "WolpertingerActorHead")
    assert mine.WolpertingerAgentParameters().network_wrappers["actor"].heads_parameters[0].batchnorm is False


@pytest.mark.reference
def test_reference_preset_text_builds_through_compat():
    from test_preset_dropin import _exec_preset
    with open("/root/reference/rl_coach/presets/%s.py" % PRESET) as f:
        gm = _exec_preset(f.read())["graph_manager"]
    from coach_amd.agents.wolpertinger_agent import WolpertingerAgentParameters
    from coach_amd.filters.action import BoxDiscretization
    assert isinstance(gm.agent_params, WolpertingerAgentParameters)
    disc = gm.agent_params.output_filter.action_filters["discretization"]
    assert isinstance(disc, BoxDiscretization) and disc.num_bins_per_dimension == 1000000
    critic = gm.agent_params.network_wrappers["critic"]
    assert critic.observation_embedder_scheme == (400,) and critic.action_embedder_scheme == ()
    v = gm.preset_validation_params
    assert v.test and v.min_reward_threshold == 500 and v.max_episodes_to_achieve_reward == 1000


# ------------------------------------------------------------------------------------------------------- GPU
BINS, K, N_ENV = 33, 3, 4


def _graph_manager(seed=5, episode_length=5, batch=None):
    gm = importlib.import_module("coach_amd.presets." + PRESET).make(level="inverted_pendulum", num_envs=N_ENV,
                                                                     agent_seed=seed, num_bins=BINS, k=K)
    gm.env_params.episode_length = episode_length
    if batch is not None:
        for w in gm.agent_params.network_wrappers.values():
            w.batch_size = batch
    return gm


def _agent(dev, **kw):
    gm = _graph_manager(**kw)
    gm.device = dev
    gm.visualization_parameters.dump_csv = False
    return gm.create_graph().agent


def _tables(agent):
    ep = agent.env.p
    low = np.broadcast_to(np.asarray(ep.action_low, dtype=np.float32), (1,))
    high = np.broadcast_to(np.asarray(ep.action_high, dtype=np.float32), (1,))
    keys = R.knn_keys(BINS, np.maximum(np.abs(low), np.abs(high))).astype(np.float32)
    table = R.target_actions(low, high, BINS).astype(np.float32)
    assert np.array_equal(agent.d_keys.cpu().numpy(), keys) and np.array_equal(agent.d_target_actions.cpu().numpy(), table)
    return keys, table


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.gpu
def test_acting_follows_the_reference_step_by_step(dev):
    import torch
    from coach_amd.core_types import RunPhase
    a = _agent(dev)
    keys, table = _tables(a)
    pol = a.exploration_policy
    assert a.memory.action.dtype == torch.int32 and a.actions.dtype == torch.int32 and a.n_actions == BINS and a.k == K
    chosen = []

    def step(phase):
        a.phase = phase
        s0 = a.memory.current_states().clone()
        state = np.random.get_state()
        a.act()
        torch.cuda.synchronize()
        chosen.append(a.actions.cpu().numpy().copy())
        return s0.cpu().numpy().reshape(N_ENV, -1), state

    def drawn(state):
        rs = np.random.RandomState()
        rs.set_state(state)
        return rs

    # heat-up: DiscreteActionSpace.sample per env on the host stream, where the DQN agents draw it
    for _ in range(3):
        s0, state = step(RunPhase.HEATUP)
        rs = drawn(state)
        want = np.array([rs.choice(BINS) for _ in range(N_ENV)], dtype=np.int32)
        assert np.array_equal(a.actions.cpu().numpy(), want)
        assert np.array_equal(bits(a.env_actions.cpu().numpy()), bits(table[want]))
        assert np.array_equal(np.random.get_state()[1], rs.get_state()[1]) and np.random.get_state()[2] == rs.get_state()[2]

    std = float(np.float32(pol.noise_schedule.current_value))
    for t in range(20):                       # the first eager, the second captured, then replays
        schedule_before = pol.noise_schedule.current_value
        s0, state = step(RunPhase.TRAIN)
        rs = drawn(state)
        z = rs.standard_normal((N_ENV, 1))                                    # AdditiveNoise's draws, nothing else
        assert np.array_equal(np.random.get_state()[1], rs.get_state()[1]) and np.random.get_state()[2] == rs.get_state()[2]
        mu = a._mu_act.cpu().numpy().astype(np.float64)
        proto = a.proto.cpu().numpy()
        assert np.array_equal(bits(proto), bits((mu + std * z).astype(np.float32)))           # absolute std, not clipped
        assert schedule_before == 0.1
        idx = a.nn_idx.cpu().numpy()
        assert np.array_equal(idx, R.knn_topk(proto, keys, K)[0])
        want_obs, want_act = R.candidates(idx, keys, s0)
        assert np.array_equal(bits(a.cand_obs.cpu().numpy()), bits(want_obs))
        assert np.array_equal(bits(a.cand_act.cpu().numpy()), bits(want_act))
        q = a.cand_q.cpu().numpy()
        assert q.shape == (N_ENV * K,) and np.isfinite(q).all()
        action, env_action = R.select(q, idx, table)
        assert np.array_equal(a.actions.cpu().numpy(), action)
        assert np.array_equal(bits(a.env_actions.cpu().numpy()), bits(env_action))
    assert ("mu", False) in a._graphs and ("rank",) in a._graphs

    # the replay's action column holds the integers
    col = a.memory.action.cpu().numpy()
    stored = np.concatenate(chosen)
    for v in range(1, BINS):
        assert int((col == v).sum()) == int((stored == v).sum()), v

    # TEST: the mean itself, no draw, no schedule step
    steps_before = dict(vars(pol.noise_schedule))
    a.phase = RunPhase.TEST
    for _ in range(3):
        state = np.random.get_state()
        a.choose_action(a.memory.current_states())
        torch.cuda.synchronize()
        after = np.random.get_state()
        assert np.array_equal(after[1], state[1]) and after[2] == state[2]
        assert np.array_equal(bits(a.proto.cpu().numpy()), bits(a._mu_act.cpu().numpy()))
        idx = a.nn_idx.cpu().numpy()
        assert np.array_equal(idx, R.knn_topk(a.proto.cpu().numpy(), keys, K)[0])
        assert np.array_equal(a.actions.cpu().numpy(), R.select(a.cand_q.cpu().numpy(), idx, table)[0])
    assert dict(vars(pol.noise_schedule)) == steps_before
    a.check_status()


def _ddpg_twin(dev, seed, episode_length, batch):
    """a DDPGAgent with the Wolpertinger agent's seeds, schemes and environment"""
    from coach_amd.agents.ddpg_agent import DDPGAgent, DDPGAgentParameters
    from coach_amd.environments.gym_environment import create
    gm = _graph_manager(seed=seed, episode_length=episode_length, batch=batch)
    ap = DDPGAgentParameters()
    ap.seed = seed
    for name in ("actor", "critic"):
        mine, theirs = ap.network_wrappers[name], gm.agent_params.network_wrappers[name]
        for field in ("observation_embedder_scheme", "middleware_scheme", "batch_size", "learning_rate"):
            setattr(mine, field, getattr(theirs, field))
    ap.network_wrappers["critic"].action_embedder_scheme = gm.agent_params.network_wrappers["critic"].action_embedder_scheme
    return DDPGAgent(ap, create(gm.env_params, dev), dev)


@pytest.mark.gpu
def test_update_equals_ddpg_on_the_converted_actions_bit_for_bit(dev):
    """same seeds, schemes and rows; the DDPG agent's replay holds target_actions[action] where the Wolpertinger agent's
    holds the action: weights and Adam state are identical after 1 update (on its own) and after 8 chained updates (one
    staged record, one graph), three times (eager, captured, replayed) — the conversion is exact and nothing else in
    DDPG's path moved"""
    import torch
    from coach_amd.core_types import RunPhase
    L, batch = 5, 16
    w = _agent(dev, seed=7, episode_length=L, batch=batch)
    d = _ddpg_twin(dev, 7, L, batch)
    _, table = _tables(w)
    for agent in (w, d):
        random.seed(3); np.random.seed(3)
        agent.phase = RunPhase.HEATUP
        for _ in range(3 * L):
            agent.act()
        agent.memory.commit_pending()
    assert torch.equal(w.memory.obs, d.memory.obs) and torch.equal(w.memory.reward, d.memory.reward)
    d.memory.action.copy_(w.d_target_actions[w.memory.action.long()].view_as(d.memory.action))
    assert d.memory.action.shape == (w.memory.action.shape[0], 1)

    def same():
        for name in ("actor", "critic"):
            x, y = w.networks[name], d.networks[name]
            for p, q in ((x.params.weights, y.params.weights), (x.target, y.target), (x.adam.m, y.adam.m),
                         (x.adam.v, y.adam.v), (x.adam.state, y.adam.state)):
                if not torch.equal(p, q):
                    return False
        return True

    def train(updates, seed):
        for agent in (w, d):
            random.seed(seed); np.random.seed(seed)
            agent.phase = RunPhase.TRAIN
            agent.ap.algorithm.num_consecutive_training_steps = updates
            agent.last_training_phase_step = agent.total_steps_counter - 1         # one phase is due
            agent.train()
        torch.cuda.synchronize()
    assert same()
    before = w.networks["actor"].params.weights.clone()
    train(1, 11)
    assert w.training_iteration == d.training_iteration == 1 and same()
    assert not torch.equal(before, w.networks["actor"].params.weights)
    for i in range(3):
        train(8, 20 + i)
        assert w.training_iteration == d.training_iteration == 1 + 8 * (i + 1) and same()
    assert any(k[0] == "chunk" for k in w._graphs) and any(k[0] == "chunk" for k in d._graphs)
    w.check_status()
    # a stored action outside the table raises the status bit
    w.memory.action.fill_(BINS)
    train(1, 40)
    with pytest.raises(RuntimeError, match="outside the 33 discrete actions"):
        w.check_status()


@pytest.mark.gpu
def test_preset_runs_logs_and_round_trips_a_checkpoint(dev, tmp_path):
    import torch
    from coach_amd.checkpoint import restore_checkpoint, save_checkpoint
    from coach_amd.core_types import EnvironmentSteps, RunPhase
    from coach_amd.graph_managers.basic_rl_graph_manager import CsvLogger
    gm = _graph_manager(seed=2, episode_length=10)
    gm.device = dev
    gm.schedule.heatup_steps = EnvironmentSteps(40)
    gm.schedule.improve_steps = EnvironmentSteps(200)          # one period of 20 episodes + its evaluation: ~300 steps
    gm.visualization_parameters.dump_csv = True
    path = str(tmp_path / "experiment.csv")
    gm.logger = CsvLogger(path)
    random.seed(1); np.random.seed(1)
    rows = gm.improve()
    a = gm.agent
    assert a.total_steps_counter == 240 and a.training_iteration == 200
    assert gm.total_steps_counters[RunPhase.TEST] == 40
    with open(os.path.join(GOLDEN, "csv_columns.json")) as f:
        gold = json.load(f)
    fixed = gold["dqn_columns"][:gold["dqn_columns"].index("Loss/Mean")]
    signals = ["Loss", "Learning Rate", "Grads (unclipped)", "Discounted Return", "Q", "TD targets", "actions"]
    want = [gold["dqn_index"]] + fixed + ["%s/%s" % (n, s) for n in signals for s in ("Mean", "Stdev", "Max", "Min")]
    with open(path, newline="") as f:
        table = list(csv.reader(f))
    assert table[0] == want and len(table) == 1 + len(rows) and len(rows) == 24 + 1
    logged = [r for r in rows if r["actions/Mean"] != ""]
    assert logged and all(0 <= float(r["actions/Min"]) <= float(r["actions/Max"]) <= BINS - 1 for r in logged)
    assert rows[-1]["Evaluation Reward"] != "" and np.isfinite(float(logged[-1]["Loss/Mean"]))

    save_checkpoint(a, str(tmp_path))
    gm2 = _graph_manager(seed=9, episode_length=10)
    gm2.device = dev
    gm2.visualization_parameters.dump_csv = False
    b = gm2.create_graph().agent
    assert not torch.equal(a.networks["actor"].params.weights, b.networks["actor"].params.weights)
    restore_checkpoint(b, str(tmp_path))
    for name in ("actor", "critic"):
        x, y = a.networks[name], b.networks[name]
        assert torch.equal(x.params.weights, y.params.weights) and torch.equal(x.target, y.target)
        assert torch.equal(x.adam.m, y.adam.m) and torch.equal(x.adam.v, y.adam.v)
    assert torch.equal(a.memory.action, b.memory.action) and b.memory.action.dtype == torch.int32
    assert b.total_steps_counter == 240 and b.training_iteration == 200
