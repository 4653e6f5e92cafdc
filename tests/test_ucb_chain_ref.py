"""UCB over Q ensembles and the ExplorationChain on the CPU: the numpy restatements (tests/ucb_ref.py,
tests/exploration_chain_ref.py) and the package's PieceWiseSchedule against what the reference's own classes produced
(tests/golden/ucb_chain.npz, make_golden_ucb_chain.py), the parameter holders and the four presets against the unchanged
reference preset texts (tests/golden/ucb_chain_presets.json), the import layer, the agent's seam and the C ABI entries."""
import importlib
import json
import os
import re

import numpy as np
import pytest

import exploration_chain_ref as CR
import ucb_ref as UR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_PRESETS = "/root/reference/rl_coach/presets"
PRESETS = ["ExplorationChain_UCB_Q_ensembles", "ExplorationChain_Bootstrapped_DQN", "ExplorationChain_Dueling_DDQN",
           "Atari_UCB_with_Q_Ensembles"]
CHAIN_LEVEL = 'rl_coach.environments.toy_problems.exploration_chain:ExplorationChain'


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "ucb_chain.npz"))


def ucb_cases(gold):
    return [tuple(c) for c in json.loads(str(gold["ucb_cases"]))]


def acting_draws(gold, s, A):
    """the draws the fixture's calls made: np.random.seed(seed0 + env) right before every get_action (epsilon 0.5)"""
    u, seed0 = gold["ucb%d_u" % s], int(gold["ucb%d_seed0" % s])
    ra, tie = np.zeros(len(u), np.int32), np.zeros((len(u), A))
    for e in range(len(u)):
        rs = np.random.RandomState(seed0 + e)
        if u[e] < 0.5:
            ra[e] = rs.choice(A)
        else:
            tie[e] = rs.random_sample(A)
    return u, ra, tie


# --------------------------------------------------------------------------------------------------------- UCB values
@pytest.mark.parametrize("s", range(12))
def test_ucb_restatement_equals_the_reference_policy_bit_for_bit(gold, s):
    K, A, lamb = ucb_cases(gold)[s]
    q = gold["ucb%d_q" % s]
    assert q.shape == (5, K, A) and q.dtype == np.float32
    u, ra, tie = acting_draws(gold, s, A)
    greedy = u >= 0.5                                         # (an exploring call of the reference computes no values)
    for name, use_std in (("train", True), ("test", False)):
        vals, std = UR.values(q, lamb, use_std)
        ref = gold["ucb%d_%s_values" % (s, name)]
        assert ref.dtype == np.float32
        assert np.array_equal(vals[greedy].view(np.uint32), ref[greedy].view(np.uint32)), name
        if use_std:
            ref_std = gold["ucb%d_train_std" % s]
            assert np.array_equal(std[greedy].view(np.uint32), ref_std[greedy].view(np.uint32))
        else:
            assert std is None
        assert UR.egreedy(vals, u, ra, tie, 0.5).tolist() == gold["ucb%d_%s_actions" % (s, name)].tolist(), name
    # the cases the fixture holds
    train, std = gold["ucb%d_train_values" % s], gold["ucb%d_train_std" % s]
    assert len(set(train[1].tolist())) == 1 and not std[1].any()          # all heads equal: the tie draw decides
    assert train[2, 0] == train[2, A - 1] == train[2].max()                 # two actions exactly tied
    assert gold["ucb%d_train_actions" % s][1] == int(np.argmax(tie[1]))
    assert gold["ucb%d_train_actions" % s][2] == (0 if tie[2, 0] > tie[2, A - 1] else A - 1)
    assert (K == 1) == (not std[greedy].any()) and not greedy[4] and np.abs(train[3]).max() > 100
    test = gold["ucb%d_test_values" % s]
    assert (K == 1) == np.array_equal(train[greedy], test[greedy])          # the bonus is TRAIN's alone


def test_ucb_fixture_holds_the_cases_it_is_checked_on(gold):
    assert sorted(ucb_cases(gold)) == sorted((K, A, lamb) for K in (1, 2, 20) for A in (2, 18) for lamb in (0.1, 10))


def test_ucb_restatement_states_the_order_it_claims():
    """three heads whose sum depends on the order, and lamb rounded to fp32 before the product"""
    F = np.float32
    q = np.array([[[1e8], [1.0], [-1e8]]], dtype=F)
    vals, std = UR.values(q, 0.1, True)
    mean = F(F(F(F(1e8) + F(1.0)) + F(-1e8)) / F(3))
    assert mean == 0.0 and F(F(F(1e8) + F(-1e8)) + F(1.0)) / F(3) != 0.0
    d = [F(x - mean) for x in (F(1e8), F(1.0), F(-1e8))]
    sd = np.sqrt(F(F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2])) / F(3)))
    assert std[0, 0] == sd and vals[0, 0] == F(mean + F(F(0.1) * sd))
    assert UR.same_bits(np.array([np.nan, 1.0], F), np.array([-np.nan, 1.0], F))
    assert not UR.same_bits(np.array([0.0], F), np.array([-0.0], F))


# ------------------------------------------------------------------------------------------------- PieceWiseSchedule
def test_piecewise_schedule_equals_the_reference_trace_exactly(gold):
    from coach_amd.core_types import EnvironmentSteps
    from coach_amd.schedules import LinearSchedule, PieceWiseSchedule
    pieces = [(LinearSchedule(a, b, int(n)), EnvironmentSteps(int(m))) for a, b, n, m in gold["schedule_pieces"]]
    sch = PieceWiseSchedule(pieces)
    values, idx, count = gold["schedule_values"], gold["schedule_idx"], gold["schedule_count"]
    assert sch.initial_value == values[0] and sch.current_value == values[0]
    for i in range(1, len(values)):
        sch.step()
        assert float(sch.current_value) == values[i], i
        assert (sch.current_schedule_idx, sch.current_schedule_step_count) == (idx[i], count[i]), i
    switches = np.nonzero(np.diff(idx))[0] + 1
    assert len(switches) == 2 and idx[-1] == 2
    # the rule's mark: the first piece is advanced num_steps + 1 times, the switching step reports the next piece's
    # untouched initial value and already counts 1 for it
    assert switches[0] == pieces[0][1].num_steps + 1 and switches[1] - switches[0] == pieces[1][1].num_steps
    assert values[switches[0]] == pieces[1][0].initial_value and count[switches[0]] == 1
    assert values[-1] == values[-2] == 0.0                                 # the last piece is never left


def test_ucb_parameters_have_the_reference_fields_and_defaults():
    from coach_amd.exploration_policies.e_greedy import EGreedyParameters
    from coach_amd.exploration_policies.ucb import UCBParameters
    from coach_amd.schedules import LinearSchedule, PieceWiseSchedule
    p = UCBParameters()
    assert isinstance(p, EGreedyParameters)
    assert (p.architecture_num_q_heads, p.bootstrapped_data_sharing_probability, p.lamb) == (10, 1.0, 0.1)
    assert p.evaluation_epsilon == 0.05 and p.path == 'coach_amd.exploration_policies.ucb:UCB'
    sch = p.epsilon_schedule
    assert isinstance(sch, PieceWiseSchedule) and len(sch.schedules) == 2 and sch.current_value == 1
    got = [(type(s), s.initial_value, s.final_value, s.decay_steps, type(n).__name__, n.num_steps)
           for s, n in sch.schedules]
    assert got == [(LinearSchedule, 1, 0.1, 1000000, "EnvironmentSteps", 1000000),
                   (LinearSchedule, 0.1, 0.01, 4000000, "EnvironmentSteps", 4000000)]


def test_ucb_policy_draws_no_head_and_adds_the_bonus_in_train_only():
    from coach_amd.core_types import RunPhase
    from coach_amd.exploration_policies.ucb import UCB, UCBParameters
    np.random.seed(4)
    pol = UCB(3, 2, "cpu", UCBParameters())
    before = np.random.get_state()
    pol.select_head()
    pol.select_head([1, 0])
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert not hasattr(pol, "selected_head") and not hasattr(pol, "stage_heads")
    pol.std[:] = 2.0
    pol.std[1, 0] = 5.0
    for phase in RunPhase:
        pol.phase = phase
        assert pol.use_std == (phase == RunPhase.TRAIN)
        c = pol.get_control_param()
        if phase == RunPhase.TRAIN:
            assert np.asarray(c).tolist() == [2.0, 3.0]
        else:
            assert c == 0
    # EGreedy's draws, unchanged: the stream moves exactly as the plain policy moves it
    from coach_amd.exploration_policies.e_greedy import EGreedy
    states = []
    for cls in (UCB, EGreedy):
        np.random.seed(6)
        p = cls(3, 2, "cpu", UCBParameters())
        p.phase = RunPhase.TRAIN
        for _ in range(5):
            p.draw()
        states.append(np.random.get_state())
    assert np.array_equal(states[0][1], states[1][1]) and states[0][2:] == states[1][2:]


# --------------------------------------------------------------------------------------------------- ExplorationChain
def test_chain_restatement_reproduces_the_reference_class_exactly(gold):
    cases = json.loads(str(gold["chain_cases"]))
    seen, walls = set(), set()
    for c, case in enumerate(cases):
        env = CR.VectorExplorationChain(1, case["L"], case["start"], case["max_steps"], case["therm"], case["left"],
                                        case["right"])
        p = "chain%d_" % c
        i = 0
        for episode in range(2):
            first = env.reset()
            assert first.dtype == np.float32 and np.array_equal(first[0].astype(np.float64), gold[p + "first"][episode])
            for a in case["actions"]:
                before = int(env.state[0])
                nxt, rst, rew, done = env.step([a])
                assert np.array_equal(nxt[0].astype(np.float64), gold[p + "obs"][i]), (c, i)
                assert rew.dtype == np.float32 and rew[0] == np.float32(gold[p + "reward"][i]), (c, i)
                assert bool(done[0]) == bool(gold[p + "done"][i]), (c, i)
                if done[0]:
                    assert np.array_equal(rst[0], first[0]) and env.state[0] == case["start"] and env.steps[0] == 0
                elif int(env.state[0]) == before:
                    walls.add("left" if a == 0 else "right")
                i += 1
            assert done[0]
        assert i == len(gold[p + "done"]) and env.status == 0
        seen.add((case["therm"], case["L"], case["start"]))
    for therm in (True, False):
        for L in (4, 20):
            for start in (0, 1, L - 1):
                assert (therm, L, start) in seen
    assert walls == {"left", "right"} and any(c["max_steps"] == 1 for c in cases)
    assert any(float(np.float32(c["left"])) != c["left"] for c in cases)           # a reward fp32 does not hold exactly
    rewards = np.concatenate([gold["chain%d_reward" % c] for c in range(len(cases))])
    assert {0.0, 1 / 1000, 1.0} <= set(rewards.tolist())


def test_chain_restatement_flags_other_actions_and_keeps_the_reference_refusals():
    v = CR.VectorExplorationChain(3, 4, 1, 5, False)
    first = v.reset()
    assert first.tolist() == [[0, 1, 0, 0]] * 3
    nxt, _, rew, done = v.step([2, -1, 1])
    assert v.status == 2 and v.state.tolist() == [1, 1, 2] and v.steps.tolist() == [1, 1, 1] and not done.any()
    assert nxt.tolist() == [[0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]] and not rew.any()
    for kw in (dict(chain_length=3), dict(chain_length=4, start_state=4), dict(chain_length=4, start_state=-1),
               dict(chain_length=4, max_steps=None)):
        with pytest.raises(ValueError):
            CR.VectorExplorationChain(1, **dict(dict(max_steps=3), **kw))


def test_environment_parameters_follow_the_reference_constructor():
    from coach_amd.environments import gym_environment as G
    from coach_amd.environments.exploration_chain_vector_environment import (
        ExplorationChainVectorEnvironmentParameters as P, ObservationType)
    assert [(m.name, m.value) for m in ObservationType] == [("OneHot", 0), ("Therm", 1)]
    p = P(2, max_steps=9)
    assert (p.chain_length, p.start_state, p.observation_type, p.left_state_reward, p.right_state_reward) == \
        (16, 1, ObservationType.Therm, 1 / 1000, 1.0)
    assert (p.kind, p.num_envs, p.observation_shape, p.num_actions, p.action_dim) == ("vector", 2, (16,), 2, None)
    assert p.episode_length == p.min_episode_length == 9 and p.level == CHAIN_LEVEL == G.EXPLORATION_CHAIN_LEVEL
    with pytest.raises(ValueError, match="Chain length must be > 3"):
        P(1, chain_length=3, max_steps=5)
    for start in (-1, 4):
        with pytest.raises(ValueError, match="within the chain bounds"):
            P(1, chain_length=4, start_state=start, max_steps=5)
    for limit in (None, 0):
        with pytest.raises(ValueError, match="max_steps"):
            P(1, max_steps=limit)
    with pytest.raises(ValueError, match="OneHot or Therm"):
        P(1, max_steps=5, observation_type="Binary")
    assert P(1, max_steps=5, observation_type="OneHot").observation_type is ObservationType.OneHot
    # the level's parameters from additional_simulator_parameters, for both parameter classes
    for cls in (G.GymVectorEnvironment, G.GymEnvironmentParameters):
        e = cls(level=CHAIN_LEVEL)
        e.additional_simulator_parameters = {'chain_length': 20, 'max_steps': 27}
        e.num_envs = 3
        q = G.exploration_chain_parameters(e)
        assert (q.num_envs, q.chain_length, q.episode_length, q.start_state) == (3, 20, 27, 1)
        e.episode_length = 5
        assert G.exploration_chain_parameters(e).episode_length == 5
        e.additional_simulator_parameters = {'chain_length': 20, 'max_steps': 27, 'bit_length': 4}
        with pytest.raises(ValueError, match="bit_length"):
            G.exploration_chain_parameters(e)
        e.additional_simulator_parameters = {'chain_length': 20}
        e.episode_length = None
        with pytest.raises(ValueError, match="max_steps"):
            G.exploration_chain_parameters(e)


# ----------------------------------------------------------------------------------- import layer, presets, the seam
def test_reference_module_paths_resolve_through_the_import_layer():
    import coach_amd.compat as compat
    compat.install()
    ucb = importlib.import_module("rl_coach.exploration_policies.ucb")
    from rl_coach.filters.filter import NoInputFilter, NoOutputFilter
    from rl_coach.schedules import PieceWiseSchedule
    import coach_amd.exploration_policies.ucb as mine
    import coach_amd.filters as filters
    import coach_amd.schedules as schedules
    assert ucb.UCB is mine.UCB and ucb.UCBParameters is mine.UCBParameters
    assert PieceWiseSchedule is schedules.PieceWiseSchedule
    assert NoOutputFilter is filters.NoOutputFilter and NoInputFilter is filters.NoInputFilter
    assert isinstance(NoOutputFilter(), filters.OutputFilter)
    with pytest.raises(ValueError, match="no device implementation"):
        filters.OutputFilter(action_filters={"rescale": object()})


@pytest.mark.parametrize("name", PRESETS)
def test_package_presets_equal_the_unchanged_reference_preset_texts(name):
    """tests/golden/ucb_chain_presets.json holds what the reference's preset texts, executed unchanged through the import
    layer, set (make_ucb_chain_preset_dumps.py): the package's presets must equal them field by field."""
    from coach_amd.compat import resolve_reference_style
    from test_cartpole import _dump
    with open(os.path.join(GOLDEN, "ucb_chain_presets.json")) as f:
        ref = json.load(f)[name]
    mine = importlib.import_module("coach_amd.presets." + name).make()
    resolve_reference_style(mine.agent_params, mine.env_params)
    for part in ("agent_params", "env_params", "schedule", "preset_validation_params"):
        assert ref[part] == _dump(getattr(mine, part)), part
    ap, exp = mine.agent_params, mine.agent_params.exploration
    if name.startswith("ExplorationChain"):
        assert mine.env_params.level == CHAIN_LEVEL
        assert mine.env_params.additional_simulator_parameters == {'chain_length': 20, 'max_steps': 27}
        assert type(mine.env_params).__name__ == ("GymEnvironmentParameters" if "Dueling" in name
                                                  else "GymVectorEnvironment")
        assert type(mine.schedule.improve_steps).__name__ == "EnvironmentEpisodes"
        assert mine.schedule.improve_steps.num_steps == 2000 and mine.schedule.heatup_steps.num_steps == 20
        assert type(ap.output_filter).__name__ == "NoOutputFilter" and type(ap.input_filter).__name__ == "NoInputFilter"
        assert ap.algorithm.reward_clipping is None and ap.network_wrappers["main"].learning_rate == 0.00025
    if name == "ExplorationChain_UCB_Q_ensembles":
        assert type(exp).__name__ == "UCBParameters" and exp.lamb == 10 and exp.architecture_num_q_heads == 20
        assert type(exp.epsilon_schedule).__name__ == "ConstantSchedule" and exp.epsilon_schedule.current_value == 0
        assert ap.network_wrappers["main"].heads_parameters[0].num_output_head_copies == 20
    elif name == "ExplorationChain_Bootstrapped_DQN":
        assert type(exp).__name__ == "BootstrappedParameters" and exp.architecture_num_q_heads == 20
    elif name == "ExplorationChain_Dueling_DDQN":
        assert type(ap.network_wrappers["main"].heads_parameters[0]).__name__ == "DuelingQHeadParameters"
        assert exp.epsilon_schedule.decay_steps == 27 * 2000
    else:
        assert type(exp).__name__ == "UCBParameters" and exp.lamb == 0.1 and exp.architecture_num_q_heads == 10
        assert type(exp.epsilon_schedule).__name__ == "PieceWiseSchedule" and mine.env_params.is_atari


@pytest.mark.skipif(not os.path.isdir(REF_PRESETS), reason="needs the reference tree (build container)")
@pytest.mark.parametrize("name", PRESETS)
def test_reference_preset_text_executes_unchanged(name):
    from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager
    from test_preset_dropin import _exec_preset
    ns = _exec_preset(open(os.path.join(REF_PRESETS, name + ".py")).read())
    gm = ns["graph_manager"]
    assert isinstance(gm, BasicRLGraphManager)
    assert gm.agent_params is ns["agent_params"] and gm.env_params is ns["env_params"]
    assert type(gm.agent_params).__module__.startswith("coach_amd.agents.")
    if "UCB" in name:
        assert type(gm.agent_params.exploration).__module__ == "coach_amd.exploration_policies.ucb"


class _HostOnly(object):
    """the host half of a UCB BootstrappedDQNAgent's draws, without a device (as tests/test_bootstrapped_dqn_ref.py)"""

    def __init__(self, n_env, K, p):
        from coach_amd.agents.bootstrapped_dqn_agent import BootstrappedDQNAgent as Agent
        from coach_amd.exploration_policies.ucb import UCB, UCBParameters
        a = self.a = Agent.__new__(Agent)
        a.n_env, a.K, a.share_p, a.ucb = n_env, K, p, True
        params = UCBParameters()
        params.architecture_num_q_heads = K
        a.exploration_policy = UCB(2, n_env, "cpu", params)
        a._needs_head = np.ones(n_env, dtype=bool)
        a._open_rows, a.debug_masks = None, None

    def step(self, dones):
        self.a._observe_previous_host(False)
        self.a._store_extra_host(np.asarray(dones), False)


@pytest.mark.parametrize("n_env,p", [(1, 1.0), (3, 0.7)])
def test_a_ucb_agent_draws_its_masks_and_no_head(n_env, p):
    """the reference's calls per env and step with UCB: select_head is `pass`, observe draws binomial(1, p, K) for the
    previous response and once more at once for a terminal one"""
    K, steps = 10, 17
    ends = np.zeros((steps, n_env), bool)
    for e in range(n_env):
        ends[3 + 2 * e::5 + e, e] = True
    np.random.seed(11)
    h = _HostOnly(n_env, K, p)
    np.random.seed(12)
    for t in range(steps):
        h.step(ends[t])
    after = np.random.get_state()
    np.random.seed(12)
    for t in range(steps):
        for e in range(n_env):
            np.random.binomial(1, p, K)
        for e in range(n_env):
            if ends[t, e]:
                np.random.binomial(1, p, K)
    ref = np.random.get_state()
    assert ends.any() and np.array_equal(after[1], ref[1]) and after[2:] == ref[2:]
    assert not h.a._needs_head.any() or ends[-1].any()


def test_abi_declares_the_three_entry_points():
    from coach_amd import _rlx
    protos = _rlx.parse_header()
    act = [n for _, n in protos["rlx_ucb_egreedy"][1]]
    assert act == ["q_values", "ld", "n_heads", "lamb", "use_std", "explore_uniforms", "random_actions",
                   "tie_break_uniforms", "epsilon", "n_env", "n_actions", "values_out", "std_out", "actions", "stream"]
    import ctypes
    assert protos["rlx_ucb_egreedy"][1][3][0] is ctypes.c_float          # lamb: the fp32 nearest the Python value
    reset = [n for _, n in protos["rlx_chain_reset"][1]]
    assert reset == ["state", "steps", "obs", "n_env", "chain_length", "start_state", "therm", "stream"]
    step = [n for _, n in protos["rlx_chain_step"][1]]
    assert step == ["action", "state", "steps", "next_obs", "reset_obs", "reward", "game_over", "n_env", "chain_length",
                    "start_state", "max_steps", "therm", "left_state_reward", "right_state_reward", "status", "stream"]
    boot = open(os.path.join(ROOT, "coach_amd", "csrc", "bootstrapped_dqn.hip")).read()
    chain = open(os.path.join(ROOT, "coach_amd", "csrc", "exploration_chain.hip")).read()
    assert re.search(r"\bint\s+rlx_ucb_egreedy\s*\(", boot)
    for name in ("rlx_chain_reset", "rlx_chain_step"):
        assert re.search(r"\bint\s+%s\s*\(" % name, chain)
    # ONE epsilon-greedy tail in the file, called by both acting kernels
    assert len(re.findall(r"__device__[^;{]*\begreedy_choice\s*\(", boot)) == 1
    assert len(re.findall(r"=\s*egreedy_choice\s*\(", boot)) == 2 and boot.count("1e-8f + 1e-5f") == 1
    assert _rlx.ABI_VERSION == 11                                          # entry points were only added
    if os.path.exists(_rlx.LIB_PATH):
        lib = _rlx.lib()
        for name in ("ucb_egreedy", "chain_reset", "chain_step"):
            assert callable(getattr(lib, name))
