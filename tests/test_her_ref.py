"""Hindsight Experience Replay and BitFlip on the CPU: the numpy restatements (tests/her_ref.py, tests/bit_flip_ref.py)
against what the reference's own classes produced (tests/golden/her.npz, bit_flip.npz; make_golden_her.py,
make_golden_bit_flip.py), the parameter holders against the reference's defaults, and the package's two BitFlip presets
against the unchanged reference preset texts executed through the import layer (tests/golden/bit_flip_presets.json)."""
import importlib
import json
import os

import numpy as np
import pytest

import bit_flip_ref as BR
import her_ref as HR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def her():
    return np.load(os.path.join(GOLDEN, "her.npz"))


@pytest.fixture(scope="module")
def bit_flip():
    return np.load(os.path.join(GOLDEN, "bit_flip.npz"))


def her_cases(her):
    return json.loads(str(her["cases"])), json.loads(str(her["layouts"])), her["episode_lengths"].tolist()


def make_ref_memory(case, layout):
    return HR.HindsightReplay(case["max_size"], case["k"], case["method"], layout["desired_goal"][0],
                              layout["achieved"][0], layout["achieved"][1] - layout["achieved"][0], case["metric"],
                              case["threshold"], case["rewards"][0], case["rewards"][1])


# ------------------------------------------------------------------------------------------------ BitFlip dynamics
def test_bit_flip_restatement_reproduces_the_reference_class_exactly(bit_flip):
    cases = json.loads(str(bit_flip["cases"]))
    seen = set()
    for c, case in enumerate(cases):
        env = BR.BitFlip(case["L"], case["max_steps"], case["mean_zero"], case["state0"], case["goal0"])
        for i, a in enumerate(case["actions"]):
            obs, reward, done = env.step(a)
            for k in ("state", "desired_goal", "achieved_goal"):
                ref = bit_flip["c%d_%s" % (c, k)][i]
                assert np.array_equal(np.asarray(obs[k], dtype=np.float64), ref), (c, i, k)
            assert reward == bit_flip["c%d_reward" % c][i] and done == bool(bit_flip["c%d_done" % c][i]), (c, i)
        assert done
        seen.add((case["L"], case["mean_zero"], case["kind"]))
    for L in (1, 8, 20):
        for mz in (False, True):
            assert (L, mz, "early") in seen and (L, mz, "last") in seen and ((L, mz, "never") in seen or L == 1)
    assert any(c["max_steps"] not in (None, c["L"]) for c in cases)


def test_bit_flip_restatement_refuses_no_limit():
    with pytest.raises(ValueError, match="max_steps"):
        BR.BitFlip(4, 0, False, [0] * 4, [1] * 4)


def test_reset_draws_state_words_goal_words_and_the_forced_redraw():
    for L in (1, 8, 20, 33):
        goal, state, redraws = BR.draw_episode(11, 2, 5, L)
        assert goal.shape == state.shape == (L,) and not np.array_equal(goal, state)
        nw = (L + 31) // 32
        w = [BR.draw_word(11, 2, 5, i) for i in range(nw)]
        assert state.tolist() == [(w[i // 32] >> (i % 32)) & 1 for i in range(L)]       # low bit first, second word at 33
    seed, env, ep = BR.find_forced_redraw(1, 5)
    goal, state, redraws = BR.draw_episode(seed, env, ep, 1)
    assert redraws >= 1 and goal[0] != state[0]
    assert (BR.draw_word(seed, env, ep, 0) & 1) == (BR.draw_word(seed, env, ep, 1) & 1)     # the first goal draw == state


def test_vector_restatement_times_out_and_restarts():
    v = BR.VectorBitFlip(3, 4, max_steps=3, mean_zero=True, seed=3)
    first = v.reset()
    assert first.dtype == np.float32 and set(np.unique(first)) <= {-1.0, 1.0}
    ep0 = v.episode.copy()
    ended = np.zeros(3, dtype=np.int64)
    for _ in range(3):
        nxt, rst, rew, done = v.step([0, 0, 0])
        ended += done
        assert np.array_equal(rew == 0.0, np.all(nxt[:, :4] == nxt[:, 4:], axis=1))
    assert (ended >= 1).all() and np.array_equal(v.episode, ep0 + ended)      # by the limit of 3 steps at the latest
    v.step([4, -1, 0])
    assert v.status == 2


# ------------------------------------------------------------------------------------------------ hindsight replay
@pytest.mark.parametrize("c", range(24))
def test_her_restatement_reproduces_the_reference_memory_exactly(her, c):
    cases, layouts, lengths = her_cases(her)
    case = cases[c]
    mem = make_ref_memory(case, layouts[case["layout"]])
    np.random.seed(1000 + c)
    for s, T in enumerate(lengths):
        p = "c%d_s%d_" % (c, s)
        assert her[p + "in_obs"].shape[0] == T
        mem.store_episode(her[p + "in_obs"], her[p + "in_next_obs"], her[p + "in_action"], her[p + "in_reward"],
                          her[p + "in_game_over"])
        flat = mem.flat()
        for k in ("obs", "next_obs", "action", "reward", "game_over"):
            assert np.array_equal(flat[k], her[p + k]), (c, s, k)
        state = np.random.get_state()
        assert np.random.random() == float(her[p + "peek"]), (c, s)         # the stream was consumed as the reference did
        np.random.set_state(state)


def test_her_fixture_holds_the_cases_it_is_checked_on(her):
    cases, layouts, lengths = her_cases(her)
    assert sorted(set(lengths)) == [1, 2, 7]
    assert {(c["k"], c["method"], c["metric"], c["threshold"]) for c in cases} == \
        {(k, m, d, t) for k in (1, 4) for m in ("Final", "Future", "Episode") for d in ("Euclidean", "Manhattan")
         for t in (0.0, 0.5)}
    for c, case in enumerate(cases):
        k, future = case["k"], case["method"] == "Future"
        sizes = [(T + (T - 1 if future else T) * k) for T in lengths]
        # zero copies for Future at T = 1: the second store adds exactly one row or evicts down to fit
        assert sizes[1] == (1 if future else 1 + k)
        n_last = her["c%d_s%d_reward" % (c, len(lengths) - 1)].shape[0]
        assert n_last < sum(sizes) and n_last <= case["max_size"]                # whole extended episodes were evicted
        go = np.concatenate([her["c%d_s%d_game_over" % (c, s)] for s in range(len(lengths))])
        assert go.any() and not go.all()


def test_distance_is_fp64_in_index_order():
    g, a = np.array([0.1, 0.2, 0.3], np.float32), np.array([1.0, -2.0, 0.5], np.float32)
    d = [float(x) - float(y) for x, y in zip(g, a)]
    assert HR.distance(g, a, HR.EUCLIDEAN) == float(np.sqrt(np.float64((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))
    assert HR.distance(g, a, HR.MANHATTAN) == (abs(d[0]) + abs(d[1])) + abs(d[2])


# ------------------------------------------------------------------------------------------ parameter holders, presets
def test_parameter_classes_have_the_reference_fields_and_path():
    from coach_amd.memories.episodic.episodic_hindsight_experience_replay import (
        EpisodicHindsightExperienceReplayParameters, HindsightGoalSelectionMethod)
    from coach_amd.memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters
    p = EpisodicHindsightExperienceReplayParameters()
    assert isinstance(p, EpisodicExperienceReplayParameters)
    assert p.hindsight_transitions_per_regular_transition is None and p.hindsight_goal_selection_method is None
    assert p.goals_space is None
    assert p.path == ("coach_amd.memories.episodic.episodic_hindsight_experience_replay:"
                      "EpisodicHindsightExperienceReplay")
    assert [(m.name, m.value) for m in HindsightGoalSelectionMethod] == \
        [("Future", 0), ("Final", 1), ("Episode", 2), ("Random", 3)]


def test_spaces_hold_the_reference_constructor_signatures():
    from coach_amd.spaces import GoalsSpace, InverseDistanceFromGoal, ReachingGoal
    r = ReachingGoal(distance_from_goal_threshold=0.25)
    assert (r.distance_from_goal_threshold, r.goal_reaching_reward, r.default_reward) == (0.25, 0, -1)
    i = InverseDistanceFromGoal(0.5)
    assert (i.distance_from_goal_threshold, i.max_reward, i.goal_reaching_reward) == (0.5, 1, 1)
    g = GoalsSpace(goal_name="state", reward_type=r, distance_metric=GoalsSpace.DistanceMetric.Manhattan)
    assert g.goal_name == "state" and g.reward_type is r
    assert [(m.name, m.value) for m in GoalsSpace.DistanceMetric] == [("Euclidean", 0), ("Cosine", 1), ("Manhattan", 2)]


def test_reference_module_paths_resolve_through_the_import_layer():
    import coach_amd.compat as compat
    compat.install()
    from rl_coach.architectures.embedder_parameters import InputEmbedderParameters
    from rl_coach.base_parameters import EmbedderScheme
    from rl_coach.memories.episodic.episodic_hindsight_experience_replay import \
        EpisodicHindsightExperienceReplayParameters
    from rl_coach.spaces import GoalsSpace
    import coach_amd.spaces as mine
    assert GoalsSpace is mine.GoalsSpace
    assert InputEmbedderParameters(scheme=EmbedderScheme.Empty).scheme == EmbedderScheme.Empty
    assert EpisodicHindsightExperienceReplayParameters().goals_space is None


def test_input_embedders_setter_accepts_only_what_the_network_can_build():
    from coach_amd.agents.dqn_agent import DQNAgentParameters
    from coach_amd.architectures.embedder_parameters import InputEmbedderParameters
    from coach_amd.base_parameters import EmbedderScheme
    net = DQNAgentParameters().network_wrappers["main"]
    net.input_embedders_parameters = {"observation": InputEmbedderParameters(scheme=EmbedderScheme.Shallow)}
    assert net.embedder_scheme == "Shallow" and list(net.input_embedders_parameters) == ["observation"]
    net.input_embedders_parameters = {"state": InputEmbedderParameters(scheme=EmbedderScheme.Empty),
                                      "desired_goal": InputEmbedderParameters(scheme=EmbedderScheme.Empty)}
    assert net.embedder_scheme == "Empty" and sorted(net.input_embedders_parameters) == ["desired_goal", "state"]
    assert net.input_embedder_names == ("desired_goal", "state")
    with pytest.raises(ValueError, match="Empty"):
        net.input_embedders_parameters = {"state": InputEmbedderParameters(scheme=EmbedderScheme.Medium),
                                          "desired_goal": InputEmbedderParameters(scheme=EmbedderScheme.Empty)}
    with pytest.raises(ValueError):
        net.input_embedders_parameters = {}
    with pytest.raises(ValueError):
        net.input_embedders_parameters = {"camera": InputEmbedderParameters()}


@pytest.mark.parametrize("name", ["BitFlip_DQN", "BitFlip_DQN_HER"])
def test_package_presets_equal_the_unchanged_reference_preset_texts(name):
    """tests/golden/bit_flip_presets.json holds what the reference's preset texts, executed unchanged through the import
    layer, set (make_bit_flip_preset_dumps.py): the package's presets must equal them field by field."""
    from coach_amd.compat import resolve_reference_style
    from test_cartpole import _dump
    with open(os.path.join(GOLDEN, "bit_flip_presets.json")) as f:
        ref = json.load(f)[name]
    mine = importlib.import_module("coach_amd.presets." + name).make()
    resolve_reference_style(mine.agent_params, mine.env_params)
    for part in ("agent_params", "env_params", "schedule", "preset_validation_params"):
        assert ref[part] == _dump(getattr(mine, part)), part
    alg = mine.agent_params.algorithm
    if name == "BitFlip_DQN_HER":                  # (_dump keeps an enum member's class only: the members are compared here)
        from coach_amd.memories.episodic.episodic_hindsight_experience_replay import HindsightGoalSelectionMethod
        from coach_amd.spaces import GoalsSpace
        mem = mine.agent_params.memory
        assert mem.hindsight_goal_selection_method is HindsightGoalSelectionMethod.Final
        assert mem.goals_space.distance_metric is GoalsSpace.DistanceMetric.Euclidean
        assert mem.hindsight_transitions_per_regular_transition == 1 and mem.goals_space.goal_name == "state"
    assert sorted(mine.agent_params.network_wrappers["main"].input_embedders_parameters) == ["desired_goal", "state"]
    assert type(alg.num_consecutive_playing_steps).__name__ == "EnvironmentEpisodes"
    assert alg.num_consecutive_playing_steps.num_steps == 16 and alg.num_consecutive_training_steps == 40
    v = mine.preset_validation_params
    assert v.test and v.max_episodes_to_achieve_reward == 10000
    assert v.min_reward_threshold == (-7.9 if name == "BitFlip_DQN" else -15)
    assert mine.env_params.additional_simulator_parameters == \
        {"bit_length": 8 if name == "BitFlip_DQN" else 20, "mean_zero": True}
