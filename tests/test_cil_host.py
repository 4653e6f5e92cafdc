"""Host side of the CIL network: the reference's head scheme through coach_amd.compat, and the refusals (no GPU)."""
import pytest


def test_preset_head_scheme_through_compat():
    import coach_amd.compat
    coach_amd.compat.install()
    from rl_coach.architectures.head_parameters import RegressionHeadParameters
    from rl_coach.architectures.layers import BatchnormActivationDropout, Dense
    head = RegressionHeadParameters(scheme=[Dense(256), BatchnormActivationDropout(activation_function='tanh', dropout_rate=0.5),
                                            Dense(256), BatchnormActivationDropout(activation_function='tanh')],
                                    num_output_head_copies=4)                       # presets/CARLA_CIL.py:94-102
    assert head.native_scheme() == ((256, 256), (0.5, 0.0), 'tanh') and head.num_output_head_copies == 4
    assert RegressionHeadParameters().native_scheme() == ((256, 256), (0.0, 0.0), None)
    for scheme in ([Dense(8)], [Dense(8), BatchnormActivationDropout(batchnorm=True), Dense(8)],
                   [Dense(8), BatchnormActivationDropout(activation_function='relu'), Dense(8)]):
        with pytest.raises(ValueError, match="RegressionHeadParameters"):
            RegressionHeadParameters(scheme=scheme).native_scheme()


@pytest.mark.parametrize("kw,text", [(dict(embedder_dropout_rate=0.3), "input embedder"),
                                     (dict(middleware_dropout_rate=0.5), "middleware"), (dict(branches=1), "branches"),
                                     (dict(hidden=(24, 16)), "hidden"), (dict(action_dim=17), "units")])
def test_cilnet_refusals(kw, text):
    from coach_amd.nn.networks import CILNet
    args = dict(dict(obs_shape=(6,), action_dim=3, branches=4, hidden=(32, 16)), **kw)
    with pytest.raises(ValueError, match=text):
        CILNet("cpu", **args)
    with pytest.raises(NotImplementedError, match="image observations"):
        CILNet("cpu", (84, 84, 4), 3, 4)


PRESET = """
from rl_coach.agents.cil_agent import CILAgentParameters
from rl_coach.architectures.head_parameters import RegressionHeadParameters
from rl_coach.architectures.layers import Dense, BatchnormActivationDropout
from rl_coach.core_types import EnvironmentSteps
from rl_coach.exploration_policies.additive_noise import AdditiveNoiseParameters
from rl_coach.schedules import ConstantSchedule
agent_params = CILAgentParameters()
agent_params.network_wrappers['main'].heads_parameters = [RegressionHeadParameters(
    scheme=[Dense(256), BatchnormActivationDropout(activation_function='tanh', dropout_rate=0.5),
            Dense(256), BatchnormActivationDropout(activation_function='tanh')], num_output_head_copies=4)]
agent_params.network_wrappers['main'].batch_size = 120
agent_params.network_wrappers['main'].learning_rate = 0.0002
agent_params.exploration = AdditiveNoiseParameters()
agent_params.exploration.noise_schedule = ConstantSchedule(0)
agent_params.exploration.evaluation_noise = 0
agent_params.algorithm.num_consecutive_playing_steps = EnvironmentSteps(0)
agent_params.memory.state_key_with_the_class_index = 'high_level_command'
agent_params.memory.num_classes = 4
"""                                                                     # presets/CARLA_CIL.py:42, 93-107, 125-136


def _preset():
    import coach_amd.compat
    coach_amd.compat.install()
    scope = {}
    exec(PRESET, scope)
    return scope["agent_params"]


def _env(**kw):
    from types import SimpleNamespace
    p = dict(kind="vector", num_envs=1, observation_shape=(8,), num_actions=None, action_dim=2, action_low=-1.0,
             action_high=1.0, episode_length=4,
             observation_slices={"measurements": (0, 7), "high_level_command": (7, 8)})
    return SimpleNamespace(p=SimpleNamespace(**dict(p, **kw)), device="cpu")


def test_preset_style_parameters_through_compat():
    from coach_amd.agents.cil_agent import CILAgent, check_cil_parameters
    from coach_amd.nn.networks import cil_net_kwargs
    ap = _preset()
    assert ap.path == 'coach_amd.agents.cil_agent:CILAgent' and CILAgent.imitation
    assert check_cil_parameters(ap, _env().p) == (7, 7, 2)
    kw = cil_net_kwargs(ap.network_wrappers['main'], 0)
    assert (kw["branches"], kw["hidden"], kw["dropout_rates"], kw["head_activation"]) == (4, (256, 256), (0.5, 0.0), 'tanh')


def _set(path, value):
    def change(ap):
        obj, names = ap, path.split(".")
        for n in names[:-1]:
            obj = getattr(obj, n)
        setattr(obj, names[-1], value)
    return change


def _refusals():
    from coach_amd.core_types import CsvDataset, PickledReplayBuffer
    from coach_amd.exploration_policies.e_greedy import EGreedyParameters
    from coach_amd.exploration_policies.parameter_noise import ParameterNoiseParameters
    from coach_amd.memories.non_episodic.experience_replay import ExperienceReplayParameters
    return [(None, dict(kind="image"), {}, "not image observations"),
            (None, dict(action_dim=None, num_actions=3), {}, "not discrete actions"),
            (_set("exploration", object.__new__(ParameterNoiseParameters)), {}, {}, "ParameterNoise"),
            (_set("exploration", EGreedyParameters()), {}, {}, "AdditiveNoiseParameters"),
            (None, {}, dict(dist=object()), "data-parallel training"),
            (_set("memory.load_memory_from_file_path", PickledReplayBuffer("buffer.p")), {}, {}, "pickled replay buffer"),
            (_set("memory.load_memory_from_file_path", CsvDataset("data.csv")), {}, {}, "load_memory_from_file_path"),
            (_set("memory", ExperienceReplayParameters()), {}, {}, "BalancedExperienceReplay"),
            (_set("memory.state_key_with_the_class_index", "class"), {}, {}, r"under the given key \(class\)"),
            (_set("memory.num_classes", 3), {}, {}, "num_output_head_copies = 4"),
            (None, dict(num_envs=2), {}, "num_envs = 1"),
            (None, dict(observation_slices={"measurements": (0, 8)}), {}, "no width-1 slice named 'high_level_command'")]


@pytest.mark.parametrize("i", range(12))
def test_agent_refusals(i):
    from coach_amd.agents.cil_agent import CILAgent
    change, env_kw, kw, text = _refusals()[i]
    ap = _preset()
    if change:
        change(ap)
    with pytest.raises(ValueError, match=text):
        CILAgent(ap, _env(**env_kw), **kw)


def test_regression_head_is_refused_behind_the_backend_interface():
    from coach_amd.architectures.hip_architecture import _family_of
    with pytest.raises(NotImplementedError, match="does not serve a RegressionHead"):
        _family_of(_preset().network_wrappers['main'])


def _golden():
    import os
    import numpy as np
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cil.npz"))


def test_balanced_index_draws_as_the_reference():
    """class-major batches, both sampling modes draw for draw, eviction order, against the reference's recorded memory"""
    import numpy as np
    from coach_amd.memories.non_episodic.balanced_experience_replay import BalancedIndex
    g = _golden()
    for dup, key in ((True, "mem_dup"), (False, "mem_nodup")):
        index = BalancedIndex(3, 10)
        for c in g["mem_classes"]:
            index.store(c)
        np.random.seed(7)
        batches = np.array([index.sample(6, dup) for _ in range(3)])
        assert np.array_equal(batches, g[key]) and (g["mem_classes"][batches] == np.repeat(np.arange(3), 2)).all()
    assert list(index.transitions_order) == list(g["mem_order"]) and index.num_transitions() == 10
    assert all(list(index.transitions[c]) == list(g["mem_class%d" % c]) for c in range(3))


def test_balanced_replay_refusals_keep_the_reference_texts():
    import coach_amd.compat
    coach_amd.compat.install()
    from rl_coach.memories.memory import MemoryGranularity
    from rl_coach.memories.non_episodic.balanced_experience_replay import (
        BalancedExperienceReplay, BalancedExperienceReplayParameters, BalancedIndex)
    p = BalancedExperienceReplayParameters()
    assert (p.num_classes, p.state_key_with_the_class_index, p.allow_duplicates_in_batch_sampling) == (0, 'class', False)
    with pytest.raises(ValueError, match="should be at least 2. The number of classes that were defined are: 1"):
        BalancedExperienceReplay((MemoryGranularity.Transitions, 10), num_classes=1)
    with pytest.raises(ValueError, match="can only be set in terms of transitions"):
        BalancedExperienceReplay((MemoryGranularity.Episodes, 10), num_classes=2)
    index = BalancedIndex(2, 10)
    with pytest.raises(ValueError, match="The given class was: 2 and the number of classes defined is: 2"):
        index.store(2)
    with pytest.raises(ValueError, match="a multiple of the number of classes.*batch size requested is: 3"):
        index.sample(3, True)
    with pytest.raises(ValueError, match="not enough transitions yet. There are currently 0 transitions for class 0"):
        index.sample(2, False)
    with pytest.raises(ValueError, match="rescale_gradient_from_head_by_factor"):
        from coach_amd.architectures.head_parameters import RegressionHeadParameters
        from coach_amd.nn.networks import cil_net_kwargs
        from coach_amd.agents.bc_agent import BCNetworkParameters
        np_ = BCNetworkParameters()
        np_.heads_parameters = [RegressionHeadParameters(rescale_gradient_from_head_by_factor=0.5)]
        cil_net_kwargs(np_, 0)
