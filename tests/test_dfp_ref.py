"""tests/dfp_ref.py against the reference agent's recorded values (tests/golden/dfp.npz, written by
tests/golden/make_golden_dfp.py from DFPAgent's own code): the restatement equals every recorded array bit for bit, NaN
positions included; its gradient equals central differences of its own loss; the build and the binding carry what the
kernels need.  No GPU."""
import os
import re

import numpy as np
import pytest

import dfp_ref as R
from dfp_ref import ACT_CASES, ACT_STEPS, LEARN_CASES, LENGTHS, MEAS, SCALES, STEPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(name, got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, ref.dtype, got.shape, ref.shape)
    assert np.array_equal(_bits(got), _bits(ref)), name


@pytest.mark.parametrize("M", MEAS)
@pytest.mark.parametrize("T", LENGTHS)
def test_future_measurements_equal_the_reference(golden, T, M):
    g = golden("dfp")
    meas = g["fm_T%d_M%d_meas" % (T, M)]
    assert meas.dtype == np.float64 and not np.array_equal(meas, meas.astype(np.float32).astype(np.float64))
    for S in STEPS:
        for mode in ("NAN", "LastStep"):
            for sname, scale in SCALES.items():
                rec = g["fm_T%d_M%d_S%d_%s_%s" % (T, M, S, mode, sname)]
                assert rec.dtype == np.float64 and rec.shape == (T, S, M)
                got = R.future_measurements(meas, S, scale[:M], mode == "LastStep")
                _same((T, M, S, mode, sname), got, rec.astype(np.float32))
                # where the targets lie: step s of transition i exists iff i + 2^s < T
                exists = (np.arange(T)[:, None] + 2 ** np.arange(S)[None, :]) < T
                assert np.array_equal(np.isnan(rec).any(axis=2), ~exists if mode == "NAN" else np.zeros_like(exists))
                if mode == "LastStep" and T > 1:           # the LAST transition's state, not its next state
                    i, s = np.argwhere(~exists)[0]
                    assert np.array_equal(rec[i, s], np.asarray(scale[:M]) * (meas[T - 1] - meas[i]))


@pytest.mark.parametrize("case", range(len(LEARN_CASES)))
def test_targets_of_learn_from_batch_equal_the_reference(golden, case):
    g = golden("dfp")
    p = "learn%d_" % case
    B, A, S, M = LEARN_CASES[case]
    E, X, actions, future = g[p + "E"], g[p + "X"], g[p + "actions"], g[p + "future"]
    assert E.shape == (B, S * M) and X.shape == (B, A, S * M) and future.shape == (B, S, M)
    r = R.head_loss(E, X, actions, future)
    _same("y", r["y"], g[p + "y"])
    rec = g[p + "targets"]
    # the reference keeps the NaNs in its targets (the head's tf.where replaces them); the restatement has replaced them
    nan = np.isnan(rec)
    assert np.array_equal(nan[np.arange(B), actions], np.isnan(future.reshape(B, -1)))
    assert nan.sum() == np.isnan(future).sum()
    _same("targets", r["targets"], np.where(nan, r["y"], rec))
    rows = np.isnan(future.reshape(B, -1))
    assert (~rows.any(axis=1)).any() and (B == 1 or rows.all(axis=1).any())
    assert np.all(r["dE"][rows] == 0) and np.all(r["dX"][rows.all(axis=1)] == 0)
    # the loss is the head's: sum over (a, k) of the batch mean of (targets_nonan - y)^2
    d = (r["targets"].astype(np.float64) - r["y"].astype(np.float64)) ** 2
    np.testing.assert_allclose(r["loss"], d.mean(axis=0).sum(), rtol=1e-6)
    # (the fp64 loss merges in fp64: it differs from the fp32 prediction's by the merge's rounding, a few 2^-24 of |y|)
    np.testing.assert_allclose(R.total_loss64(E, X, actions, future.astype(np.float32)), d.mean(axis=0).sum(), rtol=1e-5)


@pytest.mark.parametrize("case", [1, 3])
def test_gradient_equals_central_differences_of_the_loss(golden, case):
    g = golden("dfp")
    p = "learn%d_" % case
    E, X = g[p + "E"].astype(np.float64), g[p + "X"].astype(np.float64)
    actions, future = g[p + "actions"], g[p + "future"].astype(np.float32)
    r = R.head_loss(E, X, actions, future, dtype=np.float64)
    assert r["dE"].dtype == np.float64
    np.testing.assert_allclose(r["loss"], R.total_loss64(E, X, actions, future), rtol=1e-13)
    h = 1e-5
    num_E, num_X = np.zeros_like(E), np.zeros_like(X)
    for idx in np.ndindex(*E.shape):
        hi, lo = E.copy(), E.copy()
        hi[idx] += h
        lo[idx] -= h
        num_E[idx] = (R.total_loss64(hi, X, actions, future) - R.total_loss64(lo, X, actions, future)) / (2 * h)
    for idx in np.ndindex(*X.shape):
        hi, lo = X.copy(), X.copy()
        hi[idx] += h
        lo[idx] -= h
        num_X[idx] = (R.total_loss64(E, hi, actions, future) - R.total_loss64(E, lo, actions, future)) / (2 * h)
    # the loss is quadratic: central differences are exact up to rounding
    np.testing.assert_allclose(r["dE"], num_E, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(r["dX"], num_X, rtol=1e-7, atol=1e-9)
    f32 = R.head_loss(E, X, actions, future)
    np.testing.assert_allclose(f32["dE"], r["dE"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(f32["dX"], r["dX"], rtol=1e-5, atol=1e-7)
    half = R.head_loss(E, X, actions, future, grad_scale=0.5, dtype=np.float64)
    np.testing.assert_allclose(half["dX"], 0.5 * r["dX"], rtol=1e-15)


def test_an_invalid_action_adds_no_term():
    rng = np.random.RandomState(0)
    E, X = rng.randn(3, 4).astype(np.float32), rng.randn(3, 2, 4).astype(np.float32)
    future = rng.randn(3, 4).astype(np.float32)
    ok = R.head_loss(E[[0, 2]], X[[0, 2]], np.array([1, 0]), future[[0, 2]])
    bad = R.head_loss(E, X, np.array([1, 2, 0]), future)
    assert bad["status"] == 1 and ok["status"] == 0 and np.all(bad["dE"][1] == 0) and np.all(bad["dX"][1] == 0)
    # the row count still divides: B = 3
    np.testing.assert_allclose(bad["loss"] * 3, ok["loss"] * 2, rtol=1e-6)


@pytest.mark.parametrize("case", range(len(ACT_CASES)))
def test_action_scores_equal_the_reference(golden, case):
    g = golden("dfp")
    A, M, W = ACT_CASES[case]
    p = "act%d_" % case
    want = g[p + "scores"]
    assert want.dtype == np.float64 and want.shape[1] == A and len(g[p + "weights"]) == W
    _same("scores", R.scores(g[p + "E"], g[p + "X"], g[p + "goal"], g[p + "weights"], ACT_STEPS, M), want)
    top = np.sort(want, axis=1)
    gap = top[:, -1] - top[:, -2]
    tied = gap == 0
    assert tied.sum() == (1 if case == len(ACT_CASES) - 1 else 0) and np.all(gap[~tied] >= 1e-6)


def test_the_tie_is_broken_by_the_draws():
    q = np.array([[1.5, 0.2, 1.5], [1.5, 0.2, 1.5 + 1e-4]])
    tie = np.array([[0.1, 0.9, 0.3], [0.9, 0.99, 0.3]])
    assert R.egreedy(q, np.ones(2), np.zeros(2, int), tie, 0.0).tolist() == [2, 2]
    assert R.egreedy(q, np.ones(2), np.zeros(2, int), tie[:, ::-1].copy(), 0.0).tolist() == [0, 2]
    assert R.egreedy(q, np.zeros(2), np.array([1, 1]), tie, 0.5).tolist() == [1, 1]


def test_merge_is_the_dueling_order_and_keeps_the_action_mean_at_zero():
    import glue_ref
    rng = np.random.RandomState(3)
    v, adv = rng.randn(9).astype(np.float32), (rng.randn(9, 5) * 3).astype(np.float32)
    adv[0] = -0.0
    y = R.merge(v[:, None], adv[:, :, None])
    _same("K = 1", y[:, :, 0], glue_ref.dueling_combine_f32(v, adv))
    E, X = rng.randn(4, 6), rng.randn(4, 3, 6)
    y64 = R.merge(E, X, np.float64)
    np.testing.assert_allclose(y64.mean(axis=1), E, rtol=1e-13, atol=1e-15)


def test_recorded_defaults_are_the_reference_agents(golden):
    import json
    d = json.loads(str(golden("dfp")["defaults"]))
    assert d["num_predicted_steps_ahead"] == 6 and d["goal_vector"] == [1.0, 1.0]
    assert d["future_measurements_weights"] == [0.5, 0.5, 1.0] and d["handling_targets_after_episode_end"] == "NAN"
    assert d["num_consecutive_playing_steps"] == 8 and d["batch_size"] == 64 and d["adam_optimizer_beta1"] == 0.95
    # DFPMemoryParameters sets 20000 transitions BEFORE calling its base class, whose __init__ puts its own defaults back
    # (dfp_agent.py:76-80): the reference runs with a million unless a preset says otherwise
    assert d["memory"] == ["DFPMemoryParameters", "Transitions", 1000000] and d["shared_memory"] is False
    assert d["embedders"] == ["goal", "measurements", "observation"]
    assert set(d["embedder_activations"].values()) == {"leaky_relu"} and d["head"][1] == "leaky_relu"


def test_build_and_binding_carry_the_new_entry_points():
    from coach_amd import _rlx
    mk = open(os.path.join(ROOT, "coach_amd", "csrc", "Makefile")).read()
    assert "dfp" in mk.split("EXACT :=")[1].split("$(foreach")[0].split()
    assert _rlx.ACT["leaky_relu"] == 3 and _rlx.ACT["tanh"] == 2 and _rlx.ABI_VERSION == 11
    protos = _rlx.parse_header()
    for name in ("rlx_dfp_head_loss", "rlx_dfp_egreedy", "rlx_dfp_argmax", "rlx_dfp_future_measurements"):
        assert name in protos, name
    src = open(os.path.join(ROOT, "coach_amd", "csrc", "dfp.hip")).read()
    assert "atomicAdd" not in src and '#include "dfp_merge.hpp"' in src
    # the merge is written once: the kernels call the header's function
    assert len(re.findall(r"rlx::dfp_merge_row\(", src)) == 2 and "mean" not in src.split("namespace {")[1]
    # the GEMM epilogues and the narrow-dense body other files include compile as before: leaky_relu is kernels of its own
    csrc = {f: open(os.path.join(ROOT, "coach_amd", "csrc", f)).read()
            for f in sorted(os.listdir(os.path.join(ROOT, "coach_amd", "csrc"))) if f.endswith((".hip", ".hpp"))}
    gemm = csrc["gemm.hip"]
    assert "d.activation <= 2 && d.deriv_kind >= 0 && d.deriv_kind <= 2" in gemm and "leaky_relu_kernel" in gemm
    # the one definition of the activations carries the leaky branch behind a compile-time parameter that is off by
    # default, and the narrow-dense body alone passes it -- switched on by dense_small.hip alone
    shared = csrc["rlx_device.hpp"]
    assert shared.count("template <bool kLeaky = false>") == 2 == shared.count("if (kLeaky && ")
    assert [f for f, s in csrc.items() if re.search(r"act_(apply|deriv_out)<", s)] == ["dense_small_body.hpp"]
    assert csrc["dense_small_body.hpp"].count("#ifdef RLX_DENSE_SMALL_LEAKY") == 1
    assert [f for f, s in csrc.items() if "RLX_ACT_LEAKY_RELU) return" in s] == ["rlx_device.hpp"]
    assert [f for f, s in csrc.items() if "#define RLX_DENSE_SMALL_LEAKY" in s] == ["dense_small.hip"]
    assert "rlx_leaky_relu" in protos
    # the launches that do not implement leaky_relu still refuse an activation above 2
    for f, n in (("noisy_dense.hip", 2), ("batchnorm.hip", 2), ("conv_fused.hip", 2), ("conv_bwd_fused.hip", 1),
                 ("ppo_fc_fused.hip", 1)):
        text = open(os.path.join(ROOT, "coach_amd", "csrc", f)).read()
        assert len(re.findall(r"activation <= 2", text)) == n and "LEAKY" not in text, f


# ----------------------------------------------------------------------- parameters, preset, import layer, refusals
def _defaults(ap):
    net, alg = ap.network_wrappers['main'], ap.algorithm
    emb = net.input_embedders_parameters
    kind = lambda s: ["Dense"] * len(s) if isinstance(s, list) else s
    return {"num_predicted_steps_ahead": alg.num_predicted_steps_ahead, "goal_vector": alg.goal_vector,
            "future_measurements_weights": alg.future_measurements_weights,
            "use_accumulated_reward_as_measurement": alg.use_accumulated_reward_as_measurement,
            "handling_targets_after_episode_end": alg.handling_targets_after_episode_end.name,
            "scale_measurements_targets": alg.scale_measurements_targets,
            "num_consecutive_playing_steps": alg.num_consecutive_playing_steps.num_steps,
            "batch_size": net.batch_size, "adam_optimizer_beta1": net.adam_optimizer_beta1,
            "async_training": net.async_training, "embedders": sorted(emb),
            "embedder_activations": {k: emb[k].activation_function for k in sorted(emb)},
            "embedder_schemes": {k: kind(emb[k].scheme) for k in sorted(emb)},
            "middleware": ["FCMiddlewareParameters", net.middleware_parameters.scheme,
                           net.middleware_parameters.activation_function],
            "head": [type(net.heads_parameters[0]).__name__, net.heads_parameters[0].activation_function],
            "memory": [type(ap.memory).__name__, ap.memory.max_size[0].name, ap.memory.max_size[1]],
            "shared_memory": ap.memory.shared_memory,
            "classes": [type(alg).__name__, type(ap.exploration).__name__, type(net).__name__]}


def test_parameter_defaults_equal_the_reference(golden):
    import json
    from coach_amd.agents.dfp_agent import DFPAgentParameters, HandlingTargetsAfterEpisodeEnd
    ref = json.loads(str(golden("dfp")["defaults"]))
    mine = _defaults(DFPAgentParameters())
    # two departures, both stated in DFPMemoryParameters: the memory's size is the 20000 the reference assigns (its base
    # class's __init__ overwrites it with a million); the default observation embedder is the vector 'Medium' scheme,
    # because the reference's default (three convolutions + Dense(512)) is an image embedder, which is not served
    assert ref["memory"][2] == 1000000 and mine["memory"][2] == 20000
    assert ref["embedder_schemes"]["observation"] == ["Conv2d", "Conv2d", "Conv2d", "Dense"]
    assert mine["embedder_schemes"]["observation"] == "Medium"
    ref["memory"][2], ref["embedder_schemes"]["observation"] = 20000, "Medium"
    assert mine == ref
    assert [m.name for m in HandlingTargetsAfterEpisodeEnd] == ["LastStep", "NAN"]
    assert [m.value for m in HandlingTargetsAfterEpisodeEnd] == [0, 1]
    assert DFPAgentParameters().path == "coach_amd.agents.dfp_agent:DFPAgent"


def test_reference_module_path_resolves_through_the_import_layer():
    import importlib
    import coach_amd.compat as compat
    compat.install()
    mod = importlib.import_module("rl_coach.agents.dfp_agent")
    import coach_amd.agents.dfp_agent as mine
    assert mod.DFPAgentParameters is mine.DFPAgentParameters and mod.DFPAgent is mine.DFPAgent
    assert mod.HandlingTargetsAfterEpisodeEnd is mine.HandlingTargetsAfterEpisodeEnd
    from rl_coach.architectures.head_parameters import MeasurementsPredictionHeadParameters
    assert isinstance(mine.DFPNetworkParameters().heads_parameters[0], MeasurementsPredictionHeadParameters)
    from coach_amd.architectures.hip_architecture import DFPArchitecture, _family_of
    assert _family_of(mine.DFPNetworkParameters()) is DFPArchitecture


def test_package_preset_equals_the_unchanged_reference_preset_text():
    """tests/golden/dfp_preset.json holds what the reference's CartPole_DFP.py text, executed unchanged through the import
    layer, set (make_dfp_preset_dump.py): the package's preset must equal it field by field."""
    import importlib
    import json
    from coach_amd.agents.dfp_agent import HandlingTargetsAfterEpisodeEnd
    from coach_amd.compat import resolve_reference_style
    from test_cartpole import _dump
    with open(os.path.join(ROOT, "tests", "golden", "dfp_preset.json")) as f:
        ref = json.load(f)["CartPole_DFP"]
    mine = importlib.import_module("coach_amd.presets.CartPole_DFP").make()
    resolve_reference_style(mine.agent_params, mine.env_params)      # what create_graph does first
    for part in ("agent_params", "schedule", "preset_validation_params"):
        assert ref[part] == _dump(getattr(mine, part)), part
    assert ref["level_name"] == "CartPole-v0" == mine.env_params.level
    alg, net = mine.agent_params.algorithm, mine.agent_params.network_wrappers["main"]
    assert alg.handling_targets_after_episode_end is HandlingTargetsAfterEpisodeEnd.LastStep and alg.goal_vector == [1]
    assert net.learning_rate == 0.0001 and set(net.embedder_schemes.values()) == {"Medium"}
    v = mine.preset_validation_params
    assert v.test and v.min_reward_threshold == 120 and v.max_episodes_to_achieve_reward == 250


def test_reference_preset_text_runs_through_the_import_layer():
    from test_preset_dropin import REF, _exec_preset
    path = os.path.join(REF, "CartPole_DFP.py")
    if not os.path.exists(path):
        pytest.skip("the reference tree is not present")
    from coach_amd.agents.dfp_agent import DFPAgent, DFPAgentParameters
    ns = _exec_preset(open(path).read())
    ap = ns["agent_params"]
    assert isinstance(ap, DFPAgentParameters) and ns["graph_manager"].agent_params is ap
    assert ap.network_wrappers["main"].embedder_schemes == {k: "Medium" for k in ("goal", "measurements", "observation")}
    from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
    names, factors, goal, weights = DFPAgent.check_parameters(ap, CartPoleVectorEnvironmentParameters(1))
    assert names == ["accumulated_reward"] and factors.tolist() == [1.0] and goal == [1.0] and weights == [0.5, 0.5, 1.0]


class _Env(object):
    def __init__(self, **p):
        self.p = type("P", (), dict(dict(kind="vector", observation_shape=(4,), num_actions=2, num_envs=1,
                                         episode_length=200), **p))()


def _params(**alg):
    from coach_amd.agents.dfp_agent import DFPAgentParameters
    p = DFPAgentParameters()
    p.algorithm.use_accumulated_reward_as_measurement = True
    p.algorithm.goal_vector = [1.0]
    for k, v in alg.items():
        setattr(p.algorithm, k, v)
    return p


@pytest.mark.parametrize("env,alg,text", [
    (dict(kind="image", observation_shape=(84, 84)), {}, "image observations are not served"),
    (dict(num_actions=None, action_dim=3), {}, "Box action space is not served"),
    ({}, dict(goal_vector=[1.0, 1.0]), "the goal vector"),
    ({}, dict(goal_vector=[]), "the goal vector"),
    ({}, dict(scale_measurements_targets={"health": 2.0}), "are not defined in the measurements space"),
    ({}, dict(use_accumulated_reward_as_measurement=False), "Measurements are not present"),
    (dict(measurements_names=["health"]), {}, "supplied by the environment are not served"),
    ({}, dict(future_measurements_weights=[1.0] * 7), "future_measurements_weights"),
])
def test_agent_refuses_what_it_does_not_serve(env, alg, text):
    """before anything touches the device: the constructor raises on a machine without a GPU as well"""
    from coach_amd.agents.dfp_agent import DFPAgent
    with pytest.raises(ValueError, match=text):
        DFPAgent(_params(**alg), _Env(**env))


def test_agent_refuses_other_memories_and_parameter_noise():
    from coach_amd.agents.dfp_agent import DFPAgent
    from coach_amd.exploration_policies.parameter_noise import ParameterNoiseParameters
    from coach_amd.memories.non_episodic.experience_replay import ExperienceReplayParameters
    p = _params()
    p.memory = ExperienceReplayParameters()
    with pytest.raises(ValueError, match="EpisodicExperienceReplay"):
        DFPAgent(p, _Env())
    p = _params()
    p.memory.shared_memory = True
    with pytest.raises(ValueError, match="shared_memory"):
        DFPAgent(p, _Env())
    with pytest.raises(ValueError, match="only DQN variants"):      # the policy's own refusal, as in the reference
        ParameterNoiseParameters(_params())
    names, factors, goal, weights = DFPAgent.check_parameters(_params(scale_measurements_targets={"accumulated_reward": 3}),
                                                              _Env().p)
    assert names == ["accumulated_reward"] and factors.tolist() == [3.0]


def test_memory_keeps_no_measurement_columns_unless_asked():
    src = open(os.path.join(ROOT, "coach_amd", "memories", "episodic", "episodic_experience_replay.py")).read()
    assert "measurements_dim=None, future_measurements=None" in src
    assert "self.measurements = self.future_measurements = None" in src


def test_accumulated_reward_measurement_lags_one_step():
    r = np.array([1.0, 2.0, 4.0, 8.0], np.float32)
    assert R.accumulated_reward_measurements(r).tolist() == [0.0, 0.0, 1.0, 3.0, 7.0]
    assert R.accumulated_reward_measurements(r[:0]).tolist() == [0.0]
    inexact = np.array([0.1, 0.2, 0.3], np.float32)
    m = R.accumulated_reward_measurements(inexact)
    assert m.dtype == np.float64 and m[3] == float(inexact[0]) + float(inexact[1])
