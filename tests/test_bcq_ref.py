"""Batch RL's DDQN-BCQ pieces on the CPU: the numpy restatement (tests/bcq_ref.py) against what the reference's own
EpisodicExperienceReplay, DDQNBCQAgent, DQNAgent and ValueOptimizationAgent computed (tests/golden/bcq.npz,
make_golden_bcq.py), bit for bit; the C ABI entries."""
import os
import random

import numpy as np
import pytest

import bcq_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name -> (B, A, W, keys per action, zero-confidence rows)
CASES = {"s0": (1, 2, 1, [1, 1], 0), "s1": (5, 3, 4, [3, 0, 7], 0), "s1f": (5, 3, 4, [3, 0, 7], 0),
         "s2": (37, 2, 256, [91, 40], 3), "s3": (128, 2, 256, [300, 211], 6)}
MEMORIES = (([200] * 3 + [9, 1, 57], 0.4), ([1] * 10, 0.8), ([13, 200, 200, 45], 0.5))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "bcq.npz"))


def case(gold, name):
    c = {k[len(name) + 1:]: gold[k] for k in gold.files if k.startswith(name + "_")}
    c["keys"], c["set_offsets"] = R.key_sets(c["emb"], c["data_actions"], int(c["n_actions"]))
    return c


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("i", range(len(MEMORIES)))
def test_split_and_shuffled_batches_equal_the_reference_memory(gold, i):
    lengths, ratio = MEMORIES[i]
    p = "mem%d_" % i
    assert gold[p + "lengths"].tolist() == lengths and float(gold[p + "ratio"]) == ratio
    episode_id, transition_id = R.split(lengths, ratio)
    assert (episode_id, transition_id) == (int(gold[p + "episode_id"]), int(gold[p + "transition_id"]))
    assert gold[p + "eval_lengths"].tolist() == lengths[episode_id + 1:]
    assert gold[p + "eval_transitions"].tolist() == list(range(transition_id, sum(lengths)))
    random.seed(7)
    size = int(gold[p + "size"])
    for epoch in range(2):
        batches = R.shuffled_batches(transition_id, size)
        assert [len(b) for b in batches] == gold[p + "epoch%d_sizes" % epoch].tolist()
        assert [j for b in batches for j in b] == gold[p + "epoch%d_flat" % epoch].tolist()
        assert sorted(j for b in batches for j in b) == list(range(transition_id))       # every transition once
    assert len(batches[-1]) == transition_id - size * (len(batches) - 1) and len(batches) == -(-transition_id // size)


def test_split_refusals(gold):
    with pytest.raises(ValueError) as e:
        R.split(MEMORIES[0][0], 1.0)
    assert str(e.value) == str(gold["mem_error_ratio_1"]) == 'train_to_eval_ratio should be in the (0, 1] range.'
    assert str(gold["mem_frozen_error"]) == "Memory is frozen, and cannot be changed."


@pytest.mark.parametrize("name", sorted(CASES))
def test_select_actions_and_targets_equal_the_reference_agent(gold, name):
    c = case(gold, name)
    B, A, W, counts, n_zero = CASES[name]
    assert c["emb_next"].shape == (B, W) and c["q_sel"].shape == (B, A) and c["keys_per_action"].tolist() == counts
    assert np.diff(c["set_offsets"]).tolist() == counts and c["keys"].shape == (sum(counts), W)
    print("%s: %d rows redrawn" % (name, int(c["redrawn"])))
    assert int(c["redrawn"]) <= 0.05 * B
    fam = R.nn_min_distance(c["emb_next"], c["keys"], c["set_offsets"])
    assert fam.dtype == np.float32 and np.array_equal(bits(fam), bits(c["familiarity"]))
    sel, mask, zero = R.masked_selector(c["q_sel"], fam, float(c["threshold"]), seed=3, rank=1, event=5)
    assert np.array_equal(mask, c["mask"]) and np.array_equal(zero, c["zero_rows"]) and int(zero.sum()) == n_zero
    live = ~zero
    chosen = np.argmax(sel, axis=1)
    assert np.array_equal(chosen[live], c["selected"][live])
    assert ((sel[zero] >= 0) & (sel[zero] < 1)).all()                       # the reference's np.random.rand rows
    td = R.td_targets(c["q_online"], c["q_next"], chosen, c["actions"], c["rewards"], c["go"], float(c["discount"]))
    assert td.dtype == np.float32 and np.array_equal(bits(td[live]), bits(c["targets"][live]))
    # the selection is not the unmasked Double-DQN selection everywhere, where something was masked
    if mask[live].any() and name != "s0":
        assert (chosen[live] != np.argmax(c["q_sel"], axis=1)[live]).any()


def test_the_golden_cases_hold_what_they_are_meant_to_hold(gold):
    for name, (B, A, W, counts, n_zero) in CASES.items():
        c = case(gold, name)
        fam, thr = c["familiarity"].astype(np.float64), float(c["threshold"])
        if np.isfinite(thr):
            with np.errstate(invalid="ignore"):
                assert not (np.abs(fam - thr) <= 1e-6 * abs(thr)).any()
        for b in np.nonzero(~c["zero_rows"])[0]:
            v = np.sort(c["q_sel"][b][~c["mask"][b]])
            assert len(v) >= 1 and (len(v) == 1 or v[-1] - v[-2] >= 1e-6)
    assert np.isinf(float(case(gold, "s1")["average_dist"])) and not case(gold, "s1")["mask"].any()
    c = case(gold, "s1f")
    assert c["mask"][:, 1].all() and np.isinf(c["familiarity"][:, 1]).all()       # the action without keys
    for name in ("s2", "s3"):
        c = case(gold, name)
        assert (c["familiarity"] == 0).any()                                       # a next state that is a stored state
        assert c["mask"].any() and not c["mask"].all()


@pytest.mark.parametrize("name", ["s0", "s1", "s2", "s3"])
def test_average_dist_equals_the_reference(gold, name):
    c = case(gold, name)
    dist = R.nn_min_distance(c["emb"], c["keys"], c["set_offsets"])
    own = dist[np.arange(len(dist)), c["data_actions"]]
    assert (own == 0).all()                                                 # every transition is one of its action's keys
    got = R.average_dist(dist)
    assert got == float(c["average_dist"]) or (np.isinf(got) and np.isinf(float(c["average_dist"])))


def test_reward_model_targets_equal_the_reference(gold):
    t = R.reward_model_targets(gold["rm_prediction"], gold["rm_actions"], gold["rm_rewards"])
    assert np.array_equal(bits(t), bits(gold["rm_targets"]))
    other = np.ones(t.shape, bool)
    other[np.arange(len(t)), gold["rm_actions"]] = False
    assert np.array_equal(t[other], gold["rm_prediction"][other])


def test_uniforms_are_a_function_of_key_and_counter():
    u = R.uniforms(7, 3, 3, 1, 5)
    assert u.dtype == np.float32 and ((u >= 0) & (u < 1)).all() and len(np.unique(u)) == 21
    assert np.array_equal(u, R.uniforms(7, 3, 3, 1, 5))
    assert np.array_equal(u[:4, :2], R.uniforms(4, 2, 3, 1, 5))             # u(b, a) does not depend on the batch's shape
    for other in (R.uniforms(7, 3, 3, 1, 6), R.uniforms(7, 3, 4, 1, 5), R.uniforms(7, 3, 3, 0, 5),
                  R.uniforms(7, 3, 3, 1, 5 + (1 << 32))):
        assert not np.array_equal(u, other)


def test_identical_vectors_give_exactly_zero_and_an_empty_set_inf():
    rng = np.random.RandomState(0)
    k = (rng.randn(9, 33) * 100).astype(np.float32)
    d = R.nn_min_distance(k[[4, 8]], k, [0, 9, 9])
    assert d[:, 0].tolist() == [0.0, 0.0] and np.isinf(d[:, 1]).all() and not np.signbit(d[:, 0]).any()


def test_abi_entries_are_declared():
    from coach_amd import _rlx
    protos = _rlx.parse_header()
    assert [n for _, n in protos["rlx_nn_min_distance"][1]] == [
        "queries", "ld_q", "n_queries", "width", "keys", "ld_k", "n_keys", "set_offsets", "n_sets", "dist_out", "ld_out",
        "stream"]
    assert [n for _, n in protos["rlx_bcq_masked_selector"][1]] == [
        "q_next_online", "ld_q", "familiarity", "ld_f", "threshold", "batch", "n_actions", "seed", "rank", "event",
        "sel_out", "ld_sel", "zero_rows_out", "stream"]
    assert "rlx_reward_model_targets" in protos and _rlx.CONSTANTS["RLX_NN_KEY_CHUNK"] == 128


def test_parameter_defaults_equal_the_reference(gold):
    import json
    from coach_amd.agents.ddqn_bcq_agent import DDQNBCQAlgorithmParameters, KNNParameters, NNImitationModelParameters
    d = json.loads(str(gold["defaults"]))
    assert dict(vars(KNNParameters())) == d["knn"] and dict(vars(NNImitationModelParameters())) == d["nn_imitation"]
    alg = DDQNBCQAlgorithmParameters()
    assert type(alg.action_drop_method_parameters).__name__ == d["action_drop_method"] == "KNNParameters"
    steps = alg.num_steps_between_copying_online_weights_to_target
    assert [type(steps).__name__, steps.num_steps] == d["num_steps_between_copying_online_weights_to_target"]
    steps = alg.num_consecutive_playing_steps
    assert [type(steps).__name__, steps.num_steps] == d["num_consecutive_playing_steps"]
    assert alg.discount == d["discount"] and type(alg).__name__ == d["classes"][1]


def test_memory_parameters_keep_the_reference_ratio():
    from coach_amd.memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters
    assert EpisodicExperienceReplayParameters().train_to_eval_ratio == 1


def test_agent_parameters_and_refusals_before_the_device():
    """every refusal of DDQNBCQAgent is raised before anything touches the device: they run without one"""
    import json
    from coach_amd.agents.ddqn_bcq_agent import DDQNBCQAgent, DDQNBCQAgentParameters, NNImitationModelParameters
    from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
    from coach_amd.exploration_policies.parameter_noise import ParameterNoiseParameters
    from coach_amd.memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters
    d = json.loads(str(np.load(os.path.join(GOLDEN, "bcq.npz"))["defaults"]))
    ap = DDQNBCQAgentParameters()
    sch = ap.exploration.epsilon_schedule
    assert [type(ap).__name__, type(ap.algorithm).__name__, type(ap.exploration).__name__, type(ap.memory).__name__] \
        == d["classes"] and ap.path == d["agent_path"] and ap.memory.path == d["memory_path"]
    assert [type(sch).__name__, float(sch.initial_value), float(sch.final_value), int(sch.decay_steps)] == \
        d["epsilon_schedule"] and ap.exploration.evaluation_epsilon == d["evaluation_epsilon"]

    class Env(object):
        def __init__(self, kind="vector"):
            self.p = CartPoleVectorEnvironmentParameters(1)
            self.p.kind = kind

    def params(batch_rl=True):
        ap = DDQNBCQAgentParameters()
        ap.memory = EpisodicExperienceReplayParameters()
        ap.is_batch_rl_training = batch_rl
        return ap
    with pytest.raises(ValueError, match="DDQNBCQ agent can only be used in BatchRL"):
        DDQNBCQAgent(params(False), Env())
    ap = params()
    ap.algorithm.action_drop_method_parameters = NNImitationModelParameters()
    with pytest.raises(ValueError, match="NNImitationModelParameters is not served yet"):
        DDQNBCQAgent(ap, Env())
    with pytest.raises(ValueError, match="image observations"):
        DDQNBCQAgent(params(), Env("image"))
    ap = DDQNBCQAgentParameters()
    ap.is_batch_rl_training = True
    with pytest.raises(ValueError, match="frozen episodic dataset"):
        DDQNBCQAgent(ap, Env())
    ap = params()
    ap.exploration = ParameterNoiseParameters(ap)
    with pytest.raises(ValueError, match="ParameterNoise"):
        DDQNBCQAgent(ap, Env())


def test_batch_rl_graph_manager_keeps_the_reference_signature_and_preset():
    import inspect
    from coach_amd.graph_managers.batch_rl_graph_manager import BatchRLGraphManager
    from coach_amd.presets.CartPole_DDQN_BCQ_BatchRL import graph_manager as gm
    names = list(inspect.signature(BatchRLGraphManager.__init__).parameters)[1:12]
    assert names == ["agent_params", "env_params", "schedule_params", "vis_params", "preset_validation_params", "name",
                     "spaces_definition", "reward_model_num_epochs", "train_to_eval_ratio",
                     "experience_generating_agent_params", "experience_generating_schedule_params"]
    assert gm.reward_model_num_epochs == 30 and gm.experience_generating_agent_params.memory.train_to_eval_ratio == 0.4
    assert gm.agent_params.network_wrappers["main"].l2_regularization == 0.0001
    assert gm.agent_params.network_wrappers["reward_model"].l2_regularization == 0
    assert gm.preset_validation_params.min_reward_threshold == 150


# ------------------------------------------------------------------- the reference's preset text and the import layer
PRESET = "CartPole_DDQN_BCQ_BatchRL"


def _preset_dump(gm):
    import sys
    sys.path.insert(0, GOLDEN)
    try:
        from make_bcq_preset_dump import dump_manager
    finally:
        sys.path.remove(GOLDEN)
    import json
    return json.loads(json.dumps(dump_manager(gm), sort_keys=True))


def reference_equivalent_manager(**kw):
    """the native preset's graph manager plus what the reference's preset text sets on top of it and this engine does
    not use: the imitation model's wrapper (a ClassificationHead on schemes of its own) and softmax_temperature"""
    from copy import deepcopy
    from coach_amd.architectures.head_parameters import ClassificationHeadParameters
    from coach_amd.architectures.layers import Dense
    from coach_amd.presets.CartPole_DDQN_BCQ_BatchRL import make
    gm = make(**kw)
    w = gm.agent_params.network_wrappers
    w['main'].softmax_temperature = 0.2
    w['reward_model'].softmax_temperature = 0.2
    im = w['imitation_model'] = deepcopy(w['main'])
    im.learning_rate, im.l2_regularization = 0.0001, 0
    im.heads_parameters = [ClassificationHeadParameters()]
    im.input_embedders_parameters['observation'].scheme = [Dense(1024), Dense(1024), Dense(512), Dense(512), Dense(256)]
    im.middleware_parameters.scheme = [Dense(128), Dense(64)]
    return gm


def _recorded_preset():
    import json
    with open(os.path.join(GOLDEN, "bcq_preset.json")) as f:
        return json.load(f)[PRESET]


def test_native_preset_equals_the_reference_presets_dump():
    want = _recorded_preset()
    assert _preset_dump(reference_equivalent_manager()) == want
    # and the native preset alone differs from it in exactly those additions
    got = _preset_dump(__import__("coach_amd.presets." + PRESET, fromlist=["make"]).make())
    wrappers = want["agent_params"]["network_wrappers"]
    assert wrappers.pop("imitation_model")["heads_parameters"][0]["__class__"] == "ClassificationHeadParameters"
    assert wrappers["main"].pop("softmax_temperature") == wrappers["reward_model"].pop("softmax_temperature") == 0.2
    assert got == want
    assert want["visualization_parameters"]["dump_signals_to_csv_every_x_episodes"] == 1
    assert want["preset_validation_params"]["read_csv_tries"] == 500 and want["reward_model_num_epochs"] == 30


def test_reference_preset_text_builds_through_the_import_layer():
    from test_preset_dropin import REF, _exec_preset
    if not os.path.isdir(REF):
        pytest.skip("the reference tree is not present")
    from coach_amd.graph_managers.batch_rl_graph_manager import BatchRLGraphManager
    ns = _exec_preset(open(os.path.join(REF, PRESET + ".py")).read())
    gm = ns["graph_manager"]
    assert isinstance(gm, BatchRLGraphManager) and gm.agent_params is ns["agent_params"]
    assert gm.experience_generating_agent_params is ns["experience_generating_agent_params"]
    assert type(gm.agent_params).__module__ == "coach_amd.agents.ddqn_bcq_agent"
    assert _preset_dump(gm) == _recorded_preset()


def test_import_layer_serves_what_the_preset_names():
    import importlib
    import coach_amd.compat as compat
    compat.install()
    layers = importlib.import_module("rl_coach.architectures.tensorflow_components.layers")
    assert layers is importlib.import_module("coach_amd.architectures.layers") and hasattr(layers, "Dense")
    ep = importlib.import_module("rl_coach.memories.episodic")
    from coach_amd.memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters
    assert ep.EpisodicExperienceReplayParameters is EpisodicExperienceReplayParameters
    heads = importlib.import_module("rl_coach.architectures.head_parameters")
    assert heads.ClassificationHeadParameters().head_type == "ClassificationHead"
    base = importlib.import_module("rl_coach.base_parameters")
    assert base.VisualizationParameters(dump_signals_to_csv_every_x_episodes=1).dump_signals_to_csv_every_x_episodes == 1
    assert base.PresetValidationParameters().read_csv_tries == 200
    bcq = importlib.import_module("rl_coach.agents.ddqn_bcq_agent")
    assert bcq.DDQNBCQAgentParameters().path == "coach_amd.agents.ddqn_bcq_agent:DDQNBCQAgent"
    assert importlib.import_module("rl_coach.graph_managers.batch_rl_graph_manager").BatchRLGraphManager
