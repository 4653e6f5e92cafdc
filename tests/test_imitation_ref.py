"""The imitation-learning pieces on the CPU: the numpy restatement (tests/imitation_ref.py) against what the reference's
own BCAgent, ImitationAgent and DDQNBCQAgent (NNImitationModelParameters) computed (tests/golden/imitation.npz,
make_golden_imitation.py), bit for bit; the restated cross entropy against fp64; the C ABI entries; the parameter
classes' defaults and every refusal that is raised before the device is touched."""
import json
import os

import numpy as np
import pytest

import imitation_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name -> (B, A, probabilities mode, zero-confidence rows placed by hand)
CASES = {"n0": (1, 2, False, 0), "n1": (5, 3, False, 2), "n2": (37, 18, False, 0), "n3": (128, 3, False, 2),
         "p": (5, 3, True, 2)}
THRESHOLD = 0.35


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "imitation.npz"))


def case(gold, name):
    return {k[len(name) + 1:]: gold[k] for k in gold.files if k.startswith(name + "_")}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ select_actions
@pytest.mark.parametrize("name", sorted(CASES))
def test_select_actions_equals_the_reference_agent(gold, name):
    c = case(gold, name)
    B, A, probs_in, placed = CASES[name]
    assert c["q_sel"].shape == c["imitation"].shape == (B, A) and c["q_sel"].dtype == c["imitation"].dtype == np.float32
    print("%s: %d rows redrawn" % (name, int(c["redrawn"])))
    assert int(c["redrawn"]) <= 0.05 * B
    sel, fam, mask, zero = R.imitation_selector(c["q_sel"], c["imitation"], THRESHOLD, probs_in=probs_in, seed=3, rank=1,
                                                event=5)
    assert fam.dtype == np.float32 and np.array_equal(bits(fam), bits(c["familiarity"]))
    assert np.array_equal(mask | zero[:, None], c["mask"]) and np.array_equal(zero, c["zero_rows"])
    assert int(zero[:2].sum()) == placed if A == 3 else True
    live = ~zero
    assert np.array_equal(np.argmax(sel, axis=1)[live], c["selected"][live])
    assert ((sel[zero] >= 0) & (sel[zero] < 1)).all()                        # the reference's np.random.rand rows
    assert np.array_equal(bits(sel[live][~mask[live]]), bits(c["q_sel"][live][~mask[live]]))
    assert np.isneginf(sel[live][mask[live]]).all()


def test_the_golden_cases_hold_what_they_are_meant_to_hold(gold):
    thr32 = np.float32(THRESHOLD)
    for name, (B, A, probs_in, placed) in CASES.items():
        c = case(gold, name)
        exempt = ({0, 1, 2, 3} if probs_in else {0, 1}) if A == 3 else set()
        fam = c["familiarity"].astype(np.float64)
        for b in range(B):
            if b in exempt:
                continue
            assert not (np.abs(fam[b] - THRESHOLD) <= 1e-6 * THRESHOLD).any()
            if not c["zero_rows"][b]:
                v = np.sort(c["q_sel"][b][~c["mask"][b]])
                assert len(v) >= 1 and (len(v) == 1 or v[-1] - v[-2] >= 1e-6)
        if A == 3:                                                           # every probability below the threshold
            assert c["zero_rows"][:2].all() and (c["familiarity"][:2] < thr32).all()
    p = case(gold, "p")
    # exactly np.float32(0.35): NOT masked (an fp64 comparison would mask it); the next fp32 below it: masked
    assert bits(p["imitation"][2, 0]) == bits(thr32) and not p["mask"][2, 0]
    assert float(p["imitation"][2, 0]) < THRESHOLD and not (p["imitation"][2:3, 0] < THRESHOLD)[0]
    assert bits(p["imitation"][3, 0]) == bits(np.nextafter(thr32, np.float32(0))) and p["mask"][3, 0]
    n2 = case(gold, "n2")
    assert n2["mask"].any() and not n2["mask"].all()


def test_nan_familiarity_is_not_masked_and_probabilities_mode_passes_them_through():
    q = np.array([[1, 2, 3]], dtype=np.float32)
    p = np.array([[np.nan, 0.1, 0.9]], dtype=np.float32)
    sel, fam, mask, zero = R.imitation_selector(q, p, THRESHOLD, probs_in=True)
    assert mask.tolist() == [[False, True, False]] and sel[0, 0] == 1 and np.isneginf(sel[0, 1]) and not zero.any()
    assert np.array_equal(bits(fam), bits(p))


# ------------------------------------------------------------------------------------------- improve_reward_model
@pytest.mark.parametrize("i", [0, 1])
def test_epoch_interleaving_equals_the_reference(gold, i):
    p = "sched%d_" % i
    epochs, im_epochs = int(gold[p + "epochs"]), int(gold[p + "imitation_epochs"])
    firsts = gold["sched_batch_firsts"].tolist()
    want = R.reward_model_schedule(epochs, im_epochs, len(firsts))
    got = [(int(kind), int(first)) for kind, first in gold[p + "log"]]
    assert got == [(0 if kind == "reward_model" else 1, firsts[b]) for _, b, kind in want]
    assert int(gold[p + "generators"]) == max(epochs, im_epochs)             # ONE generator per epoch
    assert sum(k == "reward_model" for _, _, k in want) == epochs * 3
    assert sum(k == "imitation_model" for _, _, k in want) == im_epochs * 3
    # the one-hot targets of every imitation update
    actions, sizes = gold["sched_actions"], gold["sched_batch_sizes"].tolist()
    rows = [R.one_hot(actions[f:f + n], 3) for _, b, k in want if k == "imitation_model" for f, n in [(firsts[b], sizes[b])]]
    assert np.array_equal(np.concatenate(rows), gold[p + "targets"]) and str(gold[p + "target_dtype"]) == "float64"


# ------------------------------------------------------------------------------------------------------- BC, acting
def test_bc_learn_from_batch_hands_the_network_actions_and_ones(gold):
    assert np.array_equal(gold["bc_observation"], gold["bc_states"])
    assert np.array_equal(gold["bc_output_0_0"], gold["bc_actions"])
    assert np.array_equal(gold["bc_targets"], np.ones(5)) and gold["bc_targets"].dtype == np.float64


def test_choose_action_is_egreedy_in_the_forced_test_phase(gold):
    """ImitationAgent.choose_action: the policy is put into TEST at every call, so evaluation_epsilon (0.25) applies although
    the agent trains; the schedule's 1.0 would explore at every step.  The decisions are replayed on numpy's stream."""
    probs, eps = gold["act_probs"], float(gold["act_evaluation_epsilon"])
    assert gold["act_phase_is_test"].all() and float(gold["act_schedule_value"]) == 1.0
    np.random.seed(4)
    current = np.random.rand()                                               # EGreedy.__init__
    actions, explored = [], 0
    for p in probs:
        if current < eps:
            a = np.random.choice(list(range(len(p))))
            explored += 1
        else:
            a = np.argmax(np.random.random(p.shape) * np.isclose(p, p.max()))
        current = np.random.rand()
        actions.append(int(a))
    assert actions == gold["act_actions"].tolist()
    assert 0 < explored < len(probs)                                         # not the schedule's epsilon of 1
    assert str(gold["imitation_error"]) == "ImitationAgent is an abstract agent. Not to be used directly."
    assert bool(gold["imitation_flag"])


# --------------------------------------------------------------------------------------- the restated cross entropy
def _rows(rng, B, A, scale):
    return (rng.randn(B, A) * scale).astype(np.float32)


@pytest.mark.parametrize("A", [1, 2, 3, 18])
@pytest.mark.parametrize("scale", [1e-3, 1.0, 30.0])
def test_restated_cross_entropy_is_within_its_rounding_bound_of_fp64(A, scale):
    """Per row, u = 2^-24 (fp32 unit roundoff), t_j = z_j - mx, T = max |t_j|:
      t_j: one rounding, |dt_j| <= u |t_j|;  e_j = exp(t_j): the rounding of t_j moves it by <= u |t_j| relatively, its own
      rounding by u;  s: A - 1 additions of positive terms, each u relatively, on terms that are off by <= u (T + 1):
      |ds / s| <= u (T + A);  log s: |d| <= u (T + A) + u |log s|;  log p_j = t_j - log s: one more rounding, u |log p_j|.
      So |d log p_j| <= u (|t_j| + T + A + |log s| + |log p_j|).  The loss: A products l_j log p_j (u each) and A - 1
      additions (each u on a partial sum of magnitude <= sum |l_k log p_k|): u A sum |l_j log p_j| more.
    The factor 1.01 covers the second-order terms (u^2).  Nothing here was fitted to what the restatement gives."""
    rng = np.random.RandomState(int(1000 * scale) + A)
    B = 257
    x = _rows(rng, B, A, scale)
    hot = R.one_hot(rng.randint(0, A, size=B), A).astype(np.float32)
    soft = rng.rand(B, A).astype(np.float32) * np.float32(2)
    u = 2.0 ** -24
    for labels in (hot, soft):
        r = R.classification_head_loss(x, labels=labels)
        want = R.cross_entropy_f64(x, labels)
        x64 = x.astype(np.float64)
        t = x64 - x64.max(axis=1, keepdims=True)
        logs = np.log(np.exp(t).sum(axis=1, keepdims=True))
        logp = t - logs
        l = np.abs(labels.astype(np.float64))
        T = np.abs(t).max(axis=1, keepdims=True)
        bound = 1.01 * u * ((l * (np.abs(t) + T + A + np.abs(logs) + np.abs(logp))).sum(axis=1)
                            + A * (l * np.abs(logp)).sum(axis=1))
        err = np.abs(r["row_loss"].astype(np.float64) - want)
        print("A=%d scale=%g: max error %.3g, max of error / bound %.3g" % (A, scale, err.max(),
                                                                            (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
        # the gradient and the probabilities against fp64 (same counting: p_j = e_j / s, <= u (|t_j| + T + A + 2) relatively)
        p64 = np.exp(logp)
        perr = np.abs(r["probs"].astype(np.float64) - p64)
        # (+ 2^-149, the spacing of fp32's subnormals: a p_j below 2^-126 has no relative accuracy in the format)
        assert (perr <= 1.01 * u * p64 * (np.abs(t) + T + A + 2) + 2.0 ** -149).all()
    acts = np.argmax(hot, axis=1)
    a, b = R.classification_head_loss(x, actions=acts), R.classification_head_loss(x, labels=hot)
    for k in ("row_loss", "dlogits", "probs"):
        assert np.array_equal(bits(a[k]), bits(b[k]))
    assert bits(a["loss_sum"]) == bits(b["loss_sum"]) and a["correct"] == b["correct"]


def test_restatement_edges():
    x = np.array([[1e4, 0, -1e4], [5, 5, 5], [0, 1e-3, 0]], dtype=np.float32)
    r = R.classification_head_loss(x, actions=[0, 3, -1], grad_scale=0.5)
    assert r["status"] == 1 and r["probs"][0].tolist() == [1.0, 0.0, 0.0] and r["row_loss"].tolist() == [0.0, 0.0, 0.0]
    assert (r["dlogits"][1:] == 0).all() and r["correct"] == 1 and np.isfinite(r["logp"]).all()
    r = R.classification_head_loss(x, actions=[2, 1, 1])
    assert r["row_loss"][0] == np.float32(2e4) and r["loss_sum"] == R.tree_sum(r["row_loss"])
    one = R.classification_head_loss(np.array([[3.0], [-2.0]], dtype=np.float32), actions=[0, 0])
    assert (one["dlogits"] == 0).all() and (one["row_loss"] == 0).all() and one["correct"] == 2
    # the tree: the additions of a workgroup of max(64, next power of two) threads, not numpy's pairwise sum
    v = (np.random.RandomState(0).rand(1000) * 7).astype(np.float32)
    w = np.zeros(1024, dtype=np.float32)
    w[:1000] = v
    while w.size > 1:
        w = w[:w.size // 2] + w[w.size // 2:]
    assert bits(R.tree_sum(v)) == bits(w[0]) and R.tree_sum(v[:1]) == v[0] and R.tree_sum(v[:65]).dtype == np.float32


# ------------------------------------------------------------------------------------------------------------ ABI
def test_abi_entries_are_declared_and_bound():
    from coach_amd import _rlx
    protos = _rlx.parse_header()
    assert [n for _, n in protos["rlx_classification_head_loss"][1]] == [
        "logits", "ld", "actions", "labels", "ld_labels", "grad_scale", "rows", "n_actions", "dlogits", "ld_dlogits",
        "probs_out", "ld_probs", "row_loss_out", "scalars", "status", "stream"]
    assert [n for _, n in protos["rlx_bcq_imitation_selector"][1]] == [
        "q_next_online", "ld_q", "imitation", "ld_i", "threshold", "flags", "batch", "n_actions", "seed", "rank", "event",
        "sel_out", "ld_sel", "familiarity_out", "ld_f", "zero_rows_out", "stream"]
    import ctypes
    assert protos["rlx_bcq_imitation_selector"][1][4][0] is ctypes.c_float          # the fp32 threshold
    assert _rlx.CONSTANTS["RLX_IMITATION_INPUT_PROBS"] == R.INPUT_PROBS == 1 and _rlx.ABI_VERSION == 11
    lib = _rlx.lib()
    assert lib.raw("rlx_classification_head_loss") and lib.raw("rlx_bcq_imitation_selector")


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """null pointers, bad sizes, both or neither of actions / labels, a leading dimension below n_actions: refused on the
    host (the pointers are never dereferenced there, so any non-null value stands for a buffer)"""
    from coach_amd import _rlx
    lib, P = _rlx.lib(), 4096
    call = lambda x=P, ld=4, a=P, l=None, ld_l=4, B=8, A=4, d=P, ld_d=4, p=None, ld_p=4, s=P, st=P: \
        lib.classification_head_loss(x, ld, a, l, ld_l, 1.0, B, A, d, ld_d, p, ld_p, None, s, st, None)
    for kw, text in ((dict(x=None), "null pointer"), (dict(d=None), "null pointer"), (dict(s=None), "null pointer"),
                     (dict(st=None), "null pointer"), (dict(a=None), "neither"), (dict(l=P), "both"),
                     (dict(B=0), "bad sizes"), (dict(B=1025), "bad sizes"), (dict(A=0), "bad sizes"),
                     (dict(A=19, ld=19, ld_d=19), "bad sizes"), (dict(ld=3), "leading dimension"),
                     (dict(ld_d=3), "leading dimension"), (dict(a=None, l=P, ld_l=3), "leading dimension"),
                     (dict(p=P, ld_p=3), "leading dimension")):
        with pytest.raises(_rlx.RlxError, match="rlx_classification_head_loss.*" + text):
            call(**kw)
    call = lambda q=P, ld_q=4, i=P, ld_i=4, flags=0, B=8, A=4, e=P, s=P, ld_s=4, f=None, ld_f=4: \
        lib.bcq_imitation_selector(q, ld_q, i, ld_i, 0.35, flags, B, A, 0, 0, e, s, ld_s, f, ld_f, None, None)
    for kw, text in ((dict(q=None), "null pointer"), (dict(i=None), "null pointer"), (dict(e=None), "null pointer"),
                     (dict(s=None), "null pointer"), (dict(flags=2), "unknown flags"), (dict(B=0), "bad sizes"),
                     (dict(B=1025), "bad sizes"), (dict(A=0), "bad sizes"), (dict(A=19, ld_q=19, ld_i=19, ld_s=19), "bad sizes"),
                     (dict(ld_q=3), "leading dimension"), (dict(ld_i=3), "leading dimension"),
                     (dict(ld_s=3), "leading dimension"), (dict(f=P, ld_f=3), "leading dimension")):
        with pytest.raises(_rlx.RlxError, match="rlx_bcq_imitation_selector.*" + text):
            call(**kw)


# ----------------------------------------------------------------------------- parameters, presets and refusals
def test_parameter_defaults_equal_the_reference(gold):
    from coach_amd.agents.ddqn_bcq_agent import NNImitationModelParameters
    from coach_amd.architectures.head_parameters import ClassificationHeadParameters
    d = json.loads(str(gold["defaults"]))
    assert dict(vars(NNImitationModelParameters())) == d["nn_imitation"] == {
        "imitation_model_num_epochs": 100, "mask_out_actions_threshold": 0.35}
    head, want = ClassificationHeadParameters(), d["classification_head"]
    assert head.head_type == want["parameterized_class_name"] == "ClassificationHead"
    for k in ("name", "activation_function", "loss_weight", "rescale_gradient_from_head_by_factor"):
        assert getattr(head, k) == want[k], k


def _bcq_params(nn=True, wrapper=True):
    from coach_amd.presets.CartPole_DDQN_BCQ_BatchRL import make
    ap = make(action_drop="nn" if nn else "knn").agent_params
    ap.is_batch_rl_training = True
    if not wrapper:
        ap.network_wrappers.pop('imitation_model', None)
    return ap


class _Env(object):
    def __init__(self, kind="vector"):
        from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
        self.p = CartPoleVectorEnvironmentParameters(1)
        self.p.kind = kind


def test_the_batch_rl_preset_takes_an_action_drop_method():
    from coach_amd.agents.ddqn_bcq_agent import KNNParameters, NNImitationModelParameters, imitation_model_wrapper
    from coach_amd.nn.networks import classification_net_kwargs
    from coach_amd.presets.CartPole_DDQN_BCQ_BatchRL import graph_manager, make
    assert isinstance(graph_manager.agent_params.algorithm.action_drop_method_parameters, KNNParameters)
    assert 'imitation_model' not in graph_manager.agent_params.network_wrappers      # the default is the experiment as it was
    assert 'imitation_model' not in make().agent_params.network_wrappers
    ap = make(action_drop="nn").agent_params
    assert isinstance(ap.algorithm.action_drop_method_parameters, NNImitationModelParameters)
    w = imitation_model_wrapper(ap)
    assert w is ap.network_wrappers['imitation_model']
    kw = classification_net_kwargs(w, 0)
    assert kw["embedder"] == [1024, 1024, 512, 512, 256] and kw["middleware"] == [128, 64]
    assert kw["learning_rate"] == 0.0001 and kw["l2_regularization"] == 0 and ap.network_wrappers['main'].l2_regularization == 0.0001
    with pytest.raises(ValueError, match='action_drop is "knn" or "nn"'):
        make(action_drop="annoy")
    with pytest.raises(ValueError, match="exactly one ClassificationHeadParameters"):
        classification_net_kwargs(ap.network_wrappers['main'], 0)


def test_bcq_refusals_before_the_device():
    """raised before anything touches the device: they run without one"""
    from copy import deepcopy
    from coach_amd.agents.ddqn_bcq_agent import DDQNBCQAgent, KNNActionMask, NNImitationModelParameters
    with pytest.raises(ValueError, match="^NNImitationModelParameters is not served yet"):
        DDQNBCQAgent(_bcq_params(wrapper=False), _Env())
    ap = _bcq_params()                               # the reference's silent deep copy of the reward model's Q head
    ap.network_wrappers['imitation_model'] = deepcopy(ap.network_wrappers['reward_model'])
    with pytest.raises(ValueError, match="^NNImitationModelParameters is not served yet"):
        DDQNBCQAgent(ap, _Env())
    with pytest.raises(ValueError, match="image observations"):
        DDQNBCQAgent(_bcq_params(), _Env("image"))
    ap = _bcq_params()
    ap.is_batch_rl_training = False
    with pytest.raises(ValueError, match="DDQNBCQ agent can only be used in BatchRL"):
        DDQNBCQAgent(ap, _Env())
    with pytest.raises(ValueError, match="NNImitationModelParameters is not served yet"):
        KNNActionMask(None, 2, NNImitationModelParameters())                 # the kNN mask keeps refusing NN parameters


def test_bc_parameter_defaults_equal_the_reference(gold):
    from coach_amd.agents.bc_agent import BCAgentParameters
    from coach_amd.agents.imitation_agent import ImitationAgent
    d = json.loads(str(gold["defaults"]))
    ap = BCAgentParameters()
    net, alg, sch = ap.network_wrappers["main"], ap.algorithm, ap.exploration.epsilon_schedule
    assert [type(ap).__name__, type(alg).__name__, type(ap.exploration).__name__, type(ap.memory).__name__,
            type(net).__name__] == d["classes"] and ap.path == d["agent_path"] and ap.memory.path == d["memory_path"]
    assert type(net.heads_parameters[0]).__name__ == d["head"] == "PolicyHeadParameters"
    for k in ("optimizer_type", "batch_size", "replace_mse_with_huber_loss", "create_target_network", "learning_rate"):
        assert getattr(net, k) == d[k], k
    assert net.middleware_scheme == "Medium" and "Medium" in d["middleware"][1] and d["embedders"] == ["observation"]
    assert hasattr(alg, "beta_entropy") == d["has_beta_entropy"] is False
    steps = alg.num_consecutive_playing_steps
    assert [type(steps).__name__, steps.num_steps] == d["num_consecutive_playing_steps"]
    assert [type(sch).__name__, float(sch.initial_value), float(sch.final_value), int(sch.decay_steps)] == \
        d["epsilon_schedule"] and ap.exploration.evaluation_epsilon == d["evaluation_epsilon"]
    assert ImitationAgent.imitation is bool(gold["imitation_flag"]) is True and ImitationAgent.is_on_policy is False


def test_bc_refusals_before_the_device(tmp_path):
    from coach_amd.agents.bc_agent import BCAgent, BCAgentParameters
    from coach_amd.core_types import PickledReplayBuffer
    from coach_amd.exploration_policies.parameter_noise import ParameterNoiseParameters
    from coach_amd.presets.CartPole_BC import make

    class Dist(object):
        enabled, rank = True, 0
    with pytest.raises(ValueError, match="image observations"):
        BCAgent(BCAgentParameters(), _Env("image"))
    box = _Env()
    box.p.action_dim = 2
    with pytest.raises(ValueError, match="Box action space"):
        BCAgent(BCAgentParameters(), box)
    with pytest.raises(ValueError, match="data-parallel training is not served by BCAgent"):
        BCAgent(BCAgentParameters(), _Env(), dist=Dist())
    ap = BCAgentParameters()
    with pytest.raises(ValueError, match="only DQN variants are supported for using an exploration type of ParameterNoise"):
        ParameterNoiseParameters(ap)                 # the policy's own refusal, as in the reference
    ap.algorithm.supports_parameter_noise = True     # and past it, the agent's
    ap.exploration = ParameterNoiseParameters(ap)
    with pytest.raises(ValueError, match="ParameterNoise exploration policy .* is not implemented for BCAgent"):
        BCAgent(ap, _Env())
    ap = BCAgentParameters()
    ap.memory.load_memory_from_file_path = PickledReplayBuffer(str(tmp_path / "buffer.p"))
    with pytest.raises(ValueError, match="pickled replay buffer"):
        BCAgent(ap, _Env())
    with pytest.raises(ValueError, match="CartPole_BC trains from a logged dataset"):
        make(None)
    gm = make(str(tmp_path / "x.csv"))
    alg = gm.agent_params.algorithm
    assert alg.num_consecutive_playing_steps.num_steps == 0 and gm.schedule.heatup_steps.num_steps == 0
    assert type(gm.schedule.improve_steps).__name__ == type(gm.schedule.steps_between_evaluation_periods).__name__ == \
        "TrainingSteps" and gm.agent_params.path == "coach_amd.agents.bc_agent:BCAgent"
