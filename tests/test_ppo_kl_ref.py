"""CPU checks of the PPO-penalty restatement tests/ppo_kl_ref.py: its float64 head gradient against central differences
of its own total loss (discrete and continuous, KL regularisation on and off, KL mean below and above the cutoff), the
coefficient update against the reference's lines evaluated literally on numpy scalars, the build's declarations, and
the restatement of the training phase (advantages, value targets, minibatch boundaries, fed inputs, last-epoch means,
coefficient sequences) against tests/golden/ppo_kl.npz, recorded from the reference's own PPOAgent, bit for bit."""
import os
import re

import numpy as np
import pytest

import head_loss_ref as H
import ppo_kl_ref as R

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KLC, HIGH = 0.1, 1000.0
SIDES = ("below", "above", "off")


def _central(f, x, h=1e-6):
    g = np.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.size):
        keep = flat[i]
        flat[i] = keep + h
        up = f(x)
        flat[i] = keep - h
        down = f(x)
        flat[i] = keep
        gf[i] = (up - down) / (2 * h)
    return g


def _close(got, want, f_abs, what, h=1e-6):
    """element by element: a central difference with step h in float64 carries a cancellation error of about
    eps |f| / h (here counted 20-fold: 20 * 2.2e-16 * |f| / h) whatever the component's size, and a truncation error
    h^2 |f'''| / 6, allowed as 1e-6 of the component"""
    bound = 20 * np.finfo(F64).eps * max(1.0, f_abs) / h + 1e-6 * np.abs(want)
    err = np.abs(got - want)
    assert np.all(err <= bound), (what, float((err / bound).max()))


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("B,n", [(1, 1), (3, 2), (7, 6), (5, 18)])
def test_discrete_gradient_is_the_total_loss_gradient(B, n, side):
    case = R.discrete_case(B * 64 + n, B, n)
    use_kl = side != "off"
    cutoff = float(R.cutoff_for(case["kl_mean"], side if use_kl else "below"))
    for beta, gs in ((0.0, 1.0), (0.01, 0.5)):
        ref = R.ppo_kl_discrete_loss(case["logits"], case["actions"], case["advantages"], case["old_probs"], beta, KLC,
                                     cutoff, HIGH, use_kl, gs)
        assert ref["side"] == side
        bt, klc, hi = float(F32(beta)), float(F32(KLC)), float(F32(HIGH))
        z = case["logits"].astype(F64)

        def total(zz):
            return R.discrete_total(zz, case["actions"], case["advantages"].astype(F64), case["old_probs"].astype(F64), bt,
                                    klc, cutoff, hi, use_kl)
        assert abs(total(z) - ref["scalars"][3]) <= 1e-12 * max(1.0, abs(ref["scalars"][3]))
        _close(ref["dlogits"], float(F32(gs)) * _central(total, z), abs(total(z)), "dlogits %s" % side)
        want_c = klc + 2 * hi * max(0.0, ref["scalars"][2] - cutoff) if use_kl else 0.0
        assert ref["scalars"][4] == want_c
        assert np.all(ref["dlogits_units"] >= 0) and np.all(ref["scalars_units"] >= 0)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("B,A", [(1, 1), (4, 3), (6, 17)])
def test_continuous_gradient_is_the_total_loss_gradient(B, A, side):
    case = R.continuous_case(B * 64 + A, B, A)
    use_kl = side != "off"
    cutoff = float(R.cutoff_for(case["kl_mean"], side if use_kl else "below"))
    for beta, gs in ((0.0, 1.0), (0.01, 0.5)):
        ref = R.ppo_kl_continuous_loss(case["mean"], case["log_std"], case["actions"], case["advantages"],
                                       case["old_mean"], case["old_std"], beta, KLC, cutoff, HIGH, use_kl, gs)
        assert ref["side"] == side
        bt, klc, hi = float(F32(beta)), float(F32(KLC)), float(F32(HIGH))
        f64 = {k: case[k].astype(F64) for k in ("mean", "log_std", "actions", "advantages", "old_mean", "old_std")}

        def total(mu=f64["mean"], ls=f64["log_std"]):
            return R.continuous_total(mu, ls, f64["actions"], f64["advantages"], f64["old_mean"], f64["old_std"], bt, klc,
                                      cutoff, hi, use_kl)
        assert abs(total() - ref["scalars"][3]) <= 1e-12 * max(1.0, abs(ref["scalars"][3]))
        _close(ref["dmean"], float(F32(gs)) * _central(lambda m: total(mu=m), f64["mean"].copy()), abs(total()), "dmean %s" % side)
        _close(ref["dlog_std"], float(F32(gs)) * _central(lambda l: total(ls=l), f64["log_std"].copy()), abs(total()),
               "dlog_std %s" % side)


def test_rejected_rows_add_nothing():
    case = R.discrete_case(7, 9, 4)
    a = case["actions"].copy()
    a[2], a[5] = 4, -1
    ref = R.ppo_kl_discrete_loss(case["logits"], a, case["advantages"], case["old_probs"], 0.01, KLC, 0.02, HIGH)
    keep = np.ones(9, dtype=bool)
    keep[[2, 5]] = False
    assert not ref["dlogits"][~keep].any() and not ref["ratio"][~keep].any() and ref["dlogits"][keep].any()
    assert ref["scalars"][2] == ref["kl_rows"][keep].sum() / 9


def test_hinge_cases_are_refused_on_the_hinge():
    case = R.discrete_case(3, 8, 3)
    with pytest.raises(AssertionError, match="hinge"):
        R.ppo_kl_discrete_loss(case["logits"], case["actions"], case["advantages"], case["old_probs"], 0.0, KLC,
                               F32(case["kl_mean"] * 1.05), HIGH)


def _literal_update(total_kl, kl_target, kl_coefficient):
    """ppo_agent.py:335-344 as written, on the types the reference holds (np.float32 scalars and python floats)"""
    new_kl_coefficient = kl_coefficient
    if total_kl > 1.3 * kl_target:
        new_kl_coefficient *= 1.5
    elif total_kl < 0.7 * kl_target:
        new_kl_coefficient /= 1.5
    return new_kl_coefficient


@pytest.mark.parametrize("target", [0.01, 0.02, 0.003, 0.1])
def test_coefficient_update_is_the_reference_lines(target):
    """NEP 50 (numpy >= 2) decides the types of _literal_update's comparisons and products"""
    hi, lo = F32(1.3 * target), F32(0.7 * target)
    up, down = F32(np.inf), F32(-np.inf)
    kls = [hi, np.nextafter(hi, up), np.nextafter(hi, down), lo, np.nextafter(lo, up), np.nextafter(lo, down),
           F32(target), F32(3 * target), F32(0.1 * target), F32(0.0)]
    for coef in (F32(0.1), F32(0.1) * F32(1.5), F32(1.0) / F32(3.0), F32(37.5)):
        for kl in kls:
            for k in (1, 4, 5):
                fetches = [np.array([kl, 1.5], dtype=F32)] * k
                mean = np.mean(fetches, 0)                               # ppo_agent.py:304
                assert mean.dtype == F32
                sums = R.accumulate([[0.0, 1.5, kl, 0.25, 0.0]] * k)     # scalars = sur, ent, KL, total, c
                got_c, got_kl = R.kl_coefficient_update(sums, target, coef)
                want = _literal_update(mean[0], target, coef)
                assert type(want) is F32 and got_c.dtype == F32
                assert got_kl.tobytes() == mean[0].tobytes() and got_c.tobytes() == want.tobytes()


def test_threshold_needs_the_double_target():
    """why rlx_ppo_kl_coefficient_update takes a double: the fp32 threshold of the default target is not reachable from
    the target rounded to fp32"""
    assert F32(1.3 * 0.01) != F32(1.3 * float(F32(0.01)))


def test_declared_and_built():
    header = open(os.path.join(ROOT, "include", "rlx.h")).read()
    for name in ("rlx_ppo_kl_discrete_loss", "rlx_ppo_kl_continuous_loss", "rlx_ppo_kl_coefficient_update"):
        assert re.search(r"\bint %s\(" % name, header), name
    mk = open(os.path.join(ROOT, "coach_amd", "csrc", "Makefile")).read()
    # built like losses.hip (whose ppo_discrete_row it must repeat bit for bit), its own arithmetic uncontracted by pragma
    assert "ppo_kl" not in mk.split("EXACT :=")[1].split("$(foreach")[0].split()
    src = open(os.path.join(ROOT, "coach_amd", "csrc", "ppo_kl.hip")).read()
    assert "ppo_discrete_row(" in src and "atomicAdd" not in src
    assert float(re.search(r"kNoClip = ([0-9.e+]+)f", src).group(1)) == R.NO_CLIP
    assert H.MAX_BLOCK == 1024


# ------------------------------------------------------------------------------------------------ the recorded fixture
@pytest.fixture(scope="module")
def fx(golden):
    return golden("ppo_kl")


def _case(fx, k):
    p = "c%d_" % k
    return {key[len(p):]: fx[key] for key in fx.files if key.startswith(p)}


def test_fixture_covers_the_cases(fx):
    cases = [_case(fx, k) for k in range(int(fx["n_cases"]))]
    assert any(len(c["lengths"]) == 1 for c in cases) and any(len(c["lengths"]) > 2 for c in cases)
    assert any(min(c["num_steps"], c["lengths"].sum()) % c["batch_size"] for c in cases)
    assert any(c["lengths"].sum() > c["num_steps"] for c in cases) and any(c["lengths"].sum() < c["num_steps"] for c in cases)
    assert {int(c["action_kind"]) for c in cases} == {0, 1, 2}
    assert {int(c["action_dim"]) for c in cases if c["action_kind"] == 1} == {1, 3}
    moves = {int(np.sign(float(b) - float(a))) for c in cases for a, b in zip(c["coefficient"][:-1], c["coefficient"][1:])}
    assert moves == {-1, 0, 1}


@pytest.mark.parametrize("k", range(6))
def test_phase_logic_is_the_fixture(fx, k):
    """batch boundaries, fed actions / advantages / value targets with shapes and dtypes, the fp64 advantages before and
    after standardisation: bit for bit what the reference's PPOAgent computed and fed"""
    c = _case(fx, k)
    n = int(c["lengths"].sum())
    raw, adv = R.gae_advantages(c["v"], c["rewards"], c["lengths"], float(c["discount"]), float(c["gae_lambda"]))
    assert raw.dtype == adv.dtype == F64 == np.dtype(str(c["adv_dtype"]))
    assert raw.tobytes() == c["adv_raw"].tobytes() and adv.tobytes() == c["adv"].tobytes()
    bs = int(c["batch_size"])
    vb = R.minibatches(n, c["num_steps"], bs)
    assert np.array_equal(np.array(vb), c["value_batches"])
    pb = R.minibatches(n, c["num_steps"], bs, epochs=10)
    assert np.array_equal(np.array(pb), c["policy_batches"])
    used = vb[-1][1]
    tg = R.value_targets(c["rewards"], c["lengths"], float(c["discount"]))
    assert str(c["value_targets_dtype"]) == "float64" and tuple(c["value_targets_shape"]) == (bs, 1)
    assert tg[:used].tobytes() == c["value_targets"].tobytes()
    assert str(c["fed_advantages_dtype"]) == "float64" and adv[:used].tobytes() == c["fed_advantages"].tobytes()
    if c["action_kind"] == 0:
        assert tuple(c["fed_actions_shape"]) == (bs,) and c["fed_old"] == 1
        assert np.array_equal(c["fed_actions"], c["actions"][:used])
    else:
        A = int(c["action_dim"])
        assert tuple(c["fed_actions_shape"]) == (bs, A) and c["fed_old"] == 2           # scalar actions: expand_dims (:268-269)
        assert np.array_equal(c["fed_actions"], c["actions"][:used].reshape(used, A))


@pytest.mark.parametrize("k", range(6))
def test_coefficient_sequence_is_the_fixture(fx, k):
    """the last epoch's mean KL / entropy and the coefficient after each of the three updates, with their dtypes"""
    c = _case(fx, k)
    assert str(c["kl_mean_dtype"]) == "float32" and str(c["coefficient_dtype"]) == "float32"
    coef = F32(fx["initial_coefficient"])
    assert coef.tobytes() == c["coefficient"][0].tobytes()
    for phase in range(3):
        sums, kl, ent = R.epoch_means(c["kl"][phase], c["entropy"][phase])
        assert kl.tobytes() == c["kl_mean"][phase].tobytes() and ent.tobytes() == c["entropy_mean"][phase].tobytes()
        coef, kl2 = R.kl_coefficient_update(sums, float(c["target_kl"]), coef)
        assert kl2.tobytes() == kl.tobytes() and coef.tobytes() == c["coefficient"][phase + 1].tobytes()


# ------------------------------------------------------------------------------------------------ parameters, preset
def test_parameter_defaults_equal_the_reference(fx):
    """the fixture's `defaults`: the reference's PPOAgentParameters() (ppo_agent.py:40-137), field by field"""
    import json
    from coach_amd.agents.ppo_agent import PPOAgentParameters
    ref = json.loads(str(fx["defaults"]))
    ap = PPOAgentParameters()
    alg = ap.algorithm
    assert [type(alg).__name__, type(ap.network_wrappers["actor"]).__name__, type(ap.network_wrappers["critic"]).__name__,
            type(ap).__name__] == ref["classes"]
    assert list(ap.network_wrappers) == ["critic", "actor"] and ap.path == "coach_amd.agents.ppo_agent:PPOAgent"
    for key in ("policy_gradient_rescaler", "gae_lambda", "target_kl_divergence", "initial_kl_coefficient",
                "high_kl_penalty_coefficient", "clip_likelihood_ratio_using_epsilon", "value_targets_mix_fraction",
                "estimate_state_value_using_gae", "use_kl_regularization", "beta_entropy", "act_for_full_episodes",
                "discount", "num_consecutive_training_steps", "distributed_coach_synchronization_type"):
        mine = getattr(alg, key)
        assert getattr(mine, "name", mine) == ref["algorithm"][key], key
    steps = alg.num_consecutive_playing_steps
    assert "%s:%s" % (type(steps).__name__, steps.num_steps) == ref["algorithm"]["num_consecutive_playing_steps"]
    for name in ("actor", "critic"):
        net, r = ap.network_wrappers[name], ref[name]
        for key in ("learning_rate", "optimizer_type", "batch_size", "async_training", "l2_regularization",
                    "create_target_network", "clip_gradients", "optimizer_epsilon", "adam_optimizer_beta1",
                    "adam_optimizer_beta2", "embedder_scheme", "middleware_scheme"):
            assert getattr(net, key) == r[key], (name, key)
        assert net.activation_function == r["embedder_activation"] == r["middleware_activation"]
        assert [list(h) for h in net.heads] == r["heads"]


def test_package_preset_equals_the_unchanged_reference_preset_text():
    """tests/golden/ppo_kl_preset.json holds what the reference's Mujoco_PPO.py text, executed unchanged through the import
    layer, set (make_ppo_kl_preset_dump.py): the package's preset must equal it field by field."""
    import importlib
    import json
    from coach_amd.compat import resolve_reference_style
    from test_cartpole import _dump
    with open(os.path.join(ROOT, "tests", "golden", "ppo_kl_preset.json")) as f:
        ref = json.load(f)["Mujoco_PPO"]
    mine = importlib.import_module("coach_amd.presets.Mujoco_PPO").make()
    resolve_reference_style(mine.agent_params, mine.env_params)
    assert ref["level_name"] == "InvertedPendulum-v2"
    for part in ("agent_params", "schedule", "preset_validation_params"):
        assert _dump(getattr(mine, part)) == ref[part], part
    alg = mine.agent_params.algorithm
    assert alg.normalize_observations is True and alg.initial_kl_coefficient == 0.2 and alg.gae_lambda == 1.0
    assert mine.agent_params.network_wrappers["actor"].learning_rate == 5e-5
    assert mine.preset_validation_params.min_reward_threshold == 400


def test_reference_preset_text_builds_through_the_import_layer():
    from test_preset_dropin import REF, _exec_preset, _text
    if not os.path.isdir(REF):
        pytest.skip("the reference's preset texts are not on this machine")
    from coach_amd.agents.ppo_agent import PPOAgentParameters
    from coach_amd.compat import resolve_reference_style
    ns = _exec_preset(_text("Mujoco_PPO"))
    gm = ns["graph_manager"]
    assert isinstance(gm.agent_params, PPOAgentParameters)
    resolve_reference_style(gm.agent_params, gm.env_params)
    assert gm.agent_params.algorithm.normalize_observations is True
    assert gm.agent_params.network_wrappers["critic"].middleware_scheme == [64]
    assert gm.schedule.heatup_steps.num_steps == 0 and gm.preset_validation_params.min_reward_threshold == 400


def test_refusals_raise_from_the_parameters_alone():
    """image observations, data-parallel training, a clip range, A_VALUE and the LBFGS critic: a ValueError before
    anything touches the device (check_served runs first in PPOAgent.__init__)"""
    import inspect
    from coach_amd.agents import ppo_agent as M
    from coach_amd.agents.policy_optimization_agent import PolicyGradientRescaler

    class Env(object):
        kind = "vector"

    class Image(object):
        kind = "image"

    class Dist(object):
        enabled = True
    M.check_served(M.PPOAgentParameters(), Env())
    with pytest.raises(ValueError, match="image observations"):
        M.check_served(M.PPOAgentParameters(), Image())
    with pytest.raises(ValueError, match="data-parallel"):
        M.check_served(M.PPOAgentParameters(), Env(), Dist())
    ap = M.PPOAgentParameters()
    ap.algorithm.clip_likelihood_ratio_using_epsilon = 0.2
    with pytest.raises(ValueError, match="ClippedPPOAgent"):
        M.check_served(ap, Env())
    ap = M.PPOAgentParameters()
    ap.algorithm.policy_gradient_rescaler = PolicyGradientRescaler.A_VALUE
    with pytest.raises(ValueError, match="A_VALUE"):
        M.check_served(ap, Env())
    ap = M.PPOAgentParameters()
    ap.network_wrappers["critic"].optimizer_type = 'LBFGS'
    with pytest.raises(ValueError, match="LBFGS"):
        M.check_served(ap, Env())
    body = inspect.getsource(M.PPOAgent.__init__)
    assert body.index("check_served(") < body.index("super().__init__")
