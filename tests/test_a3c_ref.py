"""Actor-Critic (A3C) on the CPU: the numpy restatement (tests/a3c_ref.py) against what the reference's own
ActorCriticAgent.learn_from_batch computed (tests/golden/a3c.npz, make_golden_a3c.py), the two heads' gradients against
central differences of their own fp64 loss (what stands in for TensorFlow, which cannot run here), the package's
parameter defaults and CartPole_A3C preset against the reference's (tests/golden/a3c_preset.json), and what the agent
refuses."""
import importlib
import json
import os

import numpy as np
import pytest

import a3c_ref as R
import pg_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BITS64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
BITS32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def fixture_case(z, k):
    p = "c%d_" % k
    keys = ("rewards", "actions", "v", "boot", "targets", "advantages", "fed_actions", "values_signal",
            "advantages_signal")
    return dict({n: z[p + n] for n in keys}, game_over=bool(z[p + "game_over"]), discount=float(z[p + "discount"]),
                gae_lambda=float(z[p + "gae_lambda"]), estimate_gae=bool(z[p + "estimate_gae"]),
                rescaler=int(z[p + "rescaler"]), targets_dtype=str(z[p + "targets_dtype"]),
                advantages_dtype=str(z[p + "advantages_dtype"]))


def restated(c):
    return R.window_targets(c["v"], c["boot"][0, 0], c["rewards"], c["game_over"], c["discount"], c["gae_lambda"],
                            c["rescaler"], c["estimate_gae"])


@pytest.fixture(scope="module")
def a3c():
    return np.load(os.path.join(GOLDEN, "a3c.npz"))


def test_fixture_holds_the_cases_the_issue_names(a3c):
    cs = [fixture_case(a3c, k) for k in range(int(a3c["n_cases"]))]
    seen = {(c["rescaler"], c["game_over"], c["rewards"].size) for c in cs}
    assert seen == {(r, g, T) for r in (R.A_VALUE, R.GAE) for g in (False, True) for T in (1, 2, 5, 200)}
    gae = [c for c in cs if c["rescaler"] == R.GAE]
    assert {(c["gae_lambda"], c["estimate_gae"]) for c in gae} == {(1.0, False), (1.0, True), (0.96, False), (0.96, True)}
    assert {c["discount"] for c in cs} == {0.99, 1.0}
    scale = np.float32(1 / 200.)
    assert a3c["reward_scale"] == scale
    assert any(np.all(c["rewards"] == np.float32(1.0) * scale) for c in cs)       # the preset's filtered reward
    assert any(len(set(c["rewards"].tolist())) > 1 for c in cs)
    assert all(c["rewards"].dtype == np.float32 and c["v"].dtype == np.float32 for c in cs)
    assert str(a3c["numpy_version"]) and str(a3c["scipy_version"])


def test_targets_and_advantages_equal_the_reference_agent_bit_for_bit(a3c):
    """every golden case, in fp64 before the placeholder cast and in fp32 after it.  The types of some of the reference's
    intermediates follow numpy's promotion rule (a3c_ref's module text names the lines); the fixture was recorded with
    the numpy it names (2.x: NEP 50), and the restatement restates that rule whatever numpy runs this test."""
    assert int(str(a3c["numpy_version"]).split(".")[0]) >= 2, "the fixture must come from a numpy with NEP 50 promotion"
    for k in range(int(a3c["n_cases"])):
        c = fixture_case(a3c, k)
        w = restated(c)
        assert c["targets_dtype"] == "float64" and c["advantages_dtype"] == "float64", k
        assert w["targets"].dtype == np.float64 and w["advantages"].dtype == np.float64
        assert np.array_equal(BITS64(w["targets"]), BITS64(c["targets"])), k
        assert np.array_equal(BITS64(w["advantages"]), BITS64(c["advantages"])), k
        assert np.array_equal(BITS32(w["targets32"]), BITS32(c["targets"].astype(np.float32))), k
        assert np.array_equal(BITS32(w["advantages32"]), BITS32(c["advantages"].astype(np.float32))), k
        # the signals' samples: 'Values' is the V head's output on the window, 'Advantages' what the policy head was fed
        assert np.array_equal(BITS32(c["values_signal"].reshape(-1)), BITS32(c["v"].reshape(-1)))
        assert np.array_equal(BITS64(c["advantages_signal"].reshape(-1)), BITS64(w["advantages"]))
        assert np.array_equal(c["fed_actions"], c["actions"])


def test_the_fp32_product_of_the_first_pass_shows_in_the_fixture(a3c):
    """the promotion-dependent lines matter: with every product in fp64 some bootstrapped case differs"""
    differs = 0
    for k in range(int(a3c["n_cases"])):
        c = fixture_case(a3c, k)
        if c["game_over"] or c["rescaler"] != R.A_VALUE:
            continue
        V = c["v"].reshape(-1).astype(np.float64)
        Rv = float(c["boot"][0, 0])
        t = np.empty(V.size)
        for i in reversed(range(V.size)):
            Rv = float(c["rewards"][i]) + c["discount"] * Rv
            t[i] = Rv
        differs += not np.array_equal(BITS64(t), BITS64(c["targets"]))
    assert differs > 0


def test_terminal_windows_ignore_the_bootstrap_and_discount_sum_is_the_recurrence():
    rng = np.random.RandomState(0)
    V, r = (rng.randn(7) * 0.3).astype(np.float32), rng.uniform(-1, 2, 7).astype(np.float32)
    for rescaler in (R.A_VALUE, R.GAE):
        a = R.window_targets(V, np.float32(5.0), r, True, 0.99, 0.96, rescaler)
        b = R.window_targets(V, np.float32(-3.0), r, True, 0.99, 0.96, rescaler)
        assert np.array_equal(a["targets"], b["targets"]) and np.array_equal(a["advantages"], b["advantages"])
        c = R.window_targets(V, np.float32(5.0), r, False, 0.99, 0.96, rescaler)
        assert not np.array_equal(a["targets"], c["targets"])
    x = rng.randn(6)
    y = R.discount_sum(x, 0.9)
    assert y[5] == x[5] and all(y[i] == x[i] + 0.9 * y[i + 1] for i in range(5))
    # GAE with lambda 1 is the A_VALUE advantage up to rounding, and the non-GAE value targets are the A_VALUE targets
    g = R.window_targets(V, np.float32(0.5), r, False, 0.99, 1.0, R.GAE)
    a = R.window_targets(V, np.float32(0.5), r, False, 0.99, 1.0, R.A_VALUE)
    np.testing.assert_allclose(g["advantages"], a["advantages"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(g["targets"], a["targets"], rtol=0, atol=1e-6)
    with pytest.raises(ValueError, match="rescaler"):
        R.window_targets(V, np.float32(0.5), r, False, 0.99, 1.0, 1)


def _loss64(V, z, actions, tgt, adv, beta, w, T):
    """the fp64 form of head_losses' total: 0.5-weighted MSE + pg_ref's head loss evaluated in fp64"""
    return w * np.mean((V[:T] - tgt) ** 2) + pg_ref.head_loss(z, actions, adv, beta, T=T, dtype=np.float64)["loss"]


@pytest.mark.parametrize("beta", [0.0, 0.01])
@pytest.mark.parametrize("A", [2, 6])
@pytest.mark.parametrize("T", [1, 5])
def test_loss_gradients_equal_central_differences_of_their_own_loss(T, A, beta):
    """The method and the bound of tests/test_pg_ref.py's head test: the loss evaluated in fp64, dV and dlogits against
    (L(x + h e) - L(x - h e)) / 2h with h = 1e-6; truncation ~1e-13, rounding 2^-53 |L| / h ~ 1e-10, 1e-7 absolute is
    stated.  The forward pass has T + 1 rows (the bootstrap row gets no term and a zero gradient)."""
    rng = np.random.RandomState(10 * T + A)
    rows, w = T + 1, 0.5
    z, V = rng.randn(rows, A) * 2, rng.randn(rows)
    actions, adv, tgt = rng.randint(0, A, size=T), rng.randn(T), rng.randn(T)
    pol = pg_ref.head_loss(z, actions, adv, beta, T=T, dtype=np.float64)
    dV = np.zeros(rows)
    dV[:T] = (w * (2 * (V[:T] - tgt))) / T
    h = 1e-6
    numV, numZ = np.zeros(rows), np.zeros((rows, A))
    for b in range(rows):
        Vp, Vm = V.copy(), V.copy()
        Vp[b] += h
        Vm[b] -= h
        numV[b] = (_loss64(Vp, z, actions, tgt, adv, beta, w, T) - _loss64(Vm, z, actions, tgt, adv, beta, w, T)) / (2 * h)
        for j in range(A):
            zp, zm = z.copy(), z.copy()
            zp[b, j] += h
            zm[b, j] -= h
            numZ[b, j] = (_loss64(V, zp, actions, tgt, adv, beta, w, T) -
                          _loss64(V, zm, actions, tgt, adv, beta, w, T)) / (2 * h)
    assert np.abs(pol["dlogits"]).max() > 1e-3 and np.abs(dV).max() > 1e-3
    np.testing.assert_allclose(dV, numV, rtol=0, atol=1e-7)
    np.testing.assert_allclose(pol["dlogits"], numZ, rtol=0, atol=1e-7)
    assert numV[T] == 0 and np.all(numZ[T] == 0)
    # the fp32 restatement the device test compares against is that loss and those gradients to fp32 rounding
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    r = R.head_losses(f32(V), f32(z), actions, f32(tgt), f32(adv), beta, w, T)
    V6, z6, t6, a6 = (f32(x).astype(np.float64) for x in (V, z, tgt, adv))
    p6 = pg_ref.head_loss(z6, actions, a6, beta, T=T, dtype=np.float64)
    assert all(r[k].dtype == np.float32 for k in ("loss", "value_loss", "policy_loss", "entropy", "dV", "dlogits"))
    np.testing.assert_allclose(r["loss"], _loss64(V6, z6, actions, t6, a6, beta, w, T), rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(r["value_loss"], w * np.mean((V6[:T] - t6) ** 2), rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(r["policy_loss"], p6["loss"] + beta * p6["entropy"], rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(r["entropy"], p6["entropy"], rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(r["dV"][:T], (w * 2 * (V6[:T] - t6)) / T, rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(r["dlogits"], p6["dlogits"], rtol=1e-4, atol=2e-6)
    assert r["dV"][T] == 0 and np.all(r["dlogits"][T] == 0)


def test_head_losses_divide_by_T_and_sum_the_two_heads():
    rng = np.random.RandomState(4)
    T, A = 6, 3
    V, z = rng.randn(T + 1).astype(np.float32), rng.randn(T + 1, A).astype(np.float32)
    actions, adv, tgt = rng.randint(0, A, T), rng.randn(T).astype(np.float32), rng.randn(T).astype(np.float32)
    with_row = R.head_losses(V, z, actions, tgt, adv, 0.01, 0.5, T)
    bare = R.head_losses(V[:T], z[:T], actions, tgt, adv, 0.01, 0.5, T)
    for k in ("loss", "value_loss", "policy_loss", "entropy"):
        assert with_row[k].tobytes() == bare[k].tobytes()
    assert np.array_equal(with_row["dV"][:T], bare["dV"]) and np.array_equal(with_row["dlogits"][:T], bare["dlogits"])
    np.testing.assert_allclose(bare["value_loss"], 0.5 * np.mean((V[:T] - tgt) ** 2), rtol=1e-6)
    assert bare["loss"] == bare["value_loss"] + (bare["policy_loss"] - np.float32(0.01) * bare["entropy"])
    # the policy half is pg_ref's: with the V head's weight 0 the total is its loss up to the summation order
    pol = pg_ref.head_loss(z[:T], actions, adv, 0.01)
    zero = R.head_losses(V[:T], z[:T], actions, tgt, adv, 0.01, 0.0, T)
    assert zero["value_loss"] == 0 and not zero["dV"].any() and np.array_equal(zero["dlogits"], pol["dlogits"])
    np.testing.assert_allclose(zero["loss"], pol["loss"], rtol=1e-6)
    np.testing.assert_allclose(zero["entropy"], pol["entropy"], rtol=1e-6)
    bad = R.head_losses(V[:T], z[:T], [0, 3, 1, -1, 2, 0], tgt, adv, 0.01, 0.5, T)
    assert bad["status"] == R.STATUS_BAD_ACTION and not bad["dlogits"][[1, 3]].any() and bad["dV"][[1, 3]].all()
    assert R.window_loss(V[:T], z[:T], actions, np.ones(T, np.float32), False, 0.99, 1.0, R.GAE, False, 0.01)["status"] \
        == R.STATUS_NO_BOOTSTRAP_ROW


def test_tree_sum_is_the_fixed_order_of_the_launch():
    rng = np.random.RandomState(1)
    for n in (1, 2, 255, 256, 257, 1025):
        x = rng.randn(n).astype(np.float32)
        part = np.zeros(256, np.float32)
        for b in range(n):
            part[b % 256] = part[b % 256] + x[b]
        s = 128
        while s:
            for t in range(s):
                part[t] = part[t] + part[t + s]
            s //= 2
        assert R.tree_sum(x).tobytes() == part[0].tobytes()


def _defaults(ap):
    net, alg = ap.network_wrappers["main"], ap.algorithm
    return {"policy_gradient_rescaler": alg.policy_gradient_rescaler.name,
            "apply_gradients_every_x_episodes": alg.apply_gradients_every_x_episodes, "beta_entropy": alg.beta_entropy,
            "num_steps_between_gradient_updates": alg.num_steps_between_gradient_updates, "discount": alg.discount,
            "gae_lambda": alg.gae_lambda, "estimate_state_value_using_gae": alg.estimate_state_value_using_gae,
            "learning_rate": net.learning_rate, "optimizer_type": net.optimizer_type,
            "optimizer_epsilon": net.optimizer_epsilon, "adam_optimizer_beta1": net.adam_optimizer_beta1,
            "adam_optimizer_beta2": net.adam_optimizer_beta2, "clip_gradients": net.clip_gradients,
            "async_training": net.async_training, "create_target_network": net.create_target_network,
            "heads": [[type(h).__name__, h.loss_weight] for h in net.heads_parameters],
            "embedder_scheme": net.input_embedders_parameters["observation"].scheme,
            "middleware_scheme": net.middleware_parameters.scheme,
            "activation_function": net.middleware_parameters.activation_function,
            "classes": [type(alg).__name__, type(net).__name__, type(ap).__name__],
            "discrete_exploration": type(ap.exploration).__name__, "memory": type(ap.memory).__name__}


def test_parameter_defaults_equal_the_reference(a3c):
    from coach_amd.agents.actor_critic_agent import ActorCriticAgentParameters
    from coach_amd.agents.policy_optimization_agent import PolicyGradientRescaler
    ap = ActorCriticAgentParameters()
    ref = json.loads(str(a3c["defaults"]))
    assert _defaults(ap) == ref
    assert ref["clip_gradients"] == 40.0 and ref["apply_gradients_every_x_episodes"] == 5
    assert ref["num_steps_between_gradient_updates"] == 5000 and ref["gae_lambda"] == 0.96
    assert ref["policy_gradient_rescaler"] == "A_VALUE"
    assert ap.path == "coach_amd.agents.actor_critic_agent:ActorCriticAgent"
    assert ap.memory.path == "coach_amd.memories.episodic.single_episode_buffer:SingleEpisodeBuffer"
    assert ap.exploration.path == "coach_amd.exploration_policies.categorical:Categorical"
    assert (R.A_VALUE, R.GAE) == (PolicyGradientRescaler.A_VALUE.value, PolicyGradientRescaler.GAE.value)
    heads = ap.network_wrappers["main"].heads_parameters
    assert [h.head_type for h in heads] == ["VHead", "PolicyHead"]


def test_reference_module_paths_resolve_through_the_import_layer():
    import coach_amd.compat as compat
    compat.install()
    import coach_amd.agents.actor_critic_agent as mine
    mod = importlib.import_module("rl_coach.agents.actor_critic_agent")
    assert mod.ActorCriticAgentParameters is mine.ActorCriticAgentParameters
    assert mod.ActorCriticAgent is mine.ActorCriticAgent
    assert mod.ActorCriticAlgorithmParameters is mine.ActorCriticAlgorithmParameters
    assert mod.ActorCriticNetworkParameters is mine.ActorCriticNetworkParameters
    from rl_coach.architectures.head_parameters import PolicyHeadParameters, VHeadParameters
    ap = mine.ActorCriticAgentParameters()
    v, pi = ap.network_wrappers["main"].heads_parameters
    assert isinstance(v, VHeadParameters) and isinstance(pi, PolicyHeadParameters)


def test_package_preset_equals_the_unchanged_reference_preset_text():
    """tests/golden/a3c_preset.json holds what the reference's CartPole_A3C.py text, executed unchanged through the import
    layer, set (make_a3c_preset_dump.py): the package's preset must equal it field by field."""
    from coach_amd.agents.policy_optimization_agent import PolicyGradientRescaler
    from coach_amd.compat import resolve_reference_style
    from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps
    from test_cartpole import _dump
    with open(os.path.join(GOLDEN, "a3c_preset.json")) as f:
        ref = json.load(f)["CartPole_A3C"]
    mine = importlib.import_module("coach_amd.presets.CartPole_A3C").make()
    resolve_reference_style(mine.agent_params, mine.env_params)      # what create_graph does first
    for part in ("agent_params", "schedule", "preset_validation_params"):
        assert ref[part] == _dump(getattr(mine, part)), part
    assert ref["level_name"] == "CartPole-v0" == mine.env_params.level
    alg, net = mine.agent_params.algorithm, mine.agent_params.network_wrappers["main"]
    assert alg.policy_gradient_rescaler is PolicyGradientRescaler.GAE and alg.gae_lambda == 1
    assert alg.reward_rescale == 1 / 200. and alg.discount == 0.99 and net.learning_rate == 0.0001
    assert alg.apply_gradients_every_x_episodes == 1 and alg.num_steps_between_gradient_updates == 5
    assert alg.beta_entropy == 0.01 and net.clip_gradients == 40.0 and not alg.estimate_state_value_using_gae
    s = mine.schedule
    assert isinstance(s.heatup_steps, EnvironmentSteps) and s.heatup_steps.num_steps == 0
    assert isinstance(s.steps_between_evaluation_periods, EnvironmentEpisodes)
    assert s.steps_between_evaluation_periods.num_steps == 10 and s.evaluation_steps.num_steps == 1
    v = mine.preset_validation_params
    assert v.test and v.min_reward_threshold == 150 and v.max_episodes_to_achieve_reward == 300 and v.num_workers == 8


def test_reference_preset_text_builds_through_the_import_layer():
    from test_preset_dropin import REF, _exec_preset, _text
    if not os.path.isdir(REF):
        pytest.skip("the reference's preset texts are not on this machine")
    from coach_amd.agents.policy_optimization_agent import PolicyGradientRescaler
    from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager
    ns = _exec_preset(_text("CartPole_A3C"))
    gm = ns["graph_manager"]
    assert isinstance(gm, BasicRLGraphManager) and gm.agent_params is ns["agent_params"]
    assert type(gm.agent_params).__module__ == "coach_amd.agents.actor_critic_agent"
    assert gm.agent_params.algorithm.policy_gradient_rescaler is PolicyGradientRescaler.GAE
    assert gm.schedule.heatup_steps.num_steps == 0 and gm.preset_validation_params.min_reward_threshold == 150
    assert gm.preset_validation_params.num_workers == 8               # accepted and kept as data


class _Params(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_unsupported_rescalers_and_spaces_are_refused_from_the_parameters_alone():
    """before anything touches the device (device None)"""
    from coach_amd.agents.actor_critic_agent import ActorCriticAgent, ActorCriticAgentParameters
    from coach_amd.agents.policy_optimization_agent import PolicyGradientRescaler
    discrete = _Params(p=_Params(kind="vector", num_envs=1, observation_shape=(4,), num_actions=2, action_dim=None,
                                 episode_length=200))
    for r in PolicyGradientRescaler:
        if r in (PolicyGradientRescaler.A_VALUE, PolicyGradientRescaler.GAE):
            continue
        ap = ActorCriticAgentParameters()
        ap.algorithm.policy_gradient_rescaler = r
        with pytest.raises(ValueError, match="rescaler"):
            ActorCriticAgent(ap, discrete, None)
    box = _Params(p=_Params(kind="vector", num_envs=1, observation_shape=(3,), num_actions=None, action_dim=1,
                            episode_length=200))
    with pytest.raises(ValueError, match="continuous PolicyHead"):
        ActorCriticAgent(ActorCriticAgentParameters(), box, None)
    with pytest.raises(ValueError, match="data-parallel"):
        ActorCriticAgent(ActorCriticAgentParameters(), discrete, None, dist=_Params(enabled=True, rank=0))
    image = _Params(p=_Params(kind="image", num_envs=1, observation_shape=(84, 84), num_actions=4, action_dim=None,
                              episode_length=100))
    with pytest.raises(ValueError, match="image observations"):
        ActorCriticAgent(ActorCriticAgentParameters(), image, None)
