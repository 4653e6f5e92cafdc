"""Vanilla Policy Gradients on the CPU: the numpy restatement (tests/pg_ref.py) against what the reference's own
PolicyGradientsAgent computed (tests/golden/pg.npz, make_golden_pg.py), the head loss's gradient against central
differences of its own fp64 loss (what stands in for TensorFlow, which cannot run here), the package's parameter
defaults, exploration policy and CartPole_PG preset against the reference's (tests/golden/pg_preset.json), and what the
agent refuses."""
import importlib
import json
import os

import numpy as np
import pytest

import pg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_RUNS = 10
RESCALER_OF_RUN = (0, 0, 1, 1, 2, 2, 3, 3, 3, 0)
BITS64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def mean_std_tolerance(x):
    """np.mean / np.std of the T values x against another summation order: T * 2^-53 relative — relative to the size of
    the summed values, 2 max|x| (the deviations from the mean are at most that), because a relative bound on a mean
    that cancels to (nearly) zero is a bound no summation meets."""
    x = np.asarray(x, dtype=np.float64)
    return x.size * 2.0 ** -53 * 2.0 * max(float(np.abs(x).max()), np.finfo(np.float64).tiny)


def fixture_run(z, r):
    p = "r%d_" % r
    lengths = z[p + "lengths"]
    cut = np.cumsum(lengths)[:-1]
    keys = ("win_first", "win_len", "win_actions", "targets", "applied", "current_episode", "training_iteration", "mean",
            "seen", "episode_mean", "episode_std", "returns_mean", "returns_variance")
    return dict({k: z[p + k] for k in keys}, lengths=lengths, rewards=np.split(z[p + "rewards"], cut),
                actions=np.split(z[p + "actions"], cut), discount=float(z[p + "discount"]), t_max=int(z[p + "t_max"]),
                rescaler=int(z[p + "rescaler"]))


@pytest.fixture(scope="module")
def pg():
    return np.load(os.path.join(GOLDEN, "pg.npz"))


@pytest.mark.parametrize("r", range(N_RUNS))
def test_windows_targets_statistics_and_cadence_equal_the_reference_agent(pg, r):
    f = fixture_run(pg, r)
    assert f["rescaler"] == RESCALER_OF_RUN[r] and f["rewards"][0].dtype == np.float32
    ws = R.run(f["rewards"], f["discount"], f["rescaler"], 24, f["t_max"], 5)
    offsets = np.concatenate([[0], np.cumsum(f["lengths"])])
    assert np.array_equal(f["win_first"], [offsets[w["episode"]] + w["start"] for w in ws])
    assert np.array_equal(f["win_len"], [w["end"] - w["start"] for w in ws])
    # the cadence: current_episode and training_iteration at every window, the windows that applied the gradients
    assert np.array_equal(f["current_episode"], [w["current_episode"] for w in ws])
    assert np.array_equal(f["training_iteration"], [w["training_iteration"] for w in ws])
    assert np.array_equal(f["applied"], [w["applied"] for w in ws]) and f["applied"].any() and not f["applied"].all()
    assert np.array_equal(f["applied"], f["current_episode"] % 5 == 0)
    # the targets handed to accumulate_gradients, bit for bit (np.mean / np.std are numpy's own on both sides)
    targets = np.concatenate([w["rescaled"] for w in ws])
    assert targets.dtype == np.float64 and np.array_equal(BITS64(targets), BITS64(f["targets"]))
    first = 0
    for i, w in enumerate(ws):
        T = w["end"] - w["start"]
        acts = f["actions"][w["episode"]][w["start"]:w["end"]]
        assert np.array_equal(f["win_actions"][first:first + T], acts)
        first += T
        if f["rescaler"] >= R.FUTURE_RETURN_NORMALIZED_BY_EPISODE:
            # the episode's np.mean / np.std (the per-timestep statistics have a test of their own below)
            assert abs(w["episode_mean"] - f["episode_mean"][i]) <= mean_std_tolerance(w["returns"])
            assert abs(w["episode_std"] - f["episode_std"][i]) <= mean_std_tolerance(w["returns"])
        # the two signals: np.mean, and np.std under the name 'Returns Variance', compared at T * 2^-53 relative
        assert abs(w["returns_mean"] - f["returns_mean"][i]) <= mean_std_tolerance(w["rescaled"])
        assert abs(w["returns_std"] - f["returns_variance"][i]) <= mean_std_tolerance(w["rescaled"])
        assert w["advantages"].dtype == np.float32 and np.array_equal(w["advantages"], w["rescaled"].astype(np.float32))
    if f["rescaler"] == R.TOTAL_RETURN:
        assert all(np.all(w["rescaled"] == w["returns"][w["start"]]) for w in ws)       # entry 0 of the WINDOW
    if f["rescaler"] == R.FUTURE_RETURN_NORMALIZED_BY_EPISODE:
        one = [w for w in ws if w["end"] == 1 and w["complete"]]
        assert one and all(w["episode_std"] == 0 and np.all(w["rescaled"] == 0) for w in one)       # std == 0 gives 0


@pytest.mark.parametrize("r", [4, 6, 8])
def test_per_timestep_statistics_equal_the_reference_after_every_window(pg, r):
    """replayed window by window: mean_return_over_multiple_episodes and num_episodes_where_step_has_been_seen"""
    f = fixture_run(pg, r)
    stats = R.Statistics(24)
    ws = R.run(f["rewards"], f["discount"], f["rescaler"], 24, f["t_max"], 5)
    for i, w in enumerate(ws):
        R.window(f["rewards"][w["episode"]][:w["end"]], w["start"], f["discount"], f["rescaler"], stats)
        assert np.array_equal(BITS64(stats.mean), BITS64(f["mean"][i]))
        assert np.array_equal(BITS64(stats.seen), BITS64(f["seen"][i]))
    # a longer episode after shorter ones: the counts differ along the episode
    assert len(set(stats.seen[:16].tolist())) > 3 and stats.seen[0] > stats.seen[15] >= 1


def test_fixture_holds_the_cases_the_windows_are_checked_on(pg):
    f = fixture_run(pg, 8)
    L = f["lengths"].tolist()
    assert len(L) >= 12 and {1, 2, 7, 8, 9} <= set(L)
    assert any(L[i] > max(L[:i]) for i in range(1, len(L))) and any(L[i] < min(L[:i]) for i in range(1, len(L)))
    assert f["t_max"] == 5 and len(f["win_len"]) > len(L)            # windows that start in the middle of an episode
    assert all(len(set(r.tolist())) > 1 for r in f["rewards"] if r.size > 1)
    assert {float(pg["r%d_discount" % r]) for r in range(N_RUNS)} == {0.99, 1.0}
    # the batch-position quirk of FUTURE_RETURN_NORMALIZED_BY_TIMESTEP shows: a window that starts at step s > 0 is
    # baselined with entries [0, T) of the statistics, not [s, s + T)
    ws = R.run(f["rewards"], 0.99, 3, 24, 5, 5)
    stats = R.Statistics(24)
    shown = False
    for w in ws:
        R.window(f["rewards"][w["episode"]][:w["end"]], w["start"], 0.99, 3, stats)
        if w["start"] > 0:
            T = w["end"] - w["start"]
            by_position = w["returns"][w["start"]:] - stats.mean[:T]
            by_timestep = w["returns"][w["start"]:] - stats.mean[w["start"]:w["end"]]
            assert np.array_equal(w["rescaled"], by_position)
            shown = shown or not np.array_equal(by_position, by_timestep)
    assert shown


@pytest.mark.parametrize("beta", [0.0, 0.01])
@pytest.mark.parametrize("A", [2, 6])
@pytest.mark.parametrize("T", [1, 5])
def test_head_loss_gradient_equals_central_differences_of_its_own_loss(T, A, beta):
    """The restatement evaluated in fp64: dlogits against (L(z + h e) - L(z - h e)) / 2h with h = 1e-6.  The truncation
    error is h^2 / 6 * |L'''| ~ 1e-13 and the rounding error 2^-53 * |L| / h ~ 1e-10 for |L| ~ 1, so the two agree to
    about 1e-9; 1e-7 absolute (a hundred times that, and a thousandth of a typical entry) is stated."""
    rng = np.random.RandomState(10 * T + A)
    z = rng.randn(T, A) * 2
    actions, adv = rng.randint(0, A, size=T), rng.randn(T)
    r = R.head_loss(z, actions, adv, beta, dtype=np.float64)
    h, num = 1e-6, np.zeros((T, A))
    for b in range(T):
        for j in range(A):
            zp, zm = z.copy(), z.copy()
            zp[b, j] += h
            zm[b, j] -= h
            num[b, j] = (R.head_loss(zp, actions, adv, beta, dtype=np.float64)["loss"] -
                         R.head_loss(zm, actions, adv, beta, dtype=np.float64)["loss"]) / (2 * h)
    assert np.abs(r["dlogits"]).max() > 1e-3
    np.testing.assert_allclose(r["dlogits"], num, rtol=0, atol=1e-7)
    # the fp32 restatement the device test compares against is that loss and gradient to fp32 rounding
    r32 = R.head_loss(z.astype(np.float32), actions, adv.astype(np.float32), beta)
    r64 = R.head_loss(z.astype(np.float32).astype(np.float64), actions, adv.astype(np.float32).astype(np.float64), beta,
                      dtype=np.float64)
    assert r32["dlogits"].dtype == np.float32 and r32["loss"].dtype == np.float32
    np.testing.assert_allclose(r32["loss"], r64["loss"], rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(r32["entropy"], r64["entropy"], rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(r32["dlogits"], r64["dlogits"], rtol=1e-4, atol=2e-6)


def test_head_loss_formula_and_the_eps_of_the_saturated_row():
    """loss = -mean(log pi(a) adv) - beta mean(H) with pi = (p + eps) / sum(p + eps); entropy regularisation lowers the
    loss of a uniform policy; a saturated row's log-probability is finite because of eps; padding and an invalid action
    contribute nothing"""
    z = np.array([[0.0, 0.0, 0.0], [-30.0, 30.0, -30.0]])
    adv = np.array([1.0, 2.0])
    r = R.head_loss(z, [0, 0], adv, 0.0, dtype=np.float64)
    p, q, S, lp, H = R.head_rows(z, np.float64)
    assert np.isclose(H[0], np.log(3.0)) and np.isclose(lp[0, 0], -np.log(3.0))
    assert p[1, 0] < 1e-25 and np.isclose(lp[1, 0], np.log(R.EPS / (1 + 3 * R.EPS)), rtol=1e-6)
    assert np.isclose(r["loss"], -(lp[0, 0] * 1.0 + lp[1, 0] * 2.0) / 2)
    rb = R.head_loss(z, [0, 0], adv, 0.5, dtype=np.float64)
    assert np.isclose(rb["loss"], r["loss"] - 0.5 * H.mean()) and np.isclose(rb["entropy"], H.mean())
    padded = R.head_loss(np.vstack([z, [[5.0, 1.0, 2.0]]]), [0, 0], adv, 0.5, T=2, dtype=np.float64)
    assert padded["loss"] == rb["loss"] and np.all(padded["dlogits"][2] == 0)
    assert np.array_equal(padded["dlogits"][:2], rb["dlogits"])
    bad = R.head_loss(z, [0, 3], adv, 0.5, dtype=np.float64)
    assert bad["status"] == 1 and np.all(bad["dlogits"][1] == 0) and np.any(bad["dlogits"][0] != 0)
    assert np.allclose(rb["dlogits"].sum(axis=1), 0, atol=1e-15)      # a softmax's gradient sums to zero per row


def _defaults(ap):
    from coach_amd.agents.policy_optimization_agent import PolicyGradientRescaler
    net, alg = ap.network_wrappers["main"], ap.algorithm
    return {"policy_gradient_rescaler": alg.policy_gradient_rescaler.name,
            "apply_gradients_every_x_episodes": alg.apply_gradients_every_x_episodes, "beta_entropy": alg.beta_entropy,
            "num_steps_between_gradient_updates": alg.num_steps_between_gradient_updates, "discount": alg.discount,
            "learning_rate": net.learning_rate, "optimizer_type": net.optimizer_type,
            "optimizer_epsilon": net.optimizer_epsilon, "adam_optimizer_beta1": net.adam_optimizer_beta1,
            "adam_optimizer_beta2": net.adam_optimizer_beta2, "clip_gradients": net.clip_gradients,
            "async_training": net.async_training, "create_target_network": net.create_target_network,
            "head": type(net.heads_parameters[0]).__name__, "heads": len(net.heads_parameters),
            "embedder_scheme": net.input_embedders_parameters["observation"].scheme,
            "middleware_scheme": net.middleware_parameters.scheme,
            "activation_function": net.middleware_parameters.activation_function,
            "classes": [type(alg).__name__, type(net).__name__, type(ap).__name__],
            "discrete_exploration": type(ap.exploration).__name__, "memory": type(ap.memory).__name__,
            "rescalers": {r.name: r.value for r in PolicyGradientRescaler}}


def test_parameter_defaults_equal_the_reference(pg):
    from coach_amd.agents.policy_gradients_agent import PolicyGradientsAgentParameters
    ap = PolicyGradientsAgentParameters()
    assert _defaults(ap) == json.loads(str(pg["defaults"]))
    assert ap.path == "coach_amd.agents.policy_gradients_agent:PolicyGradientsAgent"
    assert ap.memory.path == "coach_amd.memories.episodic.single_episode_buffer:SingleEpisodeBuffer"
    assert ap.exploration.path == "coach_amd.exploration_policies.categorical:Categorical"
    assert not hasattr(ap.memory, "max_size") or ap.memory.max_size is None
    assert (R.TOTAL_RETURN, R.FUTURE_RETURN, R.FUTURE_RETURN_NORMALIZED_BY_EPISODE,
            R.FUTURE_RETURN_NORMALIZED_BY_TIMESTEP) == (0, 1, 2, 3)


def test_there_is_one_policy_gradient_rescaler():
    import coach_amd.agents.policy_gradients_agent as pga
    import coach_amd.agents.policy_optimization_agent as poa
    assert pga.PolicyGradientRescaler is poa.PolicyGradientRescaler


def test_reference_module_paths_resolve_through_the_import_layer():
    import coach_amd.compat as compat
    compat.install()
    import coach_amd.agents.policy_gradients_agent as mine
    mod = importlib.import_module("rl_coach.agents.policy_gradients_agent")
    assert mod.PolicyGradientsAgentParameters is mine.PolicyGradientsAgentParameters
    assert mod.PolicyGradientsAgent is mine.PolicyGradientsAgent
    from rl_coach.agents.policy_optimization_agent import PolicyGradientRescaler
    from rl_coach.architectures.head_parameters import PolicyHeadParameters
    from rl_coach.exploration_policies.categorical import Categorical, CategoricalParameters
    from rl_coach.memories.episodic.single_episode_buffer import SingleEpisodeBufferParameters
    ap = mine.PolicyGradientsAgentParameters()
    assert isinstance(ap.network_wrappers["main"].heads_parameters[0], PolicyHeadParameters)
    assert isinstance(ap.exploration, CategoricalParameters) and isinstance(ap.memory, SingleEpisodeBufferParameters)
    assert ap.algorithm.policy_gradient_rescaler is PolicyGradientRescaler.FUTURE_RETURN_NORMALIZED_BY_TIMESTEP
    assert Categorical.__module__ == "coach_amd.exploration_policies.categorical"


def test_package_preset_equals_the_unchanged_reference_preset_text():
    """tests/golden/pg_preset.json holds what the reference's CartPole_PG.py text, executed unchanged through the import
    layer, set (make_pg_preset_dump.py): the package's preset must equal it field by field."""
    from coach_amd.compat import resolve_reference_style
    from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps
    from test_cartpole import _dump
    with open(os.path.join(GOLDEN, "pg_preset.json")) as f:
        ref = json.load(f)["CartPole_PG"]
    mine = importlib.import_module("coach_amd.presets.CartPole_PG").make()
    resolve_reference_style(mine.agent_params, mine.env_params)      # what create_graph does first
    for part in ("agent_params", "schedule", "preset_validation_params"):
        assert ref[part] == _dump(getattr(mine, part)), part
    assert ref["level_name"] == "CartPole-v0" == mine.env_params.level
    alg, net = mine.agent_params.algorithm, mine.agent_params.network_wrappers["main"]
    assert alg.reward_rescale == 1 / 200. and alg.discount == 0.99 and net.learning_rate == 0.0005
    assert alg.apply_gradients_every_x_episodes == 5 and alg.num_steps_between_gradient_updates == 20000
    s = mine.schedule
    assert isinstance(s.heatup_steps, EnvironmentSteps) and s.heatup_steps.num_steps == 0
    assert isinstance(s.steps_between_evaluation_periods, EnvironmentEpisodes)
    assert s.steps_between_evaluation_periods.num_steps == 20 and s.evaluation_steps.num_steps == 1
    v = mine.preset_validation_params
    assert v.test and v.min_reward_threshold == 130 and v.max_episodes_to_achieve_reward == 550


def test_reference_preset_text_builds_through_the_import_layer():
    from test_preset_dropin import REF, _exec_preset, _text
    if not os.path.isdir(REF):
        pytest.skip("the reference's preset texts are not on this machine")
    from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager
    ns = _exec_preset(_text("CartPole_PG"))
    gm = ns["graph_manager"]
    assert isinstance(gm, BasicRLGraphManager) and gm.agent_params is ns["agent_params"]
    assert type(gm.agent_params).__module__ == "coach_amd.agents.policy_gradients_agent"
    assert gm.schedule.heatup_steps.num_steps == 0 and gm.preset_validation_params.min_reward_threshold == 130


def test_categorical_draws_leave_np_random_in_the_recorded_state(pg):
    from coach_amd.core_types import RunPhase
    from coach_amd.exploration_policies.categorical import Categorical, CategoricalParameters
    rows = pg["cat_probs"]
    np.random.seed(int(pg["cat_seed"]))
    s0 = np.random.get_state()
    pol = Categorical(4, 1, None, CategoricalParameters())           # no draw on construction (EGreedy makes one)
    assert np.array_equal(np.random.get_state()[1], s0[1]) and np.random.get_state()[2] == s0[2]
    pol.phase = RunPhase.TRAIN
    train = [pol.get_action(p)[0] for p in rows]
    s1 = np.random.get_state()
    assert train == pg["cat_train"].tolist()
    assert np.array_equal(s1[1], pg["cat_state_after_keys"]) and s1[2] == int(pg["cat_state_after_pos"])
    pol.phase = RunPhase.TEST
    test = [pol.get_action(p)[0] for p in rows]
    s2 = np.random.get_state()
    assert test == pg["cat_test"].tolist() and np.array_equal(s1[1], s2[1]) and s1[2] == s2[2]      # no draw
    assert test[1] == 0 and test[4] == 1                             # tied maxima: the first one
    one_hot = pol.get_action(rows[1])[1]
    assert one_hot.tolist() == [1, 0, 0, 0]
    # the vector form the agent uses: one uniform per env, in env order, only in TRAIN
    np.random.seed(int(pg["cat_seed"]))
    vec = Categorical(4, len(rows), None)
    vec.phase = RunPhase.TRAIN
    u = vec.draw()
    s3 = np.random.get_state()
    assert u.shape == (len(rows),) and np.array_equal(s3[1], s1[1]) and s3[2] == s1[2]
    cdf = rows.astype(np.float64).cumsum(axis=1)
    assert [int(np.searchsorted(c / c[-1], x, side="right")) for c, x in zip(cdf, u)] == train
    vec.phase = RunPhase.TEST
    assert vec.draw() is None


class _Params(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_a_box_action_space_and_a_data_parallel_agent_are_refused():
    """both are refused from the parameters alone, before anything touches the device"""
    from coach_amd.agents.policy_gradients_agent import PolicyGradientsAgent, PolicyGradientsAgentParameters
    from coach_amd.agents.policy_optimization_agent import PolicyGradientRescaler
    discrete = _Params(p=_Params(kind="vector", num_envs=1, observation_shape=(4,), num_actions=2, action_dim=None,
                                 episode_length=200))
    box = _Params(p=_Params(kind="vector", num_envs=1, observation_shape=(3,), num_actions=None, action_dim=1,
                            episode_length=200))
    with pytest.raises(ValueError, match="continuous PolicyHead"):
        PolicyGradientsAgent(PolicyGradientsAgentParameters(), box, None)
    with pytest.raises(ValueError, match="data-parallel"):
        PolicyGradientsAgent(PolicyGradientsAgentParameters(), discrete, None, dist=_Params(enabled=True, rank=0))
    image = _Params(p=_Params(kind="image", num_envs=1, observation_shape=(84, 84), num_actions=4, action_dim=None,
                              episode_length=100))
    with pytest.raises(ValueError, match="image observations"):
        PolicyGradientsAgent(PolicyGradientsAgentParameters(), image, None)
    ap = PolicyGradientsAgentParameters()
    ap.algorithm.policy_gradient_rescaler = PolicyGradientRescaler.GAE
    with pytest.raises(ValueError, match="rescaler"):
        PolicyGradientsAgent(ap, discrete, None)
