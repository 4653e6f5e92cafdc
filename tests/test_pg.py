"""Vanilla Policy Gradients on the device: rlx_pg_episode_window and rlx_pg_head_loss (csrc/policy_gradient.hip) against
the numpy restatement (tests/pg_ref.py, itself pinned to the reference agent by tests/test_pg_ref.py), the network
update against the oracle's layers + TF1 Adam composed with that restatement, the agent's windows and cadence on the
device CartPole, and the golden bar of CartPole_PG.

Tolerances.  The returns, the per-timestep statistics and the TOTAL_RETURN / FUTURE_RETURN /
FUTURE_RETURN_NORMALIZED_BY_TIMESTEP targets are compared bit for bit (fp64 restated operation by operation; the fp32
advantages are those values rounded once).  np.mean / np.std quantities (the episode's mean and std, the
FUTURE_RETURN_NORMALIZED_BY_EPISODE targets that are formed from them, 'Returns Mean', 'Returns Variance') go through
numpy's pairwise summation: they are compared at T * 2^-53 relative (mean_std_tolerance in tests/test_pg_ref.py says
relative to what).  The head's loss, entropy and gradient differ from the restatement by fp32 summation order only and
are compared under tests/tolerances.py's LOSS and OUT, as tests/test_c51.py compares its loss kernel."""
import numpy as np
import pytest

import pg_ref as R
from test_pg_ref import fixture_run, mean_std_tolerance
from tolerances import LOSS, OUT, WEIGHTS

pytestmark = pytest.mark.gpu

BITS64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _t(x, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t if dtype is None else t.to(dtype)


class DeviceWindows(object):
    """the device side of one agent's statistics and window outputs, max_len entries each"""

    def __init__(self, rlx, dev, max_len):
        import torch
        self.rlx, self.dev, self.max_len = rlx, dev, max_len
        z = lambda dt: torch.zeros(max_len, dtype=dt, device=dev)
        self.mean, self.seen = z(torch.float64), z(torch.float64)
        self.returns, self.rescaled, self.adv = z(torch.float64), z(torch.float64), z(torch.float32)
        self.stats = torch.zeros(4, dtype=torch.float64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)

    def launch(self, rewards, start, discount, rescaler):
        L = len(rewards)
        self.rlx.pg_episode_window(_t(np.asarray(rewards, np.float32), self.dev), L, start, discount, rescaler,
                                   self.mean, self.seen, self.max_len, self.returns, self.rescaled, self.adv,
                                   self.stats, self.status, 0)
        T = L - start
        st = self.stats.cpu().numpy()
        return dict(returns=self.returns.cpu().numpy()[:min(L, self.max_len)], rescaled=self.rescaled.cpu().numpy()[:T],
                    advantages=self.adv.cpu().numpy()[:T], returns_mean=st[0], returns_std=st[1], episode_mean=st[2],
                    episode_std=st[3], status=int(self.status.item()))


@pytest.mark.parametrize("run", range(10))
def test_episode_window_equals_the_restatement_on_the_fixture_runs(rlx, dev, golden, run):
    """every window of a fixture run (four rescalers x two discounts with whole-episode windows, two runs whose windows
    start in the middle of an episode), the statistics carried on the device from window to window"""
    f = fixture_run(golden("pg"), run)
    ws = R.run(f["rewards"], f["discount"], f["rescaler"], 24, f["t_max"], 5)
    d = DeviceWindows(rlx, dev, 24)
    exact = f["rescaler"] != R.FUTURE_RETURN_NORMALIZED_BY_EPISODE
    first = 0
    for i, w in enumerate(ws):
        k = d.launch(f["rewards"][w["episode"]][:w["end"]], w["start"], f["discount"], f["rescaler"])
        T = w["end"] - w["start"]
        assert k["status"] == 0
        assert np.array_equal(BITS64(k["returns"]), BITS64(w["returns"]))
        normalized = f["rescaler"] >= R.FUTURE_RETURN_NORMALIZED_BY_EPISODE
        if normalized:            # the per-timestep statistics: the restatement's AND the reference's own
            assert np.array_equal(BITS64(d.mean.cpu().numpy()), BITS64(f["mean"][i]))
            assert np.array_equal(BITS64(d.seen.cpu().numpy()), BITS64(f["seen"][i]))
            x = w["returns"]
            assert abs(k["episode_mean"] - w["episode_mean"]) <= mean_std_tolerance(x)
            assert abs(k["episode_std"] - w["episode_std"]) <= mean_std_tolerance(x)
        else:
            assert not d.mean.cpu().numpy().any() and not d.seen.cpu().numpy().any()
        ref_targets = f["targets"][first:first + T]
        first += T
        if exact:
            assert np.array_equal(BITS64(k["rescaled"]), BITS64(w["rescaled"]))
            assert np.array_equal(BITS64(k["rescaled"]), BITS64(ref_targets))             # the reference agent's targets
            assert np.array_equal(k["advantages"].view(np.uint32), w["advantages"].view(np.uint32))
        else:
            # (x - mean) / std with mean and std at T * 2^-53: the quotient moves by that much of |x - mean| / std, plus
            # the mean's own error over std
            x = w["returns"]
            if w["episode_std"] == 0:
                assert np.all(k["rescaled"] == 0) and np.all(k["advantages"] == 0)       # the std == 0 branch
            else:
                tol = (mean_std_tolerance(x) / w["episode_std"]) * (1.0 + np.abs(w["rescaled"])) + 2.0 ** -52
                assert np.all(np.abs(k["rescaled"] - w["rescaled"]) <= tol)
                assert np.all(np.abs(k["rescaled"] - ref_targets) <= tol)
            assert np.array_equal(k["advantages"], k["rescaled"].astype(np.float32))       # ONE rounding from fp64
        assert abs(k["returns_mean"] - w["returns_mean"]) <= mean_std_tolerance(w["rescaled"]) + \
            (0 if exact else np.abs(k["rescaled"] - w["rescaled"]).max())
        assert abs(k["returns_std"] - w["returns_std"]) <= mean_std_tolerance(w["rescaled"]) + \
            (0 if exact else 2 * np.abs(k["rescaled"] - w["rescaled"]).max())
        assert abs(k["returns_mean"] - f["returns_mean"][i]) <= mean_std_tolerance(w["rescaled"]) + \
            (0 if exact else np.abs(k["rescaled"] - w["rescaled"]).max())
    assert any(w["start"] > 0 for w in ws) == (f["t_max"] == 5)
    assert any(w["end"] - w["start"] == 1 and w["start"] == 0 for w in ws)                 # a one-step episode


@pytest.mark.parametrize("rescaler", [R.FUTURE_RETURN, R.FUTURE_RETURN_NORMALIZED_BY_TIMESTEP])
def test_episode_window_at_and_one_past_the_array_limit(rlx, dev, rescaler):
    """an episode of exactly max_length steps is served (here past the LDS staging size and past the pairwise
    summation's block of 128); one step more raises the status and touches nothing"""
    rng = np.random.RandomState(5)
    max_len = 2051
    rewards = rng.uniform(-1, 2, size=max_len + 1).astype(np.float32)
    d = DeviceWindows(rlx, dev, max_len)
    stats = R.Statistics(max_len)
    w = R.window(rewards[:max_len], 3, 0.99, rescaler, stats)
    k = d.launch(rewards[:max_len], 3, 0.99, rescaler)
    assert k["status"] == 0
    assert np.array_equal(BITS64(k["returns"]), BITS64(w["returns"]))
    assert np.array_equal(BITS64(k["rescaled"]), BITS64(w["rescaled"]))
    assert np.array_equal(BITS64(d.mean.cpu().numpy()), BITS64(stats.mean))
    assert abs(k["returns_mean"] - w["returns_mean"]) <= mean_std_tolerance(w["rescaled"])
    assert abs(k["returns_std"] - w["returns_std"]) <= mean_std_tolerance(w["rescaled"])
    before = [t.clone() for t in (d.mean, d.seen, d.returns, d.rescaled, d.adv, d.stats)]
    assert R.window(rewards, 3, 0.99, rescaler, stats) is None
    import torch
    d.rlx.pg_episode_window(_t(rewards, dev), max_len + 1, 3, 0.99, rescaler, d.mean, d.seen, max_len, d.returns,
                            d.rescaled, d.adv, d.stats, d.status, 0)
    assert int(d.status.item()) == R.STATUS_EPISODE_TOO_LONG
    for a, b in zip(before, (d.mean, d.seen, d.returns, d.rescaled, d.adv, d.stats)):
        assert torch.equal(a, b)


def test_episode_window_refuses_bad_arguments(rlx, dev):
    from coach_amd._rlx import RlxError
    d = DeviceWindows(rlx, dev, 8)
    r = _t(np.ones(8, np.float32), dev)
    for length, start, rescaler in ((0, 0, 1), (4, 4, 1), (4, -1, 1), (4, 0, 4), (4, 0, -1)):
        with pytest.raises(RlxError):
            rlx.pg_episode_window(r, length, start, 0.99, rescaler, d.mean, d.seen, 8, d.returns, d.rescaled, d.adv,
                                  d.stats, d.status, 0)


def _head_launch(rlx, dev, logits, actions, adv, beta, T, ld=None):
    import torch
    rows, A = logits.shape
    ld = A if ld is None else ld
    buf = np.full((rows, ld), np.nan, np.float32)
    buf[:, :A] = logits
    d = torch.full((rows, ld), float("nan"), dtype=torch.float32, device=dev)
    sc = torch.full((2,), float("nan"), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rlx.pg_head_loss(_t(buf, dev), ld, _t(np.asarray(actions, np.int32), dev), _t(np.asarray(adv, np.float32), dev),
                     float(beta), rows, T, A, d, ld, sc, status, 0)
    torch.cuda.synchronize()
    out = d.cpu().numpy()
    assert np.isnan(out[:, A:]).all()                              # nothing is written beside the A columns
    return dict(loss=sc.cpu().numpy()[0], entropy=sc.cpu().numpy()[1], dlogits=out[:, :A], status=int(status.item()))


@pytest.mark.parametrize("beta", [0.0, 0.01])
@pytest.mark.parametrize("A", [1, 2, 6, 18])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 200, 255, 256, 257])
def test_head_loss_kernel_equals_the_restatement(rlx, dev, T, A, beta):
    """T around the wave (64) and around the workgroup's 256 threads, where a thread starts to own a second row; a
    non-unit leading dimension and two padded rows (NaN logits: they must not be read) in every case; a saturated row"""
    rng = np.random.RandomState(T * 100 + A)
    pad = 2
    logits = (rng.randn(T + pad, A) * 2).astype(np.float32)
    if A > 1:
        logits[0] = -30.0
        logits[0, A - 1] = 30.0                                    # one logit 60 above the rest: p + eps matters
    logits[T:] = np.nan
    actions = rng.randint(0, A, size=T)
    actions[0] = 0                                                 # ... and the taken action is a saturated-away one
    adv = rng.randn(T).astype(np.float32)
    k = _head_launch(rlx, dev, logits, actions, adv, beta, T, ld=A + 3)
    r = R.head_loss(np.nan_to_num(logits), actions, adv, beta, T=T)
    print("\n  T %d A %d beta %g: loss %.6g (twin %.6g), entropy %.6g (twin %.6g), max |dlogits - twin| %.2e" % (
        T, A, beta, k["loss"], r["loss"], k["entropy"], r["entropy"], np.abs(k["dlogits"] - r["dlogits"]).max()))
    assert k["status"] == 0
    np.testing.assert_allclose(k["loss"], r["loss"], **LOSS)
    np.testing.assert_allclose(k["entropy"], r["entropy"], **LOSS)
    np.testing.assert_allclose(k["dlogits"], r["dlogits"], **OUT)
    assert np.all(k["dlogits"][T:] == 0.0)                         # a padded row contributes exactly zero
    if A > 1:
        assert np.any(k["dlogits"][0] != 0.0) and np.isfinite(k["dlogits"]).all()
        # the saturated row's log pi(a) is log(eps / (1 + A eps)), not -inf
        p, q, S, lp, H = R.head_rows(logits[:1])
        assert p[0, 0] < 1e-20 and np.isfinite(lp[0, 0]) and lp[0, 0] < -15
    else:
        assert np.all(k["dlogits"] == 0.0) and k["entropy"] == 0.0
    again = _head_launch(rlx, dev, logits, actions, adv, beta, T, ld=A + 3)
    assert again["loss"].tobytes() == k["loss"].tobytes() and again["dlogits"].tobytes() == k["dlogits"].tobytes()
    # the padding does not change the window's loss or gradient
    bare = _head_launch(rlx, dev, logits[:T], actions, adv, beta, T)
    assert bare["loss"].tobytes() == k["loss"].tobytes() and bare["dlogits"].tobytes() == k["dlogits"][:T].tobytes()


def test_head_loss_flags_an_action_out_of_range_and_refuses_bad_shapes(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    rng = np.random.RandomState(2)
    logits = rng.randn(5, 3).astype(np.float32)
    actions = np.array([0, 3, 1, -1, 2])
    adv = rng.randn(5).astype(np.float32)
    k = _head_launch(rlx, dev, logits, actions, adv, 0.01, 5)
    r = R.head_loss(logits, actions, adv, 0.01)
    assert k["status"] == 1 and r["status"] == 1
    assert np.all(k["dlogits"][[1, 3]] == 0) and np.any(k["dlogits"][0] != 0)
    np.testing.assert_allclose(k["loss"], r["loss"], **LOSS)
    np.testing.assert_allclose(k["dlogits"], r["dlogits"], **OUT)
    big = torch.zeros(4, 32, dtype=torch.float32, device=dev)
    it = torch.zeros(4, dtype=torch.int32, device=dev)
    for rows, T, A, ld in ((4, 4, 19, 32), (4, 4, 0, 32), (4, 0, 2, 32), (3, 4, 2, 32), (4, 4, 6, 5)):
        with pytest.raises(RlxError):
            rlx.pg_head_loss(big, ld, it, big, 0.0, rows, T, A, big, ld, big, it, 0)


def test_action_entropy_equals_the_reference_formula(rlx, dev):
    import torch
    rng = np.random.RandomState(3)
    p = rng.dirichlet(np.ones(6), size=70).astype(np.float32)
    p[0] = [1, 0, 0, 0, 0, 0]                                      # log(0 + eps): finite
    out = torch.zeros(70, dtype=torch.float32, device=dev)
    rlx.action_entropy(_t(p, dev), 6, 70, 6, out, 0)
    ref = -np.sum(p * np.log(p + R.EPS), axis=1)                   # policy_optimization_agent.py:154
    assert ref.dtype == np.float32
    np.testing.assert_allclose(out.cpu().numpy(), ref, **OUT)
    np.testing.assert_allclose(out.cpu().numpy(), R.action_entropy(p), rtol=1e-6, atol=1e-7)


def _oracle_for(net, obs_shape, lr, eps):
    """the oracle's DQN chain (embedder, middleware, one Dense head) on the policy network's weights"""
    from oracle.agents import DQNOracle
    arrays = {k.replace("main/policy_values_head/fc", "main/q_head/dense"): v
              for k, v in net.params.named_arrays().items()}
    return DQNOracle(arrays, obs_shape, net.A, lr=lr, eps=eps)


def test_network_update_equals_the_composed_oracle(dev):
    """PolicyGradientNet: forward, head loss, backward, accumulation over three windows of different lengths, one Adam
    step — twice — against oracle layers + TF1 Adam + the restatement, in the manner and at the tolerances of
    test_c51.py::test_network_update_equals_the_composed_oracle (vector observations, CartPole's shape)."""
    import torch
    from coach_amd.nn.networks import PolicyGradientNet
    rng = np.random.RandomState(7)
    A, lr, beta = 2, 5e-4, 0.01
    net = PolicyGradientNet(dev, (4,), A, learning_rate=lr, optimizer_epsilon=1e-4, beta_entropy=beta, seed=3)
    assert "main/policy_values_head/fc/kernel" in net.params.entries and net.target is None
    o = _oracle_for(net, (4,), lr, 1e-4)
    for step in range(2):
        w0 = net.params.weights.clone()
        shards, acc_before = [], None
        for i, T in enumerate((9, 1, 37)):
            obs = rng.randn(T, 4).astype(np.float32)
            actions = rng.randint(0, A, size=T)
            adv = rng.randn(T).astype(np.float32)
            loss = net.accumulate_window(_t(obs, dev), T, _t(actions.astype(np.int32), dev), _t(adv, dev))
            r = R.head_loss(o.q(obs).astype(np.float32), actions, adv, beta)
            o.tower.backward(o.head.backward(r["dlogits"]))
            shards.append(o.snapshot_grads())
            np.testing.assert_allclose(float(loss.item()), r["loss"], **LOSS)
            np.testing.assert_allclose(float(net.entropy.item()), r["entropy"], **LOSS)
            np.testing.assert_allclose(float(net.norm.item()), o.global_norm(), **LOSS)
            # a second window ADDS to the accumulated gradient: accumulated == previous + this window's, bit for bit
            expect = net.params.grads.clone() if acc_before is None else acc_before + net.params.grads
            assert torch.equal(net.accumulated, expect) and net.accumulated.abs().sum() > 0
            acc_before = net.accumulated.clone()
            assert torch.equal(net.params.weights, w0)               # nothing is applied while accumulating
        net.apply_accumulated()
        o.apply_summed_gradients(shards, 1, False)
        assert not net.accumulated.any() and not torch.equal(net.params.weights, w0)      # applying resets
        net.check_status()
        w = net.params.named_arrays()
        wo = {k.replace("main/q_head/dense", "main/policy_values_head/fc"): v for k, v in o.weights().items()}
        assert set(wo) == set(w)
        for name, towers in wo.items():
            np.testing.assert_allclose(w[name][0], towers[0], err_msg=name, **WEIGHTS)
    assert torch.isfinite(net.params.weights).all()


def test_backend_interface_serves_the_policy_gradient_network(dev):
    """Architecture.predict / accumulate_gradients / apply_gradients through a NetworkWrapper, fed the way
    PolicyGradientsAgent.learn_from_batch feeds it (policy_gradients_agent.py:128-130), against the same network driven
    directly: identical weights after two accumulated windows and one applied step."""
    import torch
    from coach_amd.agents.policy_gradients_agent import PolicyGradientsAgentParameters
    from coach_amd.architectures.hip_architecture import PolicyGradientArchitecture
    from coach_amd.architectures.network_wrapper import NetworkWrapper
    from coach_amd.nn.networks import PolicyGradientNet, policy_gradient_net_kwargs
    from coach_amd.spaces import BoxActionSpace, DiscreteActionSpace, ObservationSpace, SpacesDefinition, StateSpace
    ap = PolicyGradientsAgentParameters()
    ap.seed = 5
    ap.algorithm.beta_entropy = 0.01
    A = 3
    spaces = SpacesDefinition(StateSpace({"observation": ObservationSpace((6,))}), None, DiscreteActionSpace(A))
    nw = NetworkWrapper(ap, has_target=False, has_global=False, name="main", spaces=spaces, worker_device=dev)
    online = nw.online_network
    assert isinstance(online, PolicyGradientArchitecture) and nw.target_network is None
    twin = PolicyGradientNet(dev, (6,), A, **policy_gradient_net_kwargs(ap.network_wrappers["main"], ap.algorithm, 5))
    assert torch.equal(twin.params.weights, online.net.params.weights)
    rng = np.random.RandomState(1)
    obs = rng.randn(4, 6).astype(np.float32)
    probs = online.predict({"observation": obs})
    z = twin.policy_values(_t(obs, dev), 4, tag="p").data.view(4, A).cpu().numpy()
    assert probs.shape == (4, A)
    np.testing.assert_allclose(probs, R.head_rows(z)[0], **OUT)
    w0 = online.net.params.weights.clone()
    for T in (7, 2):
        obs, actions = rng.randn(T, 6).astype(np.float32), rng.randint(0, A, size=T)
        targets = rng.randn(T)                                    # fp64, as learn_from_batch hands them over
        total_loss, losses, norm = online.accumulate_gradients({"observation": obs, "output_0_0": actions}, targets)[:3]
        twin.accumulate_window(_t(obs, dev), T, _t(actions.astype(np.int32), dev), _t(targets.astype(np.float32), dev))
        assert total_loss == float(twin.loss.item()) and losses == [total_loss] and norm == float(twin.norm.item())
        assert torch.equal(online.accumulated_gradients, twin.accumulated)
    assert torch.equal(online.net.params.weights, w0)
    nw.apply_gradients_and_sync_networks()
    twin.apply_accumulated()
    assert torch.equal(online.net.params.weights, twin.params.weights) and not torch.equal(twin.params.weights, w0)
    assert not online.accumulated_gradients.any()
    with pytest.raises(ValueError, match="continuous PolicyHead"):
        box = SpacesDefinition(StateSpace({"observation": ObservationSpace((6,))}), None,
                               BoxActionSpace(2, low=-1.0, high=1.0))
        NetworkWrapper(ap, has_target=False, has_global=False, name="main", spaces=box, worker_device=dev)


def _agent(dev, n_env, t_max, rescaler=None, seed=3):
    from coach_amd.agents.policy_gradients_agent import PolicyGradientsAgent, PolicyGradientsAgentParameters
    from coach_amd.core_types import RunPhase
    from coach_amd.environments.cartpole_vector_environment import (
        CartPoleVectorEnvironment, CartPoleVectorEnvironmentParameters)
    p = PolicyGradientsAgentParameters()
    p.seed = seed
    p.algorithm.num_steps_between_gradient_updates = t_max
    p.algorithm.reward_rescale = 1 / 200.
    if rescaler is not None:
        p.algorithm.policy_gradient_rescaler = rescaler
    env = CartPoleVectorEnvironment(CartPoleVectorEnvironmentParameters(n_env, "CartPole-v0", seed=11), dev)
    agent = PolicyGradientsAgent(p, env, dev)
    agent.phase = env.phase = RunPhase.TRAIN
    agent.debug_windows = []
    return agent


def _step(agent, episodes, limit=4000):
    """act() + train() until `episodes` episodes finished -> per env the finished episodes' lengths, and for every
    train() call the windows it made and whether the weights / the accumulated gradient changed"""
    import torch
    net = agent.networks["main"]
    lengths = [[] for _ in range(agent.n_env)]
    calls, done = [], 0
    for _ in range(limit):
        agent.act()
        if agent._episode_just_ended:
            for e, L in zip(np.nonzero(agent._episode_steps == 0)[0], agent.ended_episode_lengths):
                lengths[e].append(int(L))
                done += 1
        w0, n0 = net.params.weights.clone(), len(agent.debug_windows)
        agent.train()
        calls.append(dict(windows=agent.debug_windows[n0:], moved=not torch.equal(net.params.weights, w0),
                          accumulated=bool(net.accumulated.any())))
        if done >= episodes:
            break
    agent.check_status()
    return lengths, calls


@pytest.mark.parametrize("t_max", [20000, 5])
def test_agent_with_one_env_keeps_the_reference_cadence(dev, t_max):
    """windows, current_episode, training_iteration and the apply cadence of the stepped agent are those of
    PolicyOptimizationAgent.train as tests/pg_ref.py restates it (pinned to the reference by the fixture), and the
    device's per-timestep statistics after the run are the restatement's bit for bit"""
    agent = _agent(dev, 1, t_max)
    lengths, calls = _step(agent, 12)
    rewards = [np.full(L, np.float32(1.0) * np.float32(1 / 200.), np.float32) for L in lengths[0]]
    stats = R.Statistics(200)
    ws = R.run(rewards, 0.99, R.FUTURE_RETURN_NORMALIZED_BY_TIMESTEP, 200, t_max, 5, stats=stats)
    got = agent.debug_windows
    assert [(s, e, ce, ap) for _, s, e, ce, ap in got] == \
        [(w["start"], w["end"], w["current_episode"], w["applied"]) for w in ws]
    assert agent.training_iteration == len(ws) == ws[-1]["training_iteration"] and agent.current_episode == 12
    assert any(ap for *_, ap in got) and not all(ap for *_, ap in got)
    assert (t_max == 5) == any(s > 0 for _, s, *_ in got)
    # the weights move only in train() calls that applied (the first episode's windows, current_episode 0 with
    # t_max = 5, apply an exactly zero gradient), and applying clears the accumulated gradient
    assert any(c["moved"] for c in calls)
    for c in calls:
        applied = any(ap for *_, ap in c["windows"])
        assert applied or not c["moved"]
        if applied and c["windows"][0][3] >= 5:
            assert c["moved"]
        if c["windows"] and c["windows"][-1][-1]:
            assert not c["accumulated"]
    # (the very first episode is its own baseline: advantages and gradient are exactly zero)
    assert any(c["accumulated"] for c in calls if c["windows"] and not c["windows"][-1][-1])
    assert np.array_equal(BITS64(agent.mean_return_over_multiple_episodes.cpu().numpy()), BITS64(stats.mean))
    assert np.array_equal(BITS64(agent.num_episodes_where_step_has_been_seen.cpu().numpy()), BITS64(stats.seen))
    assert stats.seen.max() >= 12 and stats.mean.any()


def test_agent_with_three_envs_processes_windows_in_env_order(dev):
    """each env's windows are what its own single-env run gives for the same episode lengths; windows of one vector step
    come in env order; the envs share the episode counter and the per-timestep statistics"""
    agent = _agent(dev, 3, 5, seed=4)
    lengths, calls = _step(agent, 15)
    got = agent.debug_windows
    for e in range(3):
        eps = lengths[e] + [200]          # the env's running episode (unknown length: long enough not to end)
        ws = R.run([np.zeros(L, np.float32) for L in eps], 0.99, R.FUTURE_RETURN, 200, 5, 5)
        mine = [(s, t) for env, s, t, *_ in got if env == e]
        assert mine == [(w["start"], w["end"]) for w in ws][:len(mine)] and len(mine) >= len(lengths[e])
    for c in calls:
        envs = [w[0] for w in c["windows"]]
        assert envs == sorted(envs) and len(set(envs)) == len(envs)
    assert any(len(c["windows"]) > 1 for c in calls)
    ce = [w[3] for w in got]
    assert ce == sorted(ce) and agent.current_episode == sum(len(x) for x in lengths)
    assert agent.training_iteration == len(got)
    # the shared statistics: the windows replayed in the recorded order through the restatement
    stats = R.Statistics(200)
    for env, s, t, *_ in got:
        R.window(np.full(t, np.float32(1.0) * np.float32(1 / 200.), np.float32), s, 0.99,
                 R.FUTURE_RETURN_NORMALIZED_BY_TIMESTEP, stats)
    assert np.array_equal(BITS64(agent.mean_return_over_multiple_episodes.cpu().numpy()), BITS64(stats.mean))
    assert np.array_equal(BITS64(agent.num_episodes_where_step_has_been_seen.cpu().numpy()), BITS64(stats.seen))


def test_cartpole_pg_preset_reaches_the_golden_threshold(dev, tmp_path):
    """presets/CartPole_PG.py:42-45: min_reward_threshold 130 within max_episodes_to_achieve_reward 550, with the agent
    seed 0 the reference's golden tests use.  Stops when the bar is reached."""
    from test_cartpole import _golden
    st = _golden(dev, "CartPole_PG", tmp_path)
    assert st["passed"], st
