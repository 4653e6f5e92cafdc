"""N-step Q on the device: rlx_nstep_q_window_loss (csrc/n_step_q.hip) against the numpy restatement
(tests/n_step_q_ref.py, itself pinned to the reference agent by tests/test_n_step_q_ref.py), against the reference
agent's own target matrix (tests/golden/n_step_q.npz) and against rlx_regression_loss fed that matrix; the network update
against the oracle's layers + TF1 Adam composed with the restatement; the agent's target copies, windows, targets and
cadence on the device CartPole; the backend interface and the CartPole_NStepQ preset.

Tolerances.  The launch is compared with the restatement BIT FOR BIT on every output: the targets are restated
operation by operation with their fp32 / fp64 rounding points, the head's row arithmetic is three fp32 operations, and
the batch sum is restated in the launch's own fixed order (a3c_ref.tree_sum).  The network update goes through GEMMs
whose fp32 summation order is a tuning parameter: it is compared under tests/tolerances.py's LOSS and WEIGHTS, as
test_a3c.py::test_network_update_equals_the_composed_oracle compares Actor-Critic's."""
import numpy as np
import pytest

import n_step_q_ref as R
import pg_ref
from test_n_step_q_ref import fixture_case
from tolerances import LOSS, OUT, WEIGHTS

pytestmark = pytest.mark.gpu

BITS32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
BIG = np.float32(3e38)           # padding of the target rows: a maximum that read it would show it (fmaxf skips a NaN)


def _t(x, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t if dtype is None else t.to(dtype)


def _launch(rlx, dev, q_online, q_target, actions, rewards, game_over, discount, horizon, huber=False, pad=3,
            given=None, with_td=True):
    """q_online [T, A], q_target [rows_t, A] or None -> every output of one launch.  Every matrix gets a leading
    dimension of its own with padding columns — NaN (BIG in the target rows) — which the launch must neither read nor
    write."""
    import torch
    T, A = q_online.shape
    ld_q, ld_t, ld_tt, ld_dq = A + pad, A + pad + 1, A + pad + 2, A + 2 * pad
    qb = np.full((T, ld_q), np.nan, np.float32)
    qb[:, :A] = q_online
    rows_t, tb = 0, None
    if q_target is not None:
        rows_t = len(q_target)
        tb = np.full((rows_t, ld_t), BIG, np.float32)
        tb[:, :A] = q_target
        tb = _t(tb, dev)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    dq, td, sc = nan(T, ld_dq), (nan(T, ld_tt) if with_td else None), nan(1)
    tgt = nan(T) if given is None else _t(np.asarray(given, np.float32), dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    go = _t(np.array([int(bool(game_over))], np.uint8), dev)
    rew = None if rewards is None else _t(np.asarray(rewards, np.float32), dev)
    rlx.nstep_q_window_loss(_t(qb, dev), ld_q, tb, ld_t, rows_t, _t(np.asarray(actions, np.int32), dev), rew, go, T, A,
                            float(discount), int(horizon), int(huber), tgt, td, ld_tt, dq, ld_dq, sc, status, 0)
    torch.cuda.synchronize()
    dq, sc, tgt = dq.cpu().numpy(), sc.cpu().numpy(), tgt.cpu().numpy()
    td = td.cpu().numpy() if with_td else None
    if int(status.item()) & R.STATUS_NO_TARGET_ROWS:
        assert np.isnan(dq).all() and np.isnan(sc).all() and np.isnan(tgt).all() and (td is None or np.isnan(td).all())
        return dict(status=int(status.item()))
    assert np.isnan(dq[:, A:]).all() and (td is None or np.isnan(td[:, A:]).all())
    return dict(targets=tgt, dq=dq[:, :A], td_targets=None if td is None else td[:, :A], loss=sc[0],
                status=int(status.item()))


def _assert_bit_equal(k, r, what=""):
    assert k["status"] == r["status"], what
    valid = r["valid"]
    assert np.array_equal(BITS32(k["targets"][valid]), BITS32(r["targets"][valid])), what
    assert np.isnan(k["targets"][~valid]).all(), what               # untouched
    assert np.array_equal(BITS32(k["dq"]), BITS32(r["dq"])), what
    if k["td_targets"] is not None:
        assert np.array_equal(BITS32(k["td_targets"]), BITS32(r["td_targets"])), what
    assert BITS32(k["loss"]) == BITS32(r["loss"]), (what, k["loss"], r["loss"])


def _window(T, A, seed):
    rng = np.random.RandomState(seed)
    q = (rng.randn(T, A) * 0.3).astype(np.float32)
    q_t = (rng.randn(T, A) * 0.3).astype(np.float32)
    actions = rng.randint(0, A, size=T)
    rewards = (rng.uniform(-1, 2, size=T).astype(np.float32) * np.float32(1 / 200.))
    q[0, actions[0]] += np.float32(3.0)                              # a row with |e| > 1: Huber's linear branch
    return q, q_t, actions, rewards


@pytest.mark.parametrize("A", [1, 2, 18])
@pytest.mark.parametrize("T", [1, 2, 5, 63, 64, 65, 200, 256, 257, 1025])
def test_window_loss_kernel_equals_the_restatement_bit_for_bit(rlx, dev, T, A):
    """T around the wave (64), one row per thread (<= 256), the strided rows and a second chunk of the recurrence
    (> 256); both horizons, bootstrapped and terminal, MSE and Huber; a row with |e| > 1; padding in every buffer; a
    terminal 'N-Step' window is launched with and without its target row."""
    q, q_t, actions, rewards = _window(T, A, T * 100 + A)
    for horizon, game_over, huber in [(h, g, u) for h in (R.N_STEP, R.ONE_STEP) for g in (False, True)
                                      for u in (False, True)]:
        what = "T %d A %d horizon %d game_over %d huber %d" % (T, A, horizon, game_over, huber)
        rows = q_t[:1] if horizon == R.N_STEP else q_t
        k = _launch(rlx, dev, q, rows, actions, rewards, game_over, 0.99, horizon, huber)
        r = R.window_loss(q, rows, actions, rewards, game_over, 0.99, horizon, huber)
        assert k["status"] == 0
        _assert_bit_equal(k, r, what)
        e = q[np.arange(T), actions] - r["targets"]
        assert abs(e[0]) > 1 and np.any(k["dq"] != 0)
        if game_over and horizon == R.N_STEP:
            bare = _launch(rlx, dev, q, None, actions, rewards, True, 0.99, horizon, huber)
            assert all(np.asarray(bare[n]).tobytes() == np.asarray(k[n]).tobytes() for n in k), what
    # the optional matrix changes nothing else, and a second launch gives the same bits
    first = _launch(rlx, dev, q, q_t, actions, rewards, False, 0.99, R.ONE_STEP)
    again = _launch(rlx, dev, q, q_t, actions, rewards, False, 0.99, R.ONE_STEP)
    bare = _launch(rlx, dev, q, q_t, actions, rewards, False, 0.99, R.ONE_STEP, with_td=False)
    assert all(np.asarray(again[n]).tobytes() == np.asarray(first[n]).tobytes() for n in again)
    assert all(np.asarray(bare[n]).tobytes() == np.asarray(first[n]).tobytes() for n in ("targets", "dq", "loss"))


def test_kernel_on_the_golden_cases_gives_the_reference_agents_matrix(rlx, dev, golden):
    """what the reference's own NStepQAgent.learn_from_batch handed to accumulate_gradients (and logged as 'Q Values'),
    bit for bit, fed the recorded stand-in networks' Q values"""
    z = golden("n_step_q")
    for c in (fixture_case(z, k) for k in range(int(z["n_cases"]))):
        k = _launch(rlx, dev, c["q_online"], c["q_target"], c["actions"], c["rewards"], c["game_over"], c["discount"],
                    c["horizon"])
        assert k["status"] == 0
        assert np.array_equal(BITS32(k["td_targets"]), BITS32(c["fed"]))
        assert np.array_equal(BITS32(k["td_targets"]), BITS32(c["q_values_signal"]))


@pytest.mark.parametrize("huber", [False, True])
@pytest.mark.parametrize("T,A", [(1, 2), (65, 6), (257, 18), (200, 1)])
def test_gradient_is_bit_identical_to_the_regression_loss_on_the_full_matrix(rlx, dev, T, A, huber):
    """rlx_regression_loss fed the full target matrix: the same dq bit for bit (the untouched columns give exactly
    zero); the loss scalars differ in the order of their sums only (LOSS)"""
    import torch
    q, q_t, actions, rewards = _window(T, A, T + A)
    k = _launch(rlx, dev, q, q_t[:1], actions, rewards, False, 0.99, R.N_STEP, huber, pad=0)
    g = torch.full((T, A), float("nan"), dtype=torch.float32, device=dev)
    sc = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    rlx.regression_loss(_t(q, dev), A, _t(k["td_targets"], dev), A, None, T, A, int(huber), 1.0, 1.0, g, A, sc, 0)
    assert g.cpu().numpy().tobytes() == k["dq"].tobytes()
    np.testing.assert_allclose(float(sc.item()), k["loss"], **LOSS)


def test_given_targets_are_read_not_computed(rlx, dev):
    """RLX_NSTEPQ_TARGETS_GIVEN: targets is an input; the target rows, the rewards and the game-over flag are not read"""
    rng = np.random.RandomState(8)
    T, A = 70, 3
    q, q_t, actions, _ = _window(T, A, 8)
    tgt = rng.randn(T).astype(np.float32)
    k = _launch(rlx, dev, q, np.full((T, A), np.nan, np.float32), actions, np.full(T, np.nan, np.float32), True, 0.99,
                R.TARGETS_GIVEN, given=tgt)
    bare = _launch(rlx, dev, q, None, actions, None, True, 0.99, R.TARGETS_GIVEN, given=tgt)
    r = R.head_loss(q, actions, tgt)
    assert k["status"] == 0 and np.array_equal(BITS32(k["targets"]), BITS32(tgt))
    _assert_bit_equal(k, dict(r, targets=tgt, valid=np.ones(T, bool)))
    assert all(np.asarray(bare[n]).tobytes() == np.asarray(k[n]).tobytes() for n in k)


def test_out_of_range_actions_missing_target_rows_and_bad_arguments(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    T, A = 5, 3
    q, q_t, _, rewards = _window(T, A, 2)
    actions = np.array([0, 3, 1, -1, 2])
    for horizon in (R.N_STEP, R.ONE_STEP):
        k = _launch(rlx, dev, q, q_t, actions, rewards, False, 0.99, horizon)
        r = R.window_loss(q, q_t, actions, rewards, False, 0.99, horizon)
        assert k["status"] == R.STATUS_BAD_ACTION == r["status"]
        assert np.all(k["dq"][[1, 3]] == 0) and np.any(k["dq"][0] != 0)
        _assert_bit_equal(k, r)
        # no term, and the mean still divides by T
        e = (q[[0, 2, 4], [0, 1, 2]] - k["targets"][[0, 2, 4]]).astype(np.float64)
        np.testing.assert_allclose(k["loss"], np.sum(e * e) / 5, **LOSS)
    # missing target rows: status, and nothing is written (the outputs stay NaN: _launch asserts it)
    ok = [0, 1, 2, 0, 1]
    assert _launch(rlx, dev, q, None, ok, rewards, False, 0.99, R.N_STEP)["status"] == R.STATUS_NO_TARGET_ROWS
    assert _launch(rlx, dev, q, q_t[:4], ok, rewards, False, 0.99, R.ONE_STEP)["status"] == R.STATUS_NO_TARGET_ROWS
    assert _launch(rlx, dev, q, q_t[:4], ok, rewards, True, 0.99, R.ONE_STEP)["status"] == R.STATUS_NO_TARGET_ROWS
    assert _launch(rlx, dev, q, None, ok, rewards, True, 0.99, R.ONE_STEP)["status"] == R.STATUS_NO_TARGET_ROWS
    assert _launch(rlx, dev, q, None, ok, rewards, True, 0.99, R.N_STEP)["status"] == 0
    f = torch.zeros(8, 32, dtype=torch.float32, device=dev)
    it = torch.zeros(8, dtype=torch.int32, device=dev)
    go = torch.zeros(1, dtype=torch.uint8, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(T=4, A=2, rows_t=4, horizon=R.ONE_STEP, ld_q=32, ld_t=32, ld_tt=32, ld_dq=32, q=f, q_t=f, rewards=f,
             game_over=go, targets=f, td=f, dq=f, scalars=f, status=st, actions=it):
        rlx.nstep_q_window_loss(q, ld_q, q_t, ld_t, rows_t, actions, rewards, game_over, T, A, 0.99, horizon, 0, targets,
                                td, ld_tt, dq, ld_dq, scalars, status, 0)
    call()
    call(td=None, ld_tt=0)
    call(horizon=R.TARGETS_GIVEN, q_t=None, rows_t=0, rewards=None, game_over=None)
    for kw in (dict(T=0), dict(T=-1), dict(A=0), dict(rows_t=-1), dict(ld_q=1), dict(ld_t=1), dict(ld_tt=1),
               dict(ld_dq=1), dict(q=None), dict(q_t=None), dict(actions=None), dict(rewards=None),
               dict(game_over=None), dict(targets=None), dict(dq=None), dict(scalars=None), dict(status=None),
               dict(horizon=2), dict(horizon=-2), dict(horizon=5)):
        with pytest.raises(RlxError):
            call(**kw)
    torch.cuda.synchronize()
    assert int(st.item()) == 0


def test_network_update_equals_the_composed_oracle(dev):
    """NStepQNet: the online forward on T rows, the target forward on one or T rows, the window launch, the head and
    the torso backward, accumulation over three windows of different lengths (both horizons, bootstrapped and
    terminal), one Adam step — twice — against oracle layers + TF1 Adam + the restatement, in the manner and at the
    tolerances of test_a3c.py::test_network_update_equals_the_composed_oracle.  The target copy is refreshed before
    each round, so the oracle's one set of weights serves both networks."""
    import torch
    from coach_amd.nn.networks import NStepQNet
    from oracle import nn as N
    from oracle.agents import DQNOracle
    rng = np.random.RandomState(7)
    A, lr = 2, 5e-4
    net = NStepQNet(dev, (4,), A, learning_rate=lr, optimizer_epsilon=1e-4, seed=3)
    assert "main/q_head/dense/kernel" in net.params.entries and net.target is not None
    assert net.clip_gradients is None and not net.huber
    o = DQNOracle(net.params.named_arrays(), (4,), A, lr=lr, eps=1e-4)
    cases = ((9, False, R.N_STEP), (1, True, R.ONE_STEP), (37, False, R.ONE_STEP), (6, True, R.N_STEP))
    for step in range(2):
        net.update_target(1.0)
        assert torch.equal(net.target, net.params.weights)
        w0 = net.params.weights.clone()
        shards, acc_before = [], None
        for T, game_over, horizon in cases:
            rows_t = 1 if horizon == R.N_STEP else T
            obs, nxt = rng.randn(T, 4).astype(np.float32), rng.randn(rows_t, 4).astype(np.float32)
            actions = rng.randint(0, A, size=T)
            rewards = rng.uniform(-1, 2, size=T).astype(np.float32)
            tgt = torch.zeros(T, dtype=torch.float32, device=dev)
            loss = net.accumulate_window(_t(obs, dev), T, _t(actions.astype(np.int32), dev), tgt, _t(nxt, dev), rows_t,
                                         _t(rewards, dev), _t(np.array([int(game_over)], np.uint8), dev), 0.99, horizon)
            q_t = o.head.forward(o.tower.forward(N.prep_obs(nxt, False))).astype(np.float32)
            q = o.head.forward(o.tower.forward(N.prep_obs(obs, False))).astype(np.float32)
            r = R.window_loss(q, q_t, actions, rewards, game_over, 0.99, horizon)
            o.tower.backward(o.head.backward(r["dq"]))
            shards.append(o.snapshot_grads())
            # the targets are formed from the device's own Q values: compared at the head's output tolerance
            np.testing.assert_allclose(net.q_online.cpu().numpy(), q, **OUT)
            np.testing.assert_allclose(net.q_target.cpu().numpy(), q_t, **OUT)
            np.testing.assert_allclose(tgt.cpu().numpy(), r["targets"], **OUT)
            np.testing.assert_allclose(net.td_targets.cpu().numpy(), r["td_targets"], **OUT)
            np.testing.assert_allclose(float(loss.item()), r["loss"], **LOSS)
            np.testing.assert_allclose(float(net.norm.item()), o.global_norm(), **LOSS)
            expect = net.params.grads.clone() if acc_before is None else acc_before + net.params.grads
            assert torch.equal(net.accumulated, expect) and net.accumulated.abs().sum() > 0
            acc_before = net.accumulated.clone()
            assert torch.equal(net.params.weights, w0)               # nothing is applied while accumulating
        net.apply_accumulated()
        o.apply_summed_gradients(shards, 1, False)
        assert not net.accumulated.any() and not torch.equal(net.params.weights, w0)
        assert torch.equal(net.target, w0)                           # the target copy stays until it is refreshed
        net.check_status()
        w, wo = net.params.named_arrays(), o.weights()
        assert set(wo) == set(w)
        for name, towers in wo.items():
            np.testing.assert_allclose(w[name][0], towers[0], err_msg=name, **WEIGHTS)
    assert torch.isfinite(net.params.weights).all()


def test_huber_and_clipping_come_from_the_wrapper(dev):
    """replace_mse_with_huber_loss and clip_gradients of the network parameters reach the launch and the clip"""
    import torch
    from coach_amd.agents.n_step_q_agent import NStepQNetworkParameters
    from coach_amd.nn.networks import NStepQNet, n_step_q_net_kwargs
    np_ = NStepQNetworkParameters()
    np_.replace_mse_with_huber_loss, np_.clip_gradients = True, 0.01
    net = NStepQNet(dev, (4,), 3, **n_step_q_net_kwargs(np_, 2))
    assert net.huber and net.clip_gradients == 0.01
    rng = np.random.RandomState(3)
    T = 6
    obs, nxt = rng.randn(T, 4).astype(np.float32), rng.randn(1, 4).astype(np.float32)
    actions, rewards = rng.randint(0, 3, size=T), np.full(T, 5.0, np.float32)           # |e| > 1 on every row
    tgt = torch.zeros(T, dtype=torch.float32, device=dev)
    net.window_gradients(_t(obs, dev), T, _t(actions.astype(np.int32), dev), tgt, _t(nxt, dev), 1, _t(rewards, dev),
                         _t(np.array([0], np.uint8), dev), 0.99, R.N_STEP)
    r = R.window_loss(net.q_online.cpu().numpy(), net.q_target.cpu().numpy(), actions, rewards, False, 0.99, R.N_STEP,
                      huber=True)
    assert BITS32(net.loss.cpu().numpy())[0] == BITS32(r["loss"]) and np.array_equal(tgt.cpu().numpy(), r["targets"])
    norm = float(net.norm.item())
    assert norm > 0.01                                               # the raw norm is reported, the buffer is clipped
    np.testing.assert_allclose(float(net.params.grads.double().norm().item()), 0.01, rtol=1e-4)
    net.check_status()


def test_backend_interface_serves_the_n_step_q_network(dev):
    """Architecture.predict / accumulate_gradients / apply_gradients through a NetworkWrapper with a target network, fed
    the way NStepQAgent.learn_from_batch feeds it (n_step_q_agent.py:104-134), against the same network driven directly
    through the window launch: the same gradient bit for bit, identical weights after two accumulated windows and one
    applied step."""
    import torch
    from coach_amd.agents.n_step_q_agent import NStepQAgentParameters
    from coach_amd.architectures.hip_architecture import NStepQArchitecture
    from coach_amd.architectures.network_wrapper import NetworkWrapper
    from coach_amd.nn.networks import NStepQNet, n_step_q_net_kwargs
    from coach_amd.spaces import BoxActionSpace, DiscreteActionSpace, ObservationSpace, SpacesDefinition, StateSpace
    ap = NStepQAgentParameters()
    ap.seed = 5
    A = 3
    spaces = SpacesDefinition(StateSpace({"observation": ObservationSpace((6,))}), None, DiscreteActionSpace(A))
    nw = NetworkWrapper(ap, has_target=True, has_global=False, name="main", spaces=spaces, worker_device=dev)
    online, target = nw.online_network, nw.target_network
    assert isinstance(online, NStepQArchitecture) and isinstance(target, NStepQArchitecture) and target.net is online.net
    twin = NStepQNet(dev, (6,), A, **n_step_q_net_kwargs(ap.network_wrappers["main"], 5))
    assert torch.equal(twin.params.weights, online.net.params.weights)
    rng = np.random.RandomState(1)
    w0 = online.net.params.weights.clone()
    for T in (7, 2):
        obs, nxt = rng.randn(T, 6).astype(np.float32), rng.randn(T, 6).astype(np.float32)
        actions, rewards = rng.randint(0, A, size=T), rng.uniform(-1, 2, size=T).astype(np.float32)
        # learn_from_batch '1-Step' on the host, with the types numpy >= 2 gives the reference's line (:112-114)
        matrix = online.predict({"observation": obs})
        q_next = target.predict({"observation": nxt})
        assert matrix.shape == (T, A) and matrix.dtype == np.float32 and q_next.shape == (T, A)
        assert np.array_equal(matrix, twin.q_values(_t(obs, dev), T, tag="check").data.view(T, A).cpu().numpy())
        for i in reversed(range(T)):
            matrix[i][actions[i]] = np.float64(rewards[i]) + np.float64(1.0 - 0.0) * 0.99 * np.float64(np.max(q_next[i], 0))
        total_loss, losses, norm = online.accumulate_gradients({"observation": obs}, [matrix])[:3]
        tgt = torch.zeros(T, dtype=torch.float32, device=dev)
        twin.accumulate_window(_t(obs, dev), T, _t(actions.astype(np.int32), dev), tgt, _t(nxt, dev), T, _t(rewards, dev),
                               _t(np.array([0], np.uint8), dev), 0.99, R.ONE_STEP)
        assert np.array_equal(BITS32(twin.td_targets.cpu().numpy()), BITS32(matrix))
        np.testing.assert_allclose(total_loss, float(twin.loss.item()), **LOSS)          # the sums' orders differ
        assert losses == [total_loss] and norm == float(twin.norm.item())
        assert torch.equal(online.accumulated_gradients, twin.accumulated)
    assert torch.equal(online.net.params.weights, w0)
    nw.apply_gradients_and_sync_networks()
    twin.apply_accumulated()
    assert torch.equal(online.net.params.weights, twin.params.weights) and not torch.equal(twin.params.weights, w0)
    assert not online.accumulated_gradients.any()
    # the target view still answers with the old weights until it is updated
    obs = rng.randn(3, 6).astype(np.float32)
    assert not np.array_equal(target.predict({"observation": obs}), online.predict({"observation": obs}))
    nw.update_target_network()
    assert np.array_equal(target.predict({"observation": obs}), online.predict({"observation": obs}))
    with pytest.raises(ValueError, match="Box action space"):
        box = SpacesDefinition(StateSpace({"observation": ObservationSpace((6,))}), None,
                               BoxActionSpace(2, low=-1.0, high=1.0))
        NetworkWrapper(ap, has_target=True, has_global=False, name="main", spaces=box, worker_device=dev)


def _agent(dev, n_env, t_max, horizon, seed=3, copy_every=100, apply_every=5):
    from coach_amd.agents.n_step_q_agent import NStepQAgent, NStepQAgentParameters
    from coach_amd.core_types import EnvironmentSteps, RunPhase
    from coach_amd.environments.cartpole_vector_environment import (
        CartPoleVectorEnvironment, CartPoleVectorEnvironmentParameters)
    p = NStepQAgentParameters()
    p.seed = seed
    p.algorithm.num_steps_between_gradient_updates = t_max
    p.algorithm.apply_gradients_every_x_episodes = apply_every
    p.algorithm.reward_rescale = 1 / 200.
    p.algorithm.targets_horizon = horizon
    p.algorithm.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(copy_every)
    env = CartPoleVectorEnvironment(CartPoleVectorEnvironmentParameters(n_env, "CartPole-v0", seed=11), dev)
    agent = NStepQAgent(p, env, dev)
    agent.phase = env.phase = RunPhase.TRAIN
    agent.debug_windows, agent.debug_targets = [], []
    return agent


def _assert_targets_are_the_restatement(agent, horizon):
    """every window's fp32 targets equal the restatement fed the device's own target-network rows, bit for bit; a
    finished episode's last transition is a game over (CartPole reports its limit as one), a running one's is not"""
    reward = np.float32(1.0) * np.float32(1 / 200.)
    h = R.HORIZONS[horizon]
    assert len(agent.debug_targets) == len(agent.debug_windows) > 0
    game_overs = []
    for (env, start, end, _, _), (q, q_t, tgt, actions, go) in zip(agent.debug_windows, agent.debug_targets):
        T = end - start
        q, q_t, go = q.cpu().numpy(), q_t.cpu().numpy(), bool(go.item())
        assert q.shape == (T, 2) and q_t.shape == ((1 if h == R.N_STEP else T), 2) and np.isfinite(q_t).all()
        want = R.window_targets(q_t, np.full(T, reward, np.float32), go, 0.99, h)
        assert np.array_equal(BITS32(tgt.cpu().numpy()), BITS32(want)), (env, start, end)
        assert actions.shape == (T,) and int(actions.min()) >= 0 and int(actions.max()) <= 1
        game_overs.append(go)
    return game_overs


@pytest.mark.parametrize("horizon", ["N-Step", "1-Step"])
@pytest.mark.parametrize("t_max", [5, 5000])
def test_agent_with_one_env_keeps_the_base_cadence_and_restated_targets(dev, t_max, horizon):
    """windows, pointers, current_episode, training_iteration and the apply cadence are the on-policy base's (pg_ref.run,
    pinned to the reference by PG's fixture: what test_a3c.py holds Actor-Critic to); every window's targets are the
    restatement's on the device's own target-network values"""
    from test_pg import _step
    agent = _agent(dev, 1, t_max, horizon)
    assert not agent.is_on_policy and type(agent.exploration_policy).__name__ == "EGreedy"
    lengths, calls = _step(agent, 12)
    ws = pg_ref.run([np.zeros(L, np.float32) for L in lengths[0]], 0.99, pg_ref.FUTURE_RETURN, 200, t_max, 5)
    got = agent.debug_windows
    assert [(s, e, ce, ap) for _, s, e, ce, ap in got] == \
        [(w["start"], w["end"], w["current_episode"], w["applied"]) for w in ws]
    assert agent.training_iteration == len(ws) == ws[-1]["training_iteration"] and agent.current_episode == 12
    assert any(ap for *_, ap in got) and not all(ap for *_, ap in got)
    assert (t_max == 5) == any(s > 0 for _, s, *_ in got)
    game_overs = _assert_targets_are_the_restatement(agent, horizon)
    assert game_overs == [w["complete"] for w in ws]
    assert any(c["moved"] for c in calls)
    for c in calls:
        applied = any(ap for *_, ap in c["windows"])
        assert applied == c["moved"]
        if c["windows"] and c["windows"][-1][-1]:
            assert not c["accumulated"]
    assert any(c["accumulated"] for c in calls if c["windows"] and not c["windows"][-1][-1])


def test_agent_with_three_envs_processes_windows_in_env_order(dev):
    """each env's windows are what its own single-env run gives for the same episode lengths; windows of one vector step
    come in env order; the envs share the episode counter; the targets of every env's windows are the restatement's"""
    from test_pg import _step
    agent = _agent(dev, 3, 5, "1-Step", seed=4)
    lengths, calls = _step(agent, 15)
    got = agent.debug_windows
    for e in range(3):
        eps = lengths[e] + [200]
        ws = pg_ref.run([np.zeros(L, np.float32) for L in eps], 0.99, pg_ref.FUTURE_RETURN, 200, 5, 5)
        mine = [(s, t) for env, s, t, *_ in got if env == e]
        assert mine == [(w["start"], w["end"]) for w in ws][:len(mine)] and len(mine) >= len(lengths[e])
    for c in calls:
        envs = [w[0] for w in c["windows"]]
        assert envs == sorted(envs) and len(set(envs)) == len(envs)
    assert any(len(c["windows"]) > 1 for c in calls)
    ce = [w[3] for w in got]
    assert ce == sorted(ce) and agent.current_episode == sum(len(x) for x in lengths)
    assert agent.training_iteration == len(got)
    game_overs = _assert_targets_are_the_restatement(agent, "1-Step")
    assert any(game_overs) and not all(game_overs)


def test_target_network_is_copied_every_k_environment_steps(dev):
    """EnvironmentSteps(k): train() copies first (the existing _should_update_online_weights_to_target on
    total_steps_counter), then runs the base's train().  After a call that copied, the target equals the online
    weights as they were BEFORE that call's apply, exactly; it differs from the online weights once they moved."""
    import torch
    k = 7
    agent = _agent(dev, 1, 5, "N-Step", copy_every=k, apply_every=1)
    net = agent.networks["main"]
    assert torch.equal(net.target, net.params.weights)
    copies_seen, differed = 0, False
    for step in range(1, 61):
        agent.act()
        before, n0 = net.params.weights.clone(), agent.target_copies
        agent.train()
        if agent.target_copies > n0:
            copies_seen += 1
            assert agent.target_copies == n0 + 1 and step % k == 0
            assert torch.equal(net.target, before)
            assert agent._target_updated_since_log
        moved = not torch.equal(net.params.weights, before)
        if moved:
            assert not torch.equal(net.target, net.params.weights)
            differed = True
    assert copies_seen == 60 // k == agent.target_copies and differed
    assert agent.last_target_network_update_step == (60 // k) * k
    agent.check_status()


def test_cartpole_n_step_q_preset_builds_and_runs_200_steps(dev, tmp_path):
    """nothing about learning is asserted (the recorded validation runs are in DESIGN.md): the preset builds, trains
    for 200 vector steps with finite weights, copies the target every 100 steps, and the agent's signals reach the CSV"""
    import importlib
    import torch
    from coach_amd.core_types import EnvironmentSteps, RunPhase
    gm = importlib.import_module("coach_amd.presets.CartPole_NStepQ").make()
    gm.schedule.improve_steps = EnvironmentSteps(200)
    gm.schedule.steps_between_evaluation_periods = EnvironmentSteps(100)
    gm.device = dev
    gm.logger.__init__(str(tmp_path / "nsq.csv"))
    rows = gm.improve()
    a = gm.agent
    assert type(a).__name__ == "NStepQAgent" and gm.total_steps_counters[RunPhase.TRAIN] == 200
    assert a.training_iteration >= 40 and sum(r.get("Evaluation Reward", "") != "" for r in rows) == 2
    assert a.target_copies == 2
    gm.environment.check_status()
    a.check_status()
    net = a.networks["main"]
    assert torch.isfinite(net.params.weights).all() and torch.isfinite(net.target).all()
    header = (tmp_path / "nsq.csv").read_text().splitlines()[0].split(",")
    for name in ("Q Values", "Value Loss", "Loss", "Grads (unclipped)", "Discounted Return"):
        assert name + "/Mean" in header, name
        values = [r[name + "/Mean"] for r in rows if r.get(name + "/Mean", "") != ""]
        assert values and np.isfinite(np.asarray(values, dtype=np.float64)).all(), name
    assert "Entropy/Mean" in header                                  # registered by the base, never sampled
    assert not [r for r in rows if r.get("Entropy/Mean", "") not in ("", "nan")]
    assert any(str(r.get("Update Target Network")) == "1" for r in rows)
