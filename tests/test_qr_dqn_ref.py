"""Quantile-Regression DQN on the CPU: the numpy restatement (tests/qr_dqn_ref.py) against what the reference's own
QuantileRegressionDQNAgent computed (tests/golden/qr_dqn.npz, make_golden_qr_dqn.py), its loss and gradient against a
torch-autograd transcription of the TF head (heads/quantile_regression_q_head.py:55-74), the package's parameter
defaults and its CartPole_QR_DQN preset against the reference's (tests/golden/qr_dqn_preset.json)."""
import importlib
import json
import os

import numpy as np
import pytest

import qr_dqn_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = ((32, 2, 50), (37, 6, 200), (5, 18, 1))


@pytest.fixture(scope="module")
def qr():
    return np.load(os.path.join(GOLDEN, "qr_dqn.npz"))


@pytest.mark.parametrize("s", range(len(SHAPES)))
def test_targets_and_midpoints_equal_the_reference_agent_bit_for_bit(qr, s):
    p = "s%d_" % s
    theta, theta_next, actions = qr[p + "theta"], qr[p + "theta_next"], qr[p + "actions"]
    B, A, N = SHAPES[s]
    assert theta.shape == (B, A, N)
    a_star, T, tau, loss, d = R.update(theta, theta_next, actions, qr[p + "rewards"], qr[p + "go"],
                                       float(qr[p + "discount"]), 1.0)
    # the reference hands fp64 targets / midpoints to fp32 placeholders: compare after that one rounding
    assert np.array_equal(T.view(np.uint32), qr[p + "targets"].astype(np.float32).view(np.uint32))
    assert np.array_equal(tau.view(np.uint32), qr[p + "midpoints"].astype(np.float32).view(np.uint32))
    assert qr[p + "locations"].tolist() == [[b, int(a)] for b, a in enumerate(actions)]
    # the quirk: tau is indexed by the argsort itself, which is not the rank unless the permutation is an involution
    if N > 2:
        taken = theta[np.arange(B), actions]
        mid = (np.arange(N) + 0.5) / N
        by_rank = mid[np.argsort(np.argsort(taken, axis=1), axis=1)].astype(np.float32)
        assert not np.array_equal(tau, by_rank)
    assert np.all(d[np.arange(B), actions] == d[np.arange(B), actions]) and np.isfinite(loss)
    off = np.ones((B, A), bool)
    off[np.arange(B), actions] = False
    assert np.all(d[off] == 0)


@pytest.mark.parametrize("s", range(3))
def test_acting_q_values_equal_the_reference_and_the_device_order_agrees_to_4_ulp(qr, s):
    x, q = qr["act%d_quantiles" % s], qr["act%d_q" % s]
    assert q.dtype == np.float64
    assert np.array_equal(R.q_values(x), q)
    # ulps of the atoms' mean magnitude: a mean near zero from atoms near one carries their rounding, not its own
    dev = R.q_values_device_order(x)
    assert np.all(np.abs(dev - q) <= 4 * np.spacing(np.abs(x.astype(np.float64)).mean(-1)))
    assert q[-1, 0] == q[-1, -1]                       # the exact tie the fixture holds


def _torch_head_loss(theta_taken, T, tau, kappa):
    """heads/quantile_regression_q_head.py:55-74, line by line, in torch (fp64)."""
    import torch
    th = torch.tensor(theta_taken, dtype=torch.float64, requires_grad=True)
    N = th.shape[1]
    theta_i = th.unsqueeze(-1).expand(-1, -1, N)
    T_theta_j = torch.tensor(T, dtype=torch.float64).unsqueeze(-2).expand(-1, N, -1)
    tau_i = torch.tensor(tau, dtype=torch.float64).unsqueeze(-1).expand(-1, -1, N)
    error = T_theta_j - theta_i
    abs_error = torch.abs(error)
    quadratic = torch.clamp(abs_error, max=kappa)
    huber = kappa * (abs_error - quadratic) + 0.5 * quadratic ** 2
    qh = torch.abs(tau_i - (error < 0).to(torch.float64)) * huber
    loss = qh.sum() / float(N)
    loss.backward()
    return loss.item(), th.grad.numpy()


@pytest.mark.parametrize("kappa", [1.0, 0.5])
@pytest.mark.parametrize("s", range(len(SHAPES)))
def test_loss_and_gradient_equal_autograd_of_the_tf_head(qr, s, kappa):
    pytest.importorskip("torch")
    p = "s%d_" % s
    theta, actions = qr[p + "theta"], qr[p + "actions"]
    B = theta.shape[0]
    _, T = R.targets(qr[p + "theta_next"], qr[p + "rewards"], qr[p + "go"], 0.99)
    taken = theta[np.arange(B), actions]
    tau = R.midpoints(taken)
    loss, g = R.loss_and_grad(taken, T, tau, kappa, dtype=np.float64)
    tl, tg = _torch_head_loss(taken, T, tau, kappa)
    np.testing.assert_allclose(loss, tl, rtol=1e-12)
    np.testing.assert_allclose(g, tg, rtol=1e-12, atol=1e-15)
    # and the fp32 restatement the device test compares against is that loss to fp32 accumulation
    l32, g32 = R.loss_and_grad(taken, T, tau, kappa)
    np.testing.assert_allclose(l32, tl, rtol=2e-4)
    np.testing.assert_allclose(g32, tg, rtol=1e-4, atol=2e-6)


def test_egreedy_restatement_uses_fp64_isclose():
    q = np.array([[1.0, 1.0 + 1e-6, 0.5], [2.0, 1.0, 2.0]])
    tie = np.array([[0.9, 0.1, 0.99], [0.2, 0.7, 0.3]])
    assert R.egreedy(q, [1.0, 1.0], [0, 0], tie, 0.5).tolist() == [0, 2]
    assert R.egreedy(q, [0.1, 1.0], [2, 0], tie, 0.5).tolist() == [2, 2]


def test_parameter_defaults_equal_the_reference(qr):
    from coach_amd.agents.qr_dqn_agent import QuantileRegressionDQNAgentParameters
    ref = json.loads(str(qr["defaults"]))
    ap = QuantileRegressionDQNAgentParameters()
    net = ap.network_wrappers["main"]
    sch = ap.exploration.epsilon_schedule
    mine = {"atoms": ap.algorithm.atoms, "huber_loss_interval": ap.algorithm.huber_loss_interval,
            "discount": ap.algorithm.discount, "learning_rate": net.learning_rate,
            "optimizer_epsilon": net.optimizer_epsilon, "batch_size": net.batch_size,
            "head": type(net.heads_parameters[0]).__name__,
            "epsilon_schedule": [type(sch).__name__, float(sch.initial_value), float(sch.final_value),
                                 int(sch.decay_steps)],
            "evaluation_epsilon": ap.exploration.evaluation_epsilon,
            "num_steps_between_copying_online_weights_to_target":
                ap.algorithm.num_steps_between_copying_online_weights_to_target.num_steps,
            "memory": type(ap.memory).__name__}
    assert mine == ref
    assert ap.path == "coach_amd.agents.qr_dqn_agent:QuantileRegressionDQNAgent"


def test_package_preset_equals_the_unchanged_reference_preset_text():
    """tests/golden/qr_dqn_preset.json holds what the reference's CartPole_QR_DQN.py text, executed unchanged through the
    import layer, set (make_qr_dqn_preset_dump.py): the package's preset must equal it field by field."""
    from test_cartpole import _dump
    with open(os.path.join(GOLDEN, "qr_dqn_preset.json")) as f:
        ref = json.load(f)["CartPole_QR_DQN"]
    mine = importlib.import_module("coach_amd.presets.CartPole_QR_DQN").graph_manager
    assert ref["level_name"] == "CartPole-v0" and mine.env_params.level == "CartPole-v0"
    for part in ("agent_params", "schedule", "preset_validation_params"):
        assert ref[part] == _dump(getattr(mine, part)), part
    v = mine.preset_validation_params
    assert v.test and v.min_reward_threshold == 150 and v.max_episodes_to_achieve_reward == 250
    assert mine.agent_params.algorithm.atoms == 50 and mine.agent_params.network_wrappers["main"].learning_rate == 5e-4


def test_rainbow_stub_is_importable_and_refuses():
    from coach_amd.agents.rainbow_dqn_agent import RainbowDQNAgentParameters
    with pytest.raises(NotImplementedError):
        RainbowDQNAgentParameters()
