"""The recurrent Actor-Critic networks, agent and preset against an fp64 CPU torch restatement of the trunk (autograd)."""
import numpy as np
import pytest

import a3c_ref as R
from test_continuous_policy_head import window_ref
from tolerances import LOSS, OUT

pytestmark = pytest.mark.gpu

OBS, CELLS, N_ENV = 5, 16, 3
KW = dict(embedder=[12], middleware=[10], lstm_cells=CELLS, clip_gradients=None, beta_entropy=0.01, seed=3)


def _net(dev, continuous):
    from coach_amd.nn import networks as N
    np.random.seed(11)               # the V head's normalized-columns initialiser draws from the global stream
    return N.ContinuousActorCriticNet(dev, (OBS,), 2, **KW) if continuous else N.ActorCriticNet(dev, (OBS,), 3, **KW)


def _trunk(w, x, c, h):
    """rows of x as consecutive steps of the sequences in (c, h) [S, cells] -> (h_t of every row [steps, S, cells], c, h)"""
    import torch
    for name in ("main/embedder/dense0", "main/middleware/dense0"):
        if name + "/kernel" in w:
            x = torch.relu(x @ w[name + "/kernel"] + w[name + "/bias"])
    out = []
    for t in range(x.shape[0]):
        i, j, f, o = (torch.cat([x[t], h], 1) @ w["main/middleware/lstm/kernel"] + w["main/middleware/lstm/bias"]).split(CELLS, 1)
        c = c * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
        h = torch.tanh(c) * torch.sigmoid(o)
        out.append(h)
    return torch.stack(out), c, h


def _weights(net):
    import torch
    return {k: torch.tensor(v[0], dtype=torch.float64).requires_grad_() for k, v in net.params.named_arrays().items()}


@pytest.mark.parametrize("continuous", [False, True])
def test_acting_steps_advance_the_per_env_state(dev, continuous):
    import torch
    net, rng = _net(dev, continuous), np.random.RandomState(1)
    obs = rng.randn(7, N_ENV, OBS).astype(np.float32)
    w = _weights(net)
    c = h = torch.zeros(N_ENV, CELLS, dtype=torch.float64)
    for k in range(7):
        if k == 4:                                       # env 1's episode ended
            net.reset_state([1])
            c, h = c.clone(), h.clone()
            c[1] = h[1] = 0.0
        before = (c, h)
        (net.predict if k % 2 else net.policy_values)(torch.from_numpy(obs[k]).to(dev), N_ENV)
        _, c, h = _trunk(w, torch.tensor(obs[k:k + 1], dtype=torch.float64), c, h)
    state, previous = net.acting_state(N_ENV)
    for got, ref in zip(state + previous, (c, h) + before):
        np.testing.assert_allclose(got.cpu().numpy(), ref.detach().numpy(), **OUT)


@pytest.mark.parametrize("continuous", [False, True])
def test_window_gradients_from_a_carried_state(dev, continuous):
    import torch
    net, rng, T = _net(dev, continuous), np.random.RandomState(2), 5
    obs = rng.randn(T + 1, OBS).astype(np.float32)
    state = tuple(rng.uniform(-1, 1, size=(1, CELLS)).astype(np.float32) for _ in range(2))
    rewards = rng.uniform(-1, 2, size=T).astype(np.float32)
    actions = rng.randn(T, 2).astype(np.float32) if continuous else rng.randint(0, 3, size=T).astype(np.int32)
    dv = lambda a: torch.from_numpy(np.asarray(a)).to(dev)
    tgt, adv = (torch.zeros(T, dtype=torch.float64, device=dev) for _ in range(2))
    net.window_gradients(dv(obs), T, True, dv(actions), tgt, adv, dv(rewards), dv(np.array([0], np.uint8)), 0.99, 0.96,
                         R.GAE, False, initial_state=tuple(dv(s) for s in state))
    net.check_status()
    w = _weights(net)
    feat = _trunk(w, torch.tensor(obs[:, None], dtype=torch.float64), *(torch.tensor(s, dtype=torch.float64) for s in state))[0][:, 0]
    outs = [feat @ w[l.kname] + w[l.bname] for l in net.heads]
    np.testing.assert_allclose(net.values.cpu().numpy(), outs[0][:, 0].detach().numpy(), **OUT)
    v, z, *zs = (o.detach().numpy().astype(np.float32) for o in outs)
    if continuous:
        r = window_ref(v[:, 0], rewards, False, R.GAE, 0.01, T, m=z, s=zs[0], std=None, scale=None, a=actions)
        douts = [r["dV"][:, None], r["dmean"], r["dstd"]]
    else:
        r = R.window_loss(v[:, 0], z, actions, rewards, False, 0.99, 0.96, R.GAE, False, 0.01)
        douts = [r["dV"][:, None], r["dlogits"]]
    np.testing.assert_allclose(net.scalars.cpu().numpy(), [r[n] for n in ("loss", "value_loss", "policy_loss", "entropy")], **LOSS)
    assert not douts[0][-1].any()                        # the bootstrap row has no head gradient
    sum((o * torch.tensor(np.asarray(d), dtype=torch.float64)).sum() for o, d in zip(outs, douts)).backward()
    got = {k: v[0] for k, v in net.params.named_arrays(net.params.grads).items()}
    for name, t in w.items():
        np.testing.assert_allclose(got[name], t.grad.numpy(), err_msg=name, **OUT)
    np.testing.assert_allclose(float(net.norm.item()), np.sqrt(sum(float((t.grad ** 2).sum()) for t in w.values())), **LOSS)


def test_a_network_without_lstm_cells_is_built_as_before(dev):
    from coach_amd.nn.networks import ActorCriticNet
    assert [(n, e[1]) for n, e in ActorCriticNet(dev, (4,), 2).params.entries.items()] == [
        ("main/embedder/dense0/kernel", (4, 256)), ("main/embedder/dense0/bias", (256,)),
        ("main/middleware/dense0/kernel", (256, 512)), ("main/middleware/dense0/bias", (512,)),
        ("main/v_values_head/output/kernel", (512, 1)), ("main/v_values_head/output/bias", (1,)),
        ("main/policy_values_head/fc/kernel", (512, 2)), ("main/policy_values_head/fc/bias", (2,))]
    with pytest.raises(NotImplementedError, match="lstm_cells"):
        ActorCriticNet(dev, (84, 84, 4), 2, lstm_cells=16)


def test_agent_keeps_the_window_and_acting_states_of_every_env(dev):
    """lr 0: both states are recomputed from zeros over the running episode's stored observations"""
    import torch
    from coach_amd.agents.actor_critic_agent import ActorCriticAgent
    from coach_amd.architectures.middleware_parameters import LSTMMiddlewareParameters
    from test_a3c import _agent
    agent = _agent(dev, N_ENV, 5, R.GAE)
    wrapper = agent.ap.network_wrappers["main"]
    wrapper.learning_rate = 0.0
    wrapper.middleware_parameters = LSTMMiddlewareParameters(scheme="Empty", number_of_lstm_cells=CELLS)
    agent = ActorCriticAgent(agent.ap, agent.env, dev)
    agent.phase = agent.env.phase = agent.phase.TRAIN
    ended = set()
    for _ in range(60):
        agent.act()
        ended.add(tuple(np.nonzero(agent._episode_steps == 0)[0]))
        agent.train()
    agent.check_status()
    assert len(ended) > 2 and agent.training_iteration > 10          # episodes ended on different steps
    net, w, L = agent.networks["main"], _weights(agent.networks["main"]), agent.L
    zeros = torch.zeros(1, CELLS, dtype=torch.float64)
    for e in range(N_ENV):
        rows = agent.memory.obs[e * L:e * L + int(agent._episode_steps[e])].double().cpu()[:, None]
        for got, n in ((agent.window_state, int(agent.last_gradient_update_step_idx[e])), (net.acting_state(N_ENV)[0], len(rows))):
            ref = _trunk(w, rows[:n], zeros, zeros)[1:] if n else (zeros, zeros)
            for g, r in zip(got, ref):
                np.testing.assert_allclose(g[e:e + 1].cpu().numpy(), r.detach().numpy(), **OUT)


def test_mujoco_a3c_lstm_preset_builds_and_runs_100_steps(dev, tmp_path):
    import torch
    from coach_amd.core_types import EnvironmentSteps, RunPhase
    from coach_amd.presets import Mujoco_A3C_LSTM
    gm = Mujoco_A3C_LSTM.make(num_envs=1, episode_length=50)
    gm.schedule.improve_steps, gm.schedule.steps_between_evaluation_periods = EnvironmentSteps(100), EnvironmentSteps(100)
    gm.device = dev
    gm.logger.__init__(str(tmp_path / "a3c_lstm.csv"))
    gm.improve()
    net = gm.agent.networks["main"]
    assert net.lstm.H == 128 and net.torso.layers[-1].N == 200 and torch.isfinite(net.params.weights).all()
    # windows of 20 steps over episodes of 50: [0, 20), [20, 40), [40, 50) per episode, two episodes
    assert gm.total_steps_counters[RunPhase.TRAIN] == 100 and gm.agent.training_iteration == 6
