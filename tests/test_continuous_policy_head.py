"""The continuous PolicyHead on the device (csrc/gaussian_policy_head.hpp under rlx_a3c_continuous_window_loss,
rlx_pg_continuous_head_loss and rlx_gaussian_policy_forward) against a plain fp64 numpy evaluation of the head's formulas;
the network, the Actor-Critic agent on a Box vector environment and the Mujoco_A3C preset.  Tolerances are
tests/tolerances.py's: LOSS for the scalars, OUT for every gradient, mean and std.  Inputs: m in [-3, 3] plus a
tanh-saturated row at +-12, s in [-2, 3] plus a row at 30 (softplus's linear branch), so sigma stays in [0.12, 30]; actions
within 2 sigma of the mean; |adv| <= 2.  At exactly these inputs the same formulas in fp32 numpy (fp64 transcendentals
rounded once, as the kernel takes them) agree with head_ref / window_ref within 0.009 of OUT on the gradients, 0.002 of
OUT on mean and std and 0.004 of LOSS on the scalars (worst of all cases of the first test)."""
import numpy as np
import pytest

import a3c_ref as R
import pg_ref
from tolerances import LOSS, OUT

pytestmark = pytest.mark.gpu

EPS, LOG2PI = float(np.finfo(np.float32).eps), float(np.log(2 * np.pi))
SCALARS = ("loss", "value_loss", "policy_loss", "entropy")


def head_ref(m, s, std, scale, a, adv, beta, T):
    """fp64.  m / s [rows, D] (the first T rows are the window's), std / scale [D] or None, a [T, D], adv [T]"""
    m, a, adv = np.asarray(m, np.float64), np.asarray(a, np.float64), np.asarray(adv, np.float64)[:, None]
    D, th = m.shape[1], np.tanh(m)
    mu, dmu = (scale * th, scale * (1 - th * th)) if scale is not None else (m, np.ones_like(m))
    if s is not None:
        s = np.asarray(s, np.float64)
        sigma = np.maximum(s, 0) + np.log1p(np.exp(-np.abs(s))) + EPS
    else:
        sigma = np.broadcast_to(np.asarray(std, np.float64), m.shape)
    u = (a - mu[:T]) / sigma[:T]
    ls = np.log(sigma[:T]).sum(1)
    logpi = -0.5 * (u * u).sum(1) - ls - 0.5 * D * LOG2PI
    rest = ((0, len(m) - T), (0, 0))                                 # (zero gradients behind row T)
    dm = np.pad(-(adv / T) * u / sigma[:T] * dmu[:T], rest)
    ds = None if s is None else np.pad(
        (-(adv / T) * (u * u - 1) / sigma[:T] - beta / T / sigma[:T]) / (1 + np.exp(-s[:T])), rest)
    return dict(mean=mu, std=sigma, dmean=dm, dstd=ds,
                policy_loss=-(logpi * adv[:, 0]).mean(), entropy=(0.5 * D * (1 + LOG2PI) + ls).mean())


def window_ref(V, rewards, game_over, rescaler, beta, T, **head):
    """the window's targets (tests/a3c_ref.py), the V head (weight 0.5) and head_ref on the fp32 advantages, in fp64"""
    w = R.window_targets(V[:T], V[-1], rewards, game_over, 0.99, 0.96, rescaler, False)
    r = head_ref(adv=w["advantages32"], beta=beta, T=T, **head)
    dv = V[:T].astype(np.float64) - w["targets32"]
    r.update(w, value_loss=0.5 * (dv * dv).mean(), dV=np.append(dv / T, np.zeros(len(V) - T)))
    return dict(r, loss=r["value_loss"] + r["policy_loss"] - beta * r["entropy"])


def _t(x, dev, pad=0):           # [rows, D] gets `pad` more NaN columns, which a launch must neither read nor write
    import torch
    if x is not None and pad:
        x = np.concatenate([x, np.full((len(x), pad), np.nan, np.float32)], 1)
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _launch(rlx, dev, m, s, std, scale, a, T, beta, pad=3, V=None, rewards=None, game_over=False, rescaler=R.GAE,
            v_weight=0.5, adv=None, ld=None):
    """rlx_a3c_continuous_window_loss with V (adv given: RLX_A3C_TARGETS_GIVEN), else rlx_pg_continuous_head_loss"""
    import torch
    rows, D = m.shape
    ld = D + pad if ld is None else ld           # (ld is given only to be refused: the buffers keep D + pad columns)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    dm, ds, dv = nan(rows, D + pad), nan(rows, D + pad) if s is not None else None, nan(rows, 1 + pad)
    head = (_t(m, dev, pad), ld, _t(s, dev, pad), ld, _t(std, dev), _t(scale, dev), _t(a, dev))
    if V is None:
        sc = nan(2)
        rlx.pg_continuous_head_loss(*head, _t(np.asarray(adv, np.float32), dev), float(beta), rows, T, D, dm, ld, ds, ld,
                                    sc, 0)
        out = dict(zip(("loss", "entropy"), sc.cpu().numpy()))
    else:
        sc, status = nan(4), torch.zeros(1, dtype=torch.int32, device=dev)
        tgt, ad = (torch.full((T,), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
        if adv is not None:
            tgt, ad, rescaler = torch.zeros_like(tgt), _t(np.asarray(adv, np.float64), dev), -1
        rlx.a3c_continuous_window_loss(_t(V[:, None], dev, pad), 1 + pad, *head, _t(rewards, dev),
                                       _t(np.array([int(game_over)], np.uint8), dev), T, rows, D, 0.99, 0.96, int(rescaler),
                                       0, float(beta), float(v_weight), tgt, ad, dv, 1 + pad, dm, ld, ds, ld, sc, status, 0)
        assert int(status.item()) == 0 and np.isnan(dv.cpu().numpy()[:, 1:]).all()
        out = dict(zip(SCALARS, sc.cpu().numpy()), targets=tgt.cpu().numpy(), advantages=ad.cpu().numpy(),
                   dV=dv.cpu().numpy()[:, 0])
    for name, g in (("dmean", dm), ("dstd", ds)):
        out[name] = None if g is None else g.cpu().numpy()[:, :D]
        assert g is None or np.isnan(g.cpu().numpy()[:, D:]).all()
    return out


def _inputs(rng, T, D):          # the module text's ranges on T + 1 rows; place(mean, std) -> actions [T, D]
    m = rng.uniform(-3, 3, (T + 1, D)).astype(np.float32)
    s = rng.uniform(-2, 3, (T + 1, D)).astype(np.float32)
    m[0], s[T // 2] = 12.0 * np.where(np.arange(D) % 2, -1, 1), 30.0
    return m, s, lambda mu, sg: (mu[:T] + sg[:T] * rng.uniform(-2, 2, (T, D))).astype(np.float32)


_same_bytes = lambda x, y, names, rows=None: all(
    np.asarray(x[n]).tobytes() == np.atleast_1d(y[n])[:rows].tobytes() for n in names)


@pytest.mark.parametrize("D", [1, 2, 17, 32])
@pytest.mark.parametrize("T", [1, 64, 65, 257, 1025])
def test_kernels_equal_the_fp64_reference(rlx, dev, T, D):
    """T: one row, the wave's edge, an LDS chunk plus a row, four chunks plus a row; both std modes, bounded or not, beta
    0 / 0.01, terminal with and without the bootstrap row (the same bits); NaN padding survives; a repeat is identical"""
    import torch
    rng = np.random.RandomState(T * 100 + D)
    m, s, place = _inputs(rng, T, D)
    V, rewards = (rng.randn(T + 1) * 0.3).astype(np.float32), (rng.uniform(-1, 2, T) / 200).astype(np.float32)
    scale, std = rng.uniform(0.5, 2, D).astype(np.float32), rng.uniform(0.2, 2, D).astype(np.float32)
    for learned, bounded in [(l, b) for l in (True, False) for b in (True, False)]:
        head = dict(m=m, s=s if learned else None, std=None if learned else std, scale=scale if bounded else None)
        grads = ("dV", "dmean") + (("dstd",) if learned else ())
        fwd = head_ref(a=np.zeros((T, D)), adv=np.zeros(T), beta=0, T=T, **head)
        mean, sd = (torch.full((T + 1, D), float("nan"), device=dev) for _ in range(2))
        rlx.gaussian_policy_forward(_t(m, dev, 2), D + 2, _t(head["s"], dev, 2), D + 2, _t(head["std"], dev),
                                    _t(head["scale"], dev), T + 1, D, mean, sd, 0)
        np.testing.assert_allclose(mean.cpu().numpy(), fwd["mean"], **OUT)
        np.testing.assert_allclose(sd.cpu().numpy(), fwd["std"], **OUT)
        head["a"] = place(fwd["mean"], fwd["std"])
        for game_over, beta in [(g, b) for g in (False, True) for b in (0.0, 0.01)]:
            k = _launch(rlx, dev, T=T, beta=beta, V=V, rewards=rewards, game_over=game_over, **head)
            r = window_ref(V, rewards, game_over, R.GAE, beta, T, **head)
            assert np.array_equal(k["targets"], r["targets"]) and np.array_equal(k["advantages"], r["advantages"])
            for name in SCALARS + grads:
                np.testing.assert_allclose(k[name], r[name], err_msg=name, **(LOSS if name in SCALARS else OUT))
            assert not any(k[name][T:].any() for name in grads) and k["dV"][:T].any()
            if game_over:
                bare = _launch(rlx, dev, T=T, beta=beta, V=V[:T], rewards=rewards, game_over=True,
                               **dict(head, m=m[:T], s=s[:T] if learned else None))
                assert _same_bytes(bare, k, SCALARS + ("targets", "advantages") + grads, T)
        again = _launch(rlx, dev, T=T, beta=beta, V=V, rewards=rewards, game_over=True, **head)
        assert _same_bytes(again, k, SCALARS + ("targets", "advantages") + grads)


@pytest.mark.parametrize("T", [5, 257])
@pytest.mark.parametrize("rescaler", [R.A_VALUE, R.GAE])
def test_targets_are_the_discrete_launchs_bit_for_bit(rlx, dev, T, rescaler):
    """one recurrence (csrc/a3c_targets.hpp): the same V, rewards and flag through rlx_a3c_window_loss"""
    from test_a3c import _launch as discrete
    rng = np.random.RandomState(T)
    m, s, place = _inputs(rng, T, 3)
    V, rewards = rng.randn(T + 1).astype(np.float32), rng.uniform(-1, 2, T).astype(np.float32)
    for game_over in (False, True):
        k = _launch(rlx, dev, m, s, None, None, place(m, np.ones_like(s)), T, 0.01, V=V, rewards=rewards,
                    game_over=game_over, rescaler=rescaler)
        d = discrete(rlx, dev, V, m, np.zeros(T, np.int64), rewards, game_over, 0.99, 0.96, rescaler, False, 0.01)
        assert _same_bytes(k, d, ("targets", "advantages", "dV", "value_loss"))


@pytest.mark.parametrize("T,D,learned", [(1, 1, True), (65, 17, True), (257, 32, False), (300, 2, True)])
def test_policy_half_is_byte_identical_to_the_pg_launch(rlx, dev, T, D, learned):
    """one row arithmetic: v_loss_weight 0 and given advantages against the PG launch on their fp32 values"""
    rng = np.random.RandomState(T + D)
    m, s, place = _inputs(rng, T, D)
    scale, adv = rng.uniform(0.5, 2, D).astype(np.float32), rng.uniform(-2, 2, T)
    head = dict(m=m, s=s if learned else None, std=None if learned else np.ones(D, np.float32), scale=scale)
    head["a"] = place(m, np.ones_like(s))
    k = _launch(rlx, dev, T=T, beta=0.01, V=np.zeros(T + 1, np.float32), v_weight=0.0, adv=adv, **head)
    p = _launch(rlx, dev, T=T, beta=0.01, adv=adv.astype(np.float32), **head)
    assert _same_bytes(k, p, ("dmean", "entropy") + (("dstd",) * learned)) and p["loss"] == k["loss"]


@pytest.mark.parametrize("T,D", [(9, 2), (1, 1)])
def test_one_window_update_equals_the_composed_oracle(dev, T, D):
    """ContinuousActorCriticNet: one window and one Adam step against the oracle's layers + TF1 Adam composed with
    window_ref, as test_a3c.py::test_one_window_update_equals_the_composed_oracle_at_the_head_forks_branch_boundaries"""
    import torch
    from coach_amd.nn.networks import ContinuousActorCriticNet
    from oracle import nn as N
    from oracle.agents import DQNOracle
    rng, lr, beta, scale = np.random.RandomState(11), 5e-4, 0.01, np.full(D, 2.0, np.float32)
    net = ContinuousActorCriticNet(dev, (4,), D, scale, learning_rate=lr, optimizer_epsilon=1e-4, beta_entropy=beta, seed=3)
    arrays = {k.replace("policy_values_head/fc_mean", "q_head/dense"): v for k, v in net.params.named_arrays().items()}
    o, side = DQNOracle(arrays, (4,), D, lr=lr, eps=1e-4), {}
    for key, name in (("vh", "main/v_values_head/output"), ("sh", "main/policy_values_head/fc_std")):
        side[key] = N.Dense(arrays[name + "/kernel"][0].copy(), arrays[name + "/bias"][0].copy())
        o.chains.append((key, 0, N.Chain([side[key]])))
        o.names[(key, 0)] = [name]
    obs, rewards = rng.randn(T + 1, 4).astype(np.float32), rng.uniform(-1, 2, T).astype(np.float32)
    feat = o.tower.forward(N.prep_obs(obs, False))
    m, s, v = (l.forward(feat).astype(np.float32) for l in (o.head, side["sh"], side["vh"]))
    fwd = head_ref(m, s, None, scale, np.zeros((T, D)), np.zeros(T), 0, T)
    a = (fwd["mean"][:T] + 1.5 * fwd["std"][:T] * rng.choice([-1, 1], (T, D))).astype(np.float32)
    tgt, adv = (torch.zeros(T, dtype=torch.float64, device=dev) for _ in range(2))
    loss = net.accumulate_window(_t(obs, dev), T, True, _t(a, dev), tgt, adv, _t(rewards, dev),
                                 _t(np.array([0], np.uint8), dev), 0.99, 0.96, R.A_VALUE, False)
    r = window_ref(v[:, 0], rewards, False, R.A_VALUE, beta, T, m=m, s=s, std=None, scale=scale, a=a)
    o.tower.backward(sum(l.backward(r[g].astype(np.float32).reshape(T + 1, -1))
                         for l, g in ((o.head, "dmean"), (side["sh"], "dstd"), (side["vh"], "dV"))))
    for got, name in zip((loss,) + tuple(getattr(net, n) for n in SCALARS[1:]), SCALARS):
        np.testing.assert_allclose(float(got.item()), r[name], err_msg=name, **LOSS)
    np.testing.assert_allclose(float(net.norm.item()), o.global_norm(), **LOSS)
    net.apply_accumulated()
    net.check_status()
    assert torch.isfinite(net.params.weights).all() and not net.accumulated.any()


@pytest.mark.parametrize("lengths", [[7], [7, 11, 4]])
def test_agent_on_a_box_environment(dev, lengths):
    """Actor-Critic under ContinuousEntropyParameters: every env's windows are pg_ref.run's for its episode lengths, every
    stored action is fp32(mean + std * z) on the host stream's normals, replayed; default parameters refuse the Box"""
    import torch
    from coach_amd.agents.actor_critic_agent import ActorCriticAgent, ActorCriticAgentParameters
    from coach_amd.core_types import RunPhase
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    from coach_amd.exploration_policies.continuous_entropy import ContinuousEntropyParameters
    p = ActorCriticAgentParameters()
    p.seed, p.algorithm.num_steps_between_gradient_updates, p.algorithm.beta_entropy = 3, 5, 0.01
    env = SyntheticVectorEnvironment(SyntheticVectorEnvironmentParameters(
        "vector", len(lengths), (6,), None, action_dim=2, episode_length=max(lengths), episode_lengths=lengths,
        action_low=-2.0, action_high=2.0), dev)
    with pytest.raises(ValueError, match="continuous PolicyHead"):
        ActorCriticAgent(p, env, dev)
    p.exploration = ContinuousEntropyParameters()
    agent = ActorCriticAgent(p, env, dev)
    agent.phase, agent.debug_windows = RunPhase.TRAIN, []
    replay = np.random.RandomState()
    replay.set_state(np.random.get_state())
    n, L, w0 = len(lengths), max(lengths), agent.networks["main"].params.weights.clone()
    for step in range(60):
        pos = agent.memory.steps.copy()
        agent.act()
        expect = (agent._policy_mean.double().cpu().numpy() +
                  agent._policy_std.double().cpu().numpy() * replay.standard_normal((n, 2))).astype(np.float32)
        stored = agent.memory.action.view(n, L, 2).cpu().numpy()[np.arange(n), pos]
        assert np.array_equal(agent.actions.cpu().numpy(), expect) and np.array_equal(stored, expect)
        agent.train()
    agent.check_status()
    for e, length in enumerate(lengths):
        ws = pg_ref.run([np.zeros(length, np.float32)] * (60 // length + 1), 0.99, pg_ref.FUTURE_RETURN, L, 5, 5)
        mine = [(s, t) for env, s, t, *_ in agent.debug_windows if env == e]
        assert len(mine) >= 60 // length and mine == [(w["start"], w["end"]) for w in ws][:len(mine)]
    assert agent.current_episode == sum(60 // length for length in lengths)
    weights = agent.networks["main"].params.weights
    assert torch.isfinite(weights).all() and not torch.equal(weights, w0)


def test_bad_arguments_are_refused(rlx, dev):
    from coach_amd._rlx import RlxError
    m, s, place = _inputs(np.random.RandomState(0), 5, 3)
    ok = dict(m=m, s=s, std=None, scale=None, a=place(m, np.ones_like(s)), T=5, beta=0.0, adv=np.ones(5))
    for bad in (dict(m=np.zeros((6, 0), np.float32)), dict(m=np.zeros((6, 33), np.float32)), dict(ld=2), dict(a=None),
                dict(s=None), dict(T=0), dict(T=7)):
        for extra in ({}, dict(V=np.zeros(6, np.float32), rewards=np.zeros(5, np.float32), adv=None)):
            with pytest.raises(RlxError):
                _launch(rlx, dev, **dict(ok, **bad, **extra))


def test_mujoco_a3c_preset_builds_and_runs_100_steps(dev, tmp_path):
    import torch
    from coach_amd.core_types import EnvironmentSteps, RunPhase
    from coach_amd.presets import Mujoco_A3C
    gm = Mujoco_A3C.make(episode_length=20)
    gm.schedule.improve_steps, gm.schedule.steps_between_evaluation_periods = EnvironmentSteps(100), EnvironmentSteps(100)
    gm.device = dev
    gm.logger.__init__(str(tmp_path / "a3c.csv"))
    rows = gm.improve()
    net = gm.agent.networks["main"]
    assert type(net).__name__ == "ContinuousActorCriticNet" and torch.isfinite(net.params.weights).all()
    assert gm.total_steps_counters[RunPhase.TRAIN] == 100 and gm.agent.training_iteration == 5
    for name in ("Advantages", "Values", "Value Loss", "Policy Loss"):
        values = [r[name + "/Mean"] for r in rows if r.get(name + "/Mean", "") != ""]
        assert values and np.isfinite(np.asarray(values, dtype=np.float64)).all(), name
