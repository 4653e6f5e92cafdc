"""NAF on the device: rlx_naf_head_loss / rlx_naf_head_forward (csrc/naf.hip) against the numpy restatement
(tests/naf_ref.py, itself pinned by tests/test_naf_ref.py), the network update against the restatement composed with the
oracle's layers and TF1 Adam (tests/naf_compose.py), graph replay, the agent's cadence and signals, and a fixed-batch
learning check.

The kernel shares the restatement's operation order, so they differ by the device's expf and nothing else (the batch
sum's tree is the restatement's): Q, loss and gradients are bounded by FOUR times the fp32-against-fp64 error measured
on the CPU (test_naf_ref.MEASURED, in the conditioning-aware relative measure of test_naf_ref.errors), the TD targets
bit for bit."""
import random

import numpy as np
import pytest

import naf_ref as R
from naf_compose import FIXED, ComposedNAF, fixed_batch_problem
from test_naf_ref import ACTION_DIMS, MEASURED, as_got, errors, make_case, ref_update
from tolerances import LOSS, WEIGHTS

pytestmark = pytest.mark.gpu
HEADROOM = 4.0          # for the device expf's ulps (the issue's factor)


def _t(x, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t if dtype is None else t.to(dtype)


def _padded(x, pad, dev):
    """[B, n] -> a device buffer [B, n + pad] (NaN in the padding) holding x: a leading dimension larger than the row"""
    x = np.asarray(x, np.float32).reshape(len(x), -1)
    buf = np.full((x.shape[0], x.shape[1] + pad), np.nan, np.float32)
    buf[:, :x.shape[1]] = x
    return _t(buf, dev)


def _launch(rlx, dev, c, huber, pad=3, discount=0.99):
    import torch
    B, A = c["actions"].shape
    NL = R.packed_size(A)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    dv, dmu, dl = nan(B, 1 + pad), nan(B, A + pad), nan(B, NL + pad)
    ws, ticket, loss = torch.zeros(B, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), nan(1)
    td, q, adv = nan(B), nan(B), nan(B)
    rlx.naf_head_loss(_padded(c["v"], pad, dev), 1 + pad, _padded(c["mu_unscaled"], pad, dev), A + pad,
                      _padded(c["l_vector"], pad, dev), NL + pad, _t(c["output_scale"], dev),
                      _padded(c["actions"], pad, dev), A + pad, _padded(c["v_next"], pad, dev), 1 + pad,
                      _t(c["rewards"], dev), _t(c["game_overs"].astype(np.uint8), dev), discount, B, A, int(huber), 1.0,
                      dv, 1 + pad, dmu, A + pad, dl, NL + pad, ws, ticket, loss, td, q, adv, 0)
    torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy()
    assert np.isnan(h(dv)[:, 1:]).all() and np.isnan(h(dmu)[:, A:]).all() and np.isnan(h(dl)[:, NL:]).all()
    return dict(dv=h(dv)[:, 0], dmu=h(dmu)[:, :A], dl=h(dl)[:, :NL], loss=h(loss)[0], td=h(td), q=h(q), adv=h(adv),
                ticket=int(ticket.item()))


def _within(err, rel, what):
    print("    %-5s error %.3e  bound %.3e" % (what, err, HEADROOM * rel))
    assert err <= HEADROOM * rel, (what, err, HEADROOM * rel)


@pytest.mark.parametrize("huber", [False, True])
@pytest.mark.parametrize("A", ACTION_DIMS)
@pytest.mark.parametrize("B", [1, 32, 37, 256])
def test_loss_kernel_equals_the_restatement(rlx, dev, B, A, huber):
    c = make_case(B, A, seed=1000 * B + A)
    assert c["game_overs"].any() or B == 1
    d, u = _launch(rlx, dev, c, huber), ref_update(c, huber)
    print("\n  B=%d A=%d %s" % (B, A, "huber" if huber else "mse"))
    assert d["ticket"] == 0
    assert d["td"].tobytes() == u["td_targets"].tobytes()
    err = errors(c, huber, dict(q=d["q"], loss=d["loss"], dv=d["dv"], dmu=d["dmu"], dl=d["dl"]), as_got(u))
    for k in ("q", "loss", "dv", "dmu", "dl"):
        _within(err[k], MEASURED[A][k], k)
    same = c["same"]
    assert np.all(d["adv"][same] == 0) and np.array_equal(d["q"][same], c["v"][same])
    assert np.all(d["dmu"][same] == 0) and np.all(d["dl"][same] == 0)
    again = _launch(rlx, dev, c, huber)
    for k in ("dv", "dmu", "dl", "loss", "q"):
        assert again[k].tobytes() == d[k].tobytes(), k


def test_unsupported_shapes_and_null_pointers_are_refused(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    z = torch.zeros(300 * 600, dtype=torch.float32, device=dev)
    i = torch.zeros(512, dtype=torch.int32, device=dev)
    loss = torch.full((1,), 7.0, dtype=torch.float32, device=dev)

    def call(B, A, v=z, actions=z, dl=z, ticket=i):
        NL = A * (A + 1) // 2
        rlx.naf_head_loss(v, 1, z, A, z, NL, z, actions, A, z, 1, z, i, 0.99, B, A, 0, 1.0, z, 1, z, A, dl, NL, z,
                          ticket, loss, None, None, None, 0)
    for kw in (dict(B=1, A=33), dict(B=257, A=2), dict(B=0, A=2), dict(B=4, A=0), dict(B=4, A=2, v=None),
               dict(B=4, A=2, actions=None), dict(B=4, A=2, dl=None), dict(B=4, A=2, ticket=None)):
        with pytest.raises(RlxError):
            call(**kw)
    with pytest.raises(RlxError):
        rlx.naf_head_forward(z, 1, z, 33, z, 561, z, None, 33, 4, 33, z, z, z, z, 0)
    with pytest.raises(RlxError):
        rlx.naf_head_forward(z, 1, z, 2, z, 3, z, None, 2, 4, 2, None, None, None, None, 0)
    torch.cuda.synchronize()
    assert float(loss.item()) == 7.0 and int(i.sum().item()) == 0 and float(z.abs().sum().item()) == 0.0   # nothing ran


@pytest.mark.parametrize("B,A", [(1, 1), (5, 2), (37, 17), (300, 32)])
def test_forward_entry_point(rlx, dev, B, A):
    import torch
    c = make_case(B, A, seed=B + A)
    NL = R.packed_size(A)
    args = (_t(c["v"], dev), 1, _t(c["mu_unscaled"], dev), A, _t(c["l_vector"], dev), NL, _t(c["output_scale"], dev))
    outs = lambda: (torch.full((B, A), float("nan"), device=dev), torch.full((B,), float("nan"), device=dev),
                    torch.full((B,), float("nan"), device=dev), torch.full((B, A, A), float("nan"), device=dev))
    mu, q, adv, L = outs()
    rlx.naf_head_forward(*args, None, A, B, A, mu, q, adv, L, 0)
    f = R.forward(c["v"], c["mu_unscaled"], c["l_vector"], c["output_scale"], None)
    assert np.array_equal(q.cpu().numpy(), c["v"]) and np.all(adv.cpu().numpy() == 0)
    assert np.array_equal(mu.cpu().numpy(), f["mu"])
    Ld = L.cpu().numpy()
    assert np.all(Ld[:, np.triu_indices(A, 1)[0], np.triu_indices(A, 1)[1]] == 0)
    low = np.tril_indices(A, -1)
    assert np.array_equal(Ld[:, low[0], low[1]], f["L"][:, low[0], low[1]])
    diag = np.arange(A)
    np.testing.assert_allclose(Ld[:, diag, diag], f["L"][:, diag, diag], rtol=4 * 1.2e-7, atol=0)   # expf: ulps
    assert np.all(Ld[:, diag, diag] > 0)
    # with actions: the loss kernel's Q and Advantage
    mu, q, adv, L = outs()
    rlx.naf_head_forward(*args, _t(c["actions"], dev), A, B, A, mu, q, adv, None, 0)
    g = R.forward(c["v"], c["mu_unscaled"], c["l_vector"], c["output_scale"], c["actions"])
    s_q = np.abs(c["v"].astype(np.float64)) + np.abs(g["adv"].astype(np.float64))      # errors()'s scale of Q
    for name, got, want in (("Q", q, g["q"]), ("Adv", adv, g["adv"])):
        delta = np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64))
        assert np.all(delta[s_q == 0] == 0)
        _within(float(np.max(delta[s_q > 0] / s_q[s_q > 0])), MEASURED[A]["q"], name)


def _net(dev, clip=None, clip_by_value=False, **kw):
    from coach_amd.nn.networks import NAFNet
    scale = np.linspace(1.0, 2.0, 6).astype(np.float32)
    net = NAFNet(dev, (17,), 6, scale, embedder=[200], middleware=[200], seed=3, clip_gradients=clip,
                 clip_by_value=clip_by_value, **kw)
    return net, scale


def _batches(n, B=32, obs=17, A=6, seed=5):
    rng = np.random.RandomState(seed)
    for _ in range(n):
        yield (rng.randn(B, obs).astype(np.float32), rng.randn(B, obs).astype(np.float32),
               rng.uniform(-2, 2, size=(B, A)).astype(np.float32), rng.randn(B).astype(np.float32), rng.rand(B) < 0.2)


@pytest.mark.parametrize("updates,clip", [(1, None), (5, None), (5, 0.02)])
def test_network_update_equals_the_composed_restatement(dev, updates, clip):
    import torch
    net, scale = _net(dev, clip, clip_by_value=clip is not None)
    arrays = net.params.named_arrays()
    assert set(n for n in arrays if "head" in n) == {
        "main/naf_q_values_head/%s/%s" % (l, p) for l in ("V", "mu_unscaled", "l_vector") for p in ("kernel", "bias")}
    o = ComposedNAF(arrays, scale, clip_value=clip)
    clipped_something = False
    for obs, nxt, act, rew, go in _batches(updates):
        loss = net.learn_from_batch(_t(obs, dev), _t(nxt, dev), 32, _t(act, dev), _t(rew, dev),
                                    _t(go.astype(np.uint8), dev), 0.99)
        ref = o.learn(obs, nxt, act, rew, go, 0.99)
        np.testing.assert_allclose(float(loss.item()), ref, **LOSS)
        if clip is not None:
            raw = max(float(np.abs(l.dW).max()) for _, l in o.named_layers())
            clipped_something |= raw >= np.float32(clip)                   # (dW was clamped in place: at the threshold)
            assert float(net.params.grads.abs().max().item()) <= clip
        net.update_target(0.001)
        o.update_target(0.001)
    assert clip is None or clipped_something
    wd, wo = net.params.named_arrays(), o.weights()
    print("\n  %d updates, clip %s: weights max abs diff %.3e" % (
        updates, clip, max(float(np.abs(wd[n][0] - w).max()) for n, w in wo.items())))
    for name, w in wo.items():
        np.testing.assert_allclose(wd[name][0], w, err_msg=name, **WEIGHTS)
    assert torch.isfinite(net.params.weights).all()
    net.check_status()


@pytest.mark.parametrize("A,B", [(5, 68),       # l_vector is 15 wide, B * 15 = 1020: the three layers in one launch both ways
                                 (5, 69),       # B * 15 = 1035: l_vector's backward pass is a launch of its own
                                 (6, 8)])       # l_vector is 21 wide: a launch of its own both ways
def test_one_update_equals_the_composed_restatement_at_the_head_forks_branch_boundaries(dev, A, B):
    """test_network_update_equals_the_composed_restatement with one unclipped update, at the shapes where the head
    layers' launches change form."""
    import torch
    from coach_amd.nn.networks import NAFNet
    scale = np.linspace(1.0, 2.0, A).astype(np.float32)
    net = NAFNet(dev, (17,), A, scale, embedder=[200], middleware=[200], seed=3)
    assert net.l_layer.N == A * (A + 1) // 2
    o = ComposedNAF(net.params.named_arrays(), scale)
    (obs, nxt, act, rew, go), = _batches(1, B=B, A=A)
    loss = net.learn_from_batch(_t(obs, dev), _t(nxt, dev), B, _t(act, dev), _t(rew, dev), _t(go.astype(np.uint8), dev),
                                0.99)
    ref = o.learn(obs, nxt, act, rew, go, 0.99)
    wd, wo = net.params.named_arrays(), o.weights()
    print("\n  A %d B %d: loss %.6f / %.6f, weights max abs diff %.3e" % (
        A, B, float(loss.item()), ref, max(float(np.abs(wd[n][0] - w).max()) for n, w in wo.items())))
    np.testing.assert_allclose(float(loss.item()), ref, **LOSS)
    for name, w in wo.items():
        np.testing.assert_allclose(wd[name][0], w, err_msg=name, **WEIGHTS)
    assert torch.isfinite(net.params.weights).all()
    net.check_status()


def _agent(dev, n_env=1, use_graphs=None, L=5, batch=16, seed=5):
    from coach_amd.agents.naf_agent import NAFAgent, NAFAgentParameters
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    from coach_amd.memories.memory import MemoryGranularity
    ap = NAFAgentParameters()
    ap.seed = seed
    net = ap.network_wrappers["main"]
    net.batch_size, net.embedder_scheme, net.middleware_scheme = batch, [32], [32]
    ap.memory.max_size = (MemoryGranularity.Transitions, 400)
    env = SyntheticVectorEnvironment(SyntheticVectorEnvironmentParameters(
        "vector", n_env, (6,), None, action_dim=3, episode_length=L, seed=3), dev)
    return NAFAgent(ap, env, dev, use_graphs=use_graphs)


def test_discrete_action_space_is_refused(dev):
    from coach_amd.agents.naf_agent import NAFAgent, NAFAgentParameters
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    env = SyntheticVectorEnvironment(SyntheticVectorEnvironmentParameters("vector", 1, (4,), 2, episode_length=5, seed=3),
                                     dev)
    with pytest.raises(ValueError, match="NAF works only for continuous control problems"):
        NAFAgent(NAFAgentParameters(), env, dev)


def test_graph_captured_update_equals_eager_bit_for_bit(dev):
    import torch
    from coach_amd.core_types import RunPhase
    agents = []
    for graphs in (True, False):
        a = _agent(dev, use_graphs=graphs)
        random.seed(9); np.random.seed(9)
        a.phase = RunPhase.HEATUP
        for _ in range(5):
            a.act()
        a.phase = RunPhase.TRAIN
        for _ in range(3):                    # 15 updates: the first eager, the second captured, 13 replays
            a.act(); a.train()
        a.check_status()
        agents.append(a)
    g, e = agents
    assert g.training_iteration == e.training_iteration == 15
    assert any(k[0] == "learn" for k in g._graphs) and not e._graphs
    ng, ne = g.networks["main"], e.networks["main"]
    assert torch.equal(ng.params.weights, ne.params.weights) and torch.equal(ng.target, ne.target)
    assert torch.equal(ng.adam.v, ne.adam.v) and torch.equal(ng.loss, ne.loss) and torch.equal(g.actions, e.actions)
    assert not torch.equal(ng.params.weights, ng.target)


def test_agent_cadence_target_mixing_sampling_and_signals(dev):
    from coach_amd.core_types import RunPhase
    L, n_env = 5, 4
    a = _agent(dev, n_env=n_env, use_graphs=False, L=L)
    stats = a.enable_signal_statistics()
    assert a.SIGNAL_NAMES[-6:] == ["Q", "L", "Advantage", "Action", "V", "TD targets"]
    net = a.networks["main"]
    mixes, apply = [], net.apply_gradients
    net.apply_gradients = lambda *args, **kw: (mixes.append(kw.get("mix_rate")), apply(*args, **kw))[1]
    a.debug_draws = []
    random.seed(2); np.random.seed(2)
    a.phase = RunPhase.TRAIN
    per_step, target0 = [], net.target.clone()
    for step in range(3 * L):
        a.act()
        before, seen = a.training_iteration, len(a.debug_draws)
        a.train()
        per_step.append(a.training_iteration - before)
        complete = a.memory.num_transitions_in_complete_episodes()
        assert complete == n_env * L * ((step + 1) // L)
        for d in a.debug_draws[seen:]:                      # only complete episodes are sampled
            assert len(d) == 16 and d.max() < complete and d.min() >= 0
    a.check_status()
    # nothing before an episode is complete, then five updates per env step (n_env env steps per vector step)
    assert per_step == [0] * (L - 1) + [5 * n_env] * (2 * L + 1)
    # the target: mixed at 0.001 after every vector step's first update (EnvironmentSteps(1)), in the Adam pass
    assert len(mixes) == sum(per_step)
    assert [m for m in mixes if m is not None] == [0.001] * (2 * L + 1)
    assert all(m == 0.001 for m in mixes[::5 * n_env]) and not np.array_equal(target0.cpu().numpy(), net.target.cpu().numpy())
    row = stats.flush()
    for name in ("Q", "L", "Advantage", "Action", "V", "TD targets", "Loss", "Grads (unclipped)"):
        assert row[name + "/Mean"] != "" and np.isfinite(row[name + "/Mean"]), name
    assert row["Advantage/Max"] == 0 and row["Advantage/Min"] == 0          # the head's values at u = mu
    assert row["Q/Mean"] == row["V/Mean"]


def test_fixed_batch_learning_check(dev):
    """Rewards -||u - W s||^2, every row terminal, one batch of 64 reused for 200 updates (naf_compose.FIXED): the
    device loss must end below 10 % of its initial value and at most twice the loss the CPU restatement reaches from the
    same initial weights (the restatement alone ends at 0.0035 %, tests/test_naf_ref.py)."""
    import torch
    from coach_amd.nn.networks import NAFNet
    f = FIXED
    obs, actions, rewards, arrays, scale = fixed_batch_problem()
    net = NAFNet(dev, (f["obs_dim"],), f["A"], scale, embedder=f["embedder"], middleware=f["middleware"],
                 learning_rate=f["lr"], seed=0)
    for name, towers in arrays.items():
        net.params.w(name, 0).copy_(torch.from_numpy(towers[0]))
    net.target.copy_(net.params.weights)
    o = ComposedNAF(arrays, scale, lr=f["lr"])
    go = np.ones(f["B"], bool)
    d_obs, d_act, d_rew, d_go = _t(obs, dev), _t(actions, dev), _t(rewards, dev), _t(go.astype(np.uint8), dev)
    dev_losses = torch.zeros(200, device=dev)
    cpu_losses = []
    for k in range(200):
        dev_losses[k] = net.learn_from_batch(d_obs, d_obs, f["B"], d_act, d_rew, d_go, 0.99)[0]
        cpu_losses.append(o.learn(obs, obs, actions, rewards, go, 0.99))
    dl = dev_losses.cpu().numpy()
    print("\n  device loss %.4g -> %.4g (%.4f %%), restatement %.4g -> %.4g" % (
        dl[0], dl[-1], 100 * dl[-1] / dl[0], cpu_losses[0], cpu_losses[-1]))
    np.testing.assert_allclose(dl[0], cpu_losses[0], **LOSS)
    assert dl[-1] < 0.10 * dl[0]
    assert dl[-1] <= 2.0 * cpu_losses[-1]
