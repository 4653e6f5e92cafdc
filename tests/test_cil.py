"""csrc/cil.hip (G.BranchStack, CILNet) against plain fp64 evaluations: numpy for the forward pass, the targets, the losses
and dy; CPU torch autograd for everything behind dy.  The dropout masks are rebuilt from the Philox twin in noise_ref.

Margins: the largest error of the SAME evaluation carried out in float32 on the CPU against the fp64 one, times 4 (MFMA
chains in k order and the device tanh differ from numpy's pairwise sums and libm by a few ulp of the same kind).  That
float32 error of the clean forward pass, measured for the three cases below: 1.2e-07, 4.7e-07, 2.0e-06 (F32_ERR).
A head loss is ONE number per branch (a single squared error in the smallest case), and the float32 error of one number
varies by 15x from one set of inputs to the next (3.8e-08 .. 5.7e-07 in the smallest case), so for the losses the float32
error is the largest over LOSS_SEEDS = 8 input sets of the same shape -- still 4x the reference's own float32 error."""
import numpy as np
import pytest

import noise_ref

pytestmark = pytest.mark.gpu

CASES = [(1, 16, 16, 16, 1, 2), (17, 48, 32, 16, 3, 4), (33, 512, 256, 256, 16, 8)]          # B, F, H1, H2, A, K
F32_ERR = dict(zip(CASES, (1.2e-07, 4.7e-07, 2.0e-06)))       # max |float32 - fp64| of y, measured on the CPU
SEED, STREAM0, BAD, LOSS_SEEDS = 11, 128, 1, 8


def inputs(case, seed=0):
    B, F, H1, H2, A, K = case
    rng = np.random.RandomState(sum(case) + 1000 * seed)
    f32 = lambda a: a.astype(np.float32)
    lim = lambda k, u: np.sqrt(6.0 / (k + u))
    w = [(f32(rng.uniform(-lim(k, u), lim(k, u), (K, k, u))), f32(0.1 * rng.randn(K, u)))
         for k, u in ((F, H1), (H1, H2), (H2, A))]
    return dict(w=w, x=f32(rng.randn(B, F)), commands=rng.randint(0, K, B).astype(np.int32), actions=f32(rng.randn(B, A)))


def chain(inp, dtype, masks=(1.0, 1.0)):
    """-> (y [K, B, A], h1, h2) in dtype; masks: the (mask * scale) factors behind the two hidden activations"""
    h, hs = inp["x"].astype(dtype)[None], []
    for l, (W, b) in enumerate(inp["w"]):
        h = h @ W.astype(dtype) + b.astype(dtype)[:, None, :]
        if l < 2:
            h = np.tanh(h) * np.asarray(masks[l]).astype(dtype)
            hs.append(h)
    return h, hs[0], hs[1]


def masks(case, rates, draw, seed=SEED):
    """float32 mask * scale [K, B, H] of both layers at a draw index: the counter layout of include/rlx.h"""
    B, _, H1, H2, _, K = case
    out = []
    for l, (H, rate) in enumerate(zip((H1, H2), rates)):
        k, b, c4 = np.ix_(np.arange(K), np.arange(B), np.arange(H // 4))
        words = noise_ref.philox4x32_10(b * 64 + c4 + 0 * k, STREAM0 + 2 * k + l + 0 * b + 0 * c4, draw & 0xFFFFFFFF,
                                        (draw >> 32) ^ noise_ref.NOISE_TAG, seed, 0)
        keep = np.stack(words, -1).reshape(K, B, H) >= np.uint64(float(np.float32(rate)) * 2.0 ** 32)
        out.append(keep * (np.float32(1) / (np.float32(1) - np.float32(rate))))
    return out


def head_loss(inp, y, y_train, huber, dtype):
    """the targets of CILAgent.learn_from_batch, the K head losses + total, dy"""
    K, B, _ = y.shape
    own = (inp["commands"][None, :] == np.arange(K)[:, None])[:, :, None]
    e = y_train - np.where(own, inp["actions"].astype(dtype)[None], y)
    if huber:
        terms, g = np.where(np.abs(e) <= 1, 0.5 * e * e, np.abs(e) - 0.5), np.clip(e, -1, 1)
    else:
        terms, g = e * e, 2 * e
    losses = terms.sum((1, 2), dtype=dtype) / dtype(B)
    return np.append(losses, losses.sum()), g / dtype(B)


def torch_grads(inp, m, dy, dtype, trunk=None):
    """autograd from dy at the training pass's output, masks injected -> {name: gradient}; trunk: [(W, b)] of relu layers"""
    import torch
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype, requires_grad=True)
    x = x0 = t(inp["x"])
    tw = [(t(W), t(b)) for W, b in trunk or ()]
    for W, b in tw:
        x = torch.relu(x @ W + b)
    w, zs = [(t(W), t(b)) for W, b in inp["w"]], []
    h = x[None]
    for l, (W, b) in enumerate(w):
        h = h @ W + b[:, None, :]
        if l < 2:
            h.retain_grad()
            zs.append(h)
            h = torch.tanh(h) * torch.tensor(np.asarray(m[l], dtype=np.float64), dtype=dtype)
    h.backward(torch.tensor(np.asarray(dy, dtype=np.float64), dtype=dtype))
    out = {"dx": x0.grad, "dz1": zs[0].grad, "dz2": zs[1].grad}
    for i, (W, b) in enumerate(w + tw):
        out["w%d" % i], out["b%d" % i] = W.grad, b.grad
    return {k: v.numpy() for k, v in out.items()}


def close(got, ref64, ref32, what):
    margin = 4 * np.abs(np.asarray(ref32, dtype=np.float64) - ref64).max()
    err = np.abs(np.asarray(got, dtype=np.float64) - ref64).max()
    print("%s: error %.3g, margin %.3g" % (what, err, margin))
    assert err <= margin, what


class Stack:
    """a G.BranchStack on the case's weights and input"""

    def __init__(self, dev, case, rates=(0.0, 0.0)):
        import torch
        from coach_amd.nn import graph as G
        B, F, H1, H2, A, K = case
        self.inp, self.torch, self.params = inputs(case), torch, G.FlatParams()
        self.layer = G.BranchStack(self.params, "head", F, (H1, H2), A, K, "tanh", rates, seed=SEED)
        self.params.finalize(dev)
        self.layer.initialize(np.random.RandomState(0))
        for n, (W, b) in zip(self.layer.names, self.inp["w"]):
            for k in range(K):
                self.params.w(n + "/kernel", k).copy_(torch.from_numpy(W[k]))
                self.params.w(n + "/bias", k).copy_(torch.from_numpy(b[k]))
        self.ctx = G.Context(dev)
        to = lambda a: torch.from_numpy(a).to(dev)
        self.x = G.Tensor(to(self.inp["x"]).view(1, B, F), B, F, 1, act=None)
        self.commands, self.actions = to(self.inp["commands"]), to(self.inp["actions"])
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)

    def train(self, huber=False):
        s = self.layer.train(self.ctx, self.x, self.commands, self.actions, self.status, huber=huber, want_y_train=True)
        self.torch.cuda.synchronize()
        return s, {k: v.cpu().numpy().copy() for k, v in s.items() if hasattr(v, "cpu")}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def drop(clean, m):
    """clean * mask * scale as the device forms it: one float32 product where kept, +0 where dropped"""
    return np.where(m != 0, clean * m.astype(np.float32), np.float32(0))


@pytest.mark.parametrize("case", CASES)
def test_clean_forward_and_selected_values(dev, case):
    s = Stack(dev, case)
    y64 = chain(s.inp, np.float64)[0]
    y, values = s.layer.forward(s.ctx, s.x, commands=s.commands, status=s.status)
    rows = np.arange(case[0])
    close(y.cpu().numpy(), y64, y64 + F32_ERR[case], "y")
    assert np.array_equal(values.cpu().numpy(), y.cpu().numpy()[s.inp["commands"], rows]) and s.status.item() == 0
    values.fill_(7.0)
    s.commands[0] = case[5]                                             # one past the last branch
    s.layer.forward(s.ctx, s.x, commands=s.commands, status=s.status)
    got = values.cpu().numpy()
    assert s.status.item() == BAD and (got[0] == 7.0).all() and np.array_equal(got[1:], y.cpu().numpy()[s.inp["commands"], rows][1:])


@pytest.mark.parametrize("case", CASES)
def test_rates_zero_is_the_clean_pass(dev, case):
    s = Stack(dev, case)
    y = s.layer.forward(s.ctx, s.x)[0].cpu().numpy()
    _, out = s.train()
    assert np.array_equal(bits(out["y"]), bits(y)) and np.array_equal(bits(out["y_train"]), bits(y))
    own = s.inp["commands"][None, :] == np.arange(case[5])[:, None]
    assert (out["dy"][~own] == 0).all() and (out["dy"][own] != 0).any()


@pytest.mark.parametrize("rates,name", [((0.5, 0.0), "h1"), ((0.0, 0.3), "h2"), ((0.5, 0.3), "h1")])
@pytest.mark.parametrize("case", CASES)
def test_dropout_masks_are_the_twins_and_fresh_every_launch(dev, case, rates, name):
    clean, s = Stack(dev, case).train()[1], Stack(dev, case, rates)
    first, second = s.train()[1], s.train()[1]                         # draw indices 0 and 1
    for draw, out in enumerate((first, second)):
        assert np.array_equal(bits(out[name]), bits(drop(clean[name], masks(case, rates, draw)[int(name[1]) - 1])))
    assert not np.array_equal(first[name], second[name])


def test_captured_update_draws_new_masks_every_replay(dev):
    """CILNet.learn_from_batch captured before any eager update ran: every replay uses the next draw index, and the
    zeros of the saved activations are the twin's masks of that index (the weights move, so only the pattern is pinned)"""
    import torch
    from coach_amd.nn.networks import CILNet
    case = B, F, H1, H2, A, K = (17, 48, 32, 16, 3, 4)
    net = CILNet(dev, (6,), A, K, hidden=(H1, H2), head_activation="tanh", dropout_rates=(0.5, 0.3), embedder=[32],
                 middleware=[F], seed=SEED)
    inp = inputs(case)
    obs, cmd, act = (torch.from_numpy(a).to(dev) for a in (inp["x"][:, :6].copy(), inp["commands"], inp["actions"]))
    net.predict(obs, B)                                                 # (loads the library's kernels; no update, no draw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.accumulate_gradients(obs, B, cmd, act)                      # allocates the pass's buffers; draw 0
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.learn_from_batch(obs, B, cmd, act)
    for draw in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert net.stack.draw_used.item() == draw
        for l, name in enumerate(("h1", "h2")):
            got = net.ctx.buffer("main/regression_head/" + name, masks(case, (0.5, 0.3), draw)[l].shape, tag="train")
            assert np.array_equal(got.cpu().numpy() != 0, masks(case, (0.5, 0.3), draw)[l] != 0)


@pytest.mark.parametrize("huber", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_losses_and_backward(dev, case, huber):
    s = Stack(dev, case, (0.5, 0.3))
    saved, out = s.train(huber)
    m, ref = masks(case, (0.5, 0.3), 0), {}
    for dtype in (np.float64, np.float32):
        y, (yt, h1, h2) = chain(s.inp, dtype)[0], chain(s.inp, dtype, m)
        losses, dy = head_loss(s.inp, y, yt, huber, dtype)
        ref[dtype] = dict(y=y, y_train=yt, h2=h2, losses=losses, dy=dy)
    for name in ("y", "y_train", "h2", "dy"):
        close(out[name], ref[np.float64][name], ref[np.float32][name], name)
    f32_err = 0.0
    for seed in range(LOSS_SEEDS):
        other = inputs(case, seed)
        l64, l32 = (head_loss(other, chain(other, dt)[0], chain(other, dt, m)[0], huber, dt)[0] for dt in (np.float64, np.float32))
        f32_err = max(f32_err, np.abs(l32.astype(np.float64) - l64).max())
    close(out["losses"], ref[np.float64]["losses"], ref[np.float64]["losses"] + f32_err, "losses")
    s.layer.backward(s.ctx, s.x, saved)
    s.torch.cuda.synchronize()
    import torch
    g64, g32 = (torch_grads(s.inp, m, out["dy"], dt) for dt in (torch.float64, torch.float32))
    got = {"dx": s.x.grad.view(case[0], case[1]), "dz1": s.ctx.buffer("head/dz1", g64["dz1"].shape, tag="train"),
           "dz2": s.ctx.buffer("head/dz2", g64["dz2"].shape, tag="train")}
    for i, n in enumerate(s.layer.names):
        got["w%d" % i] = torch.stack([s.params.g(n + "/kernel", k) for k in range(case[5])])
        got["b%d" % i] = torch.stack([s.params.g(n + "/bias", k) for k in range(case[5])])
    for name, v in got.items():
        close(v.cpu().numpy(), g64[name], g32[name], name)


def test_cilnet_full_gradient(dev):
    """CILNet (vector embedder + FC middleware + the stack): every parameter's gradient of one update's total loss"""
    import torch
    from coach_amd.nn.networks import CILNet
    case = B, F, H1, H2, A, K = (17, 48, 32, 16, 3, 4)
    net = CILNet(dev, (6,), A, K, hidden=(H1, H2), head_activation="tanh", dropout_rates=(0.5, 0.3), embedder=[32],
                 middleware=[F], seed=SEED)
    inp, arrays = inputs(case), net.params.named_arrays()
    inp["x"] = np.random.RandomState(3).randn(B, 6).astype(np.float32)
    trunk = [(arrays[n + "/kernel"][0], arrays[n + "/bias"][0]) for n in ("main/embedder/dense0", "main/middleware/dense0")]
    inp["w"] = [(np.stack(arrays[n + "/kernel"]), np.stack(arrays[n + "/bias"])) for n in net.stack.names]
    to = lambda a: torch.from_numpy(a).to(dev)
    saved = net.accumulate_gradients(to(inp["x"]), B, to(inp["commands"]), to(inp["actions"]), want_y_train=True)
    net.check_status()
    m = masks(case, (0.5, 0.3), 0)
    dy = saved["dy"].cpu().numpy()
    g64, g32 = (torch_grads(inp, m, dy, dt, trunk) for dt in (torch.float64, torch.float32))
    names = [n for n in net.stack.names] + ["main/embedder/dense0", "main/middleware/dense0"]
    for i, n in enumerate(names):
        T = K if i < 3 else 1
        for kind, part in (("w", "/kernel"), ("b", "/bias")):
            got = torch.stack([net.params.g(n + part, k) for k in range(T)]).cpu().numpy()
            close(got if i < 3 else got[0], g64["%s%d" % (kind, i)], g32["%s%d" % (kind, i)], n + part)


def test_balanced_replay_rows_and_recorded_targets(dev):
    """BalancedExperienceReplay on the device ring: the reference's recorded batches (rewards = sequence numbers) through
    store / deferred visibility / eviction / gather; and the recorded targets of CILAgent.learn_from_batch as dy"""
    import os
    import torch
    from coach_amd.memories.memory import MemoryGranularity
    from coach_amd.memories.non_episodic.balanced_experience_replay import BalancedExperienceReplay
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cil.npz"))
    mem = BalancedExperienceReplay((MemoryGranularity.Transitions, 10), True, 3, 'class', class_column=1, device=dev,
                                   observation_shape=(2,), action_dim=2)
    t = lambda v, dt=torch.float32: torch.tensor(v, dtype=dt, device=dev)
    mem.reset(t([[0.0, float(g["mem_classes"][0])]]))
    for i, c in enumerate(g["mem_classes"]):
        nxt = t([[i + 1.0, float(g["mem_classes"][(i + 1) % 16])]])
        mem.store(t([[i, -i]]), t([float(i)]), t([0], torch.uint8), nxt, nxt, classes_host=[c], defer=i % 2 == 0)
    mem.commit_pending()
    np.random.seed(7)
    for want in g["mem_dup"]:
        b = mem.sample(6)
        assert np.array_equal(b.rewards().cpu().numpy(), want) and np.array_equal(b.actions().cpu().numpy()[:, 0], want)
        assert np.array_equal(b._states["observation"].cpu().numpy(), np.stack([want, g["mem_classes"][want.astype(int)]], 1))
    mem.check_status()


def test_agent_acts_by_command_and_trains_as_its_network(dev):
    """CILAgent over an 8-wide observation whose column 3 is the command: acting is the command's head on the other seven
    columns, whatever the phase; three train() calls (eager, captured, replayed) move the weights exactly as a twin
    CILNet fed the same rows directly, dropout masks included"""
    import torch
    from coach_amd.agents.cil_agent import CILAgent
    from coach_amd.core_types import RunPhase
    from coach_amd.environments.synthetic_vector_environment import (SyntheticVectorEnvironment,
                                                                      SyntheticVectorEnvironmentParameters)
    from coach_amd.memories.memory import MemoryGranularity
    from coach_amd.nn.networks import CILNet, cil_net_kwargs
    from test_cil_host import _preset
    ap, K, A, N, B = _preset(), 4, 2, 24, 8
    net_p = ap.network_wrappers['main']
    net_p.batch_size, net_p.embedder_scheme, net_p.middleware_scheme = B, [32], [48]
    ap.memory.max_size, ap.seed = (MemoryGranularity.Transitions, 64), SEED
    ep = SyntheticVectorEnvironmentParameters("vector", 1, (8,), None, action_dim=A, episode_length=4)
    ep.observation_slices = {"camera": (0, 3), "high_level_command": (3, 4), "measurements": (4, 8)}
    agent = CILAgent(ap, SyntheticVectorEnvironment(ep, dev), use_graphs=True)
    twin = CILNet(dev, (7,), A, **cil_net_kwargs(net_p, SEED))
    rng = np.random.RandomState(5)
    obs, act = rng.randn(N + 1, 8).astype(np.float32), rng.randn(N, A).astype(np.float32)
    obs[:, 3] = np.arange(N + 1) % K
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rest = lambda o: t(np.delete(o, 3, axis=1))
    state = t(obs[2:3])                                                  # (a static buffer: acting is captured)
    for phase in (RunPhase.TRAIN, RunPhase.TEST):
        agent.phase = phase
        got = agent.choose_action(state).cpu().numpy()
        assert np.array_equal(got, twin.predict(rest(obs[2:3]), 1).cpu().numpy()[int(obs[2, 3])])
    agent.memory.reset(t(obs[:1]))
    for i in range(N):
        assert agent._store_extra_host(None, True)["classes_host"].tolist() == [i % K]
        agent.memory.store(t(act[i:i + 1]), t(np.zeros(1, np.float32)), t(np.zeros(1, np.uint8)), t(obs[i + 1:i + 2]),
                           t(obs[i + 1:i + 2]), classes_host=[i % K])
    agent.phase, agent.debug_draws = RunPhase.TRAIN, []
    for update in range(3):
        loss = agent.train()
        rows = agent.debug_draws[update]
        assert (obs[rows, 3] == np.repeat(np.arange(K), B // K)).all()                  # class-major
        want = twin.learn_from_batch(rest(obs[rows]), B, t(obs[rows, 3].astype(np.int32)), t(act[rows]))
        assert loss.item() == want.item() and agent.networks["main"].stack.draw_used.item() == update
    assert torch.equal(agent.networks["main"].params.weights, twin.params.weights)
    agent.check_status()
    state.fill_(float(K))                                                # a command past the last branch
    agent.choose_action(state)
    with pytest.raises(ValueError, match="status bits"):
        agent.check_status()
