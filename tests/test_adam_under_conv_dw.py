"""The Adam step split over two launches: the early blocks (rlx_adam_tf1_step_early, or riders of the convolution
weight-gradient launch, rlx_conv_dw_multi_adam) and the late blocks + finish (rlx_adam_tf1_step_late), against the one
launch of rlx_adam_tf1_step.  Nothing but the launch a block runs in changes, so every comparison is torch.equal."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ACC = 6


def _c2_layout():
    from test_adam_split_blocks import C2_FC, C2_N
    return C2_N, [C2_FC]


def _library_cases():
    c2_n, c2_fc = _c2_layout()
    return {
        # n, ranges, workspace cap of the partial sums (None: 1024)
        "one_run_per_block_with_tail": (4099, [(1024, 3072)], None),
        # 3 blocks of 4 runs each: blocks 1 and 2 early (every run inside a range), block 0 owns the tail
        "capped_grid_four_runs": (12001, [(1024, 3072), (4096, 6144), (7168, 9216), (10240, 12001)], 3),
        "nothing_early": (4099, [], None),
        "everything_in_range_empty_block_late": (8192, [(0, 8192)], None),
        "c2_fc_range": (c2_n, c2_fc, None),
    }


@pytest.mark.parametrize("case", sorted(_library_cases()))
def test_early_plus_late_equals_one_launch(rlx, dev, case):
    import torch
    from coach_amd import _rlx
    n, ranges, cap = _library_cases()[case]
    ws_floats = 1024 if cap is None else cap
    blocks = ctypes.c_int()
    rlx.adam_step_blocks(n, ws_floats, ctypes.byref(blocks))
    nb = blocks.value
    assert nb >= 1
    flat = (ctypes.c_longlong * max(1, 2 * len(ranges)))(*[x for r in ranges for x in r])
    early, late = (ctypes.c_int * nb)(), (ctypes.c_int * nb)()
    ne, nl = ctypes.c_int(), ctypes.c_int()
    rlx.adam_split_blocks(n, nb, flat if ranges else None, len(ranges), early, ctypes.byref(ne), late, ctypes.byref(nl))
    if case == "nothing_early":
        assert ne.value == 0
    else:
        assert ne.value >= 1
    lists = torch.tensor(list(early[:ne.value]) + list(late[:nl.value]), dtype=torch.int32, device=dev)

    gen = torch.Generator(device="cpu").manual_seed(1234)
    rand = lambda: torch.randn(n, generator=gen, dtype=torch.float32).to(dev)
    lr, b1, b2, eps, scale = 2.5e-4, 0.9, 0.99, 1e-4, 0.5

    def fresh():
        gen.manual_seed(99)
        w, m, v = rand(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        state = torch.tensor([b1, b2], dtype=torch.float32, device=dev)
        return dict(w=w, m=m, v=v, state=state, norm=torch.zeros(1, device=dev), acc=torch.zeros(N_ACC, device=dev),
                    ticket=torch.zeros(_rlx.ADAM_TICKET_WORDS, dtype=torch.int32, device=dev),
                    part=torch.full((max(nb, ws_floats),), float("nan"), device=dev))
    one, two = fresh(), fresh()
    gen.manual_seed(7)
    grads = [rand() for _ in range(3)]
    src = [torch.randn(N_ACC, generator=gen).to(dev) for _ in range(3)]
    stream = _rlx.current_stream()
    for g, s in zip(grads, src):
        a = one
        rlx.adam_tf1_step(a["w"], g, a["m"], a["v"], n, lr, b1, b2, eps, a["state"], scale, a["norm"], a["part"], ws_floats,
                          s, a["acc"], N_ACC, None, 0.0, a["ticket"], stream)
        b = two
        d = _rlx.AdamSplitDesc()
        d.weights, d.grads, d.m, d.v, d.n = b["w"].data_ptr(), g.data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), n
        d.learning_rate, d.beta1, d.beta2, d.epsilon, d.grad_scale = lr, b1, b2, eps, scale
        d.state, d.partials, d.blocks = b["state"].data_ptr(), b["part"].data_ptr(), nb
        d.early, d.late, d.n_early, d.n_late = lists.data_ptr(), lists.data_ptr() + 4 * ne.value, ne.value, nl.value
        rlx.adam_tf1_step_early(ctypes.byref(d), 256 if n > 100000 else 2, stream)      # 2: a workgroup loops over blocks
        rlx.adam_tf1_step_late(ctypes.byref(d), b["norm"], s, b["acc"], N_ACC, b["ticket"], stream)
        torch.cuda.synchronize()
        for k in ("w", "m", "v", "state", "norm", "acc"):
            assert torch.equal(one[k], two[k]), (case, k)
        assert torch.equal(one["part"][:nb], two["part"][:nb])
        assert int(two["ticket"].abs().sum()) == 0                  # re-armed
    assert float(one["norm"]) > 0 and torch.isfinite(one["w"]).all()


# ------------------------------------------------------------------ riders: the agent's two calls, switch on / off
def _agent(dev, B, n_env, L, use_graphs=False):
    from coach_amd.agents.clipped_ppo_agent import ClippedPPOAgent, ClippedPPOAgentParameters
    from coach_amd.core_types import EnvironmentSteps
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    env = SyntheticVectorEnvironment(SyntheticVectorEnvironmentParameters("image", n_env, (84, 84), 6, episode_length=L,
                                                                          seed=1234), dev)
    ap = ClippedPPOAgentParameters()
    ap.seed = 0
    ap.algorithm.num_consecutive_playing_steps = EnvironmentSteps(n_env * L)
    ap.network_wrappers["main"].batch_size = B
    agent = ClippedPPOAgent(ap, env, dev, use_graphs=use_graphs)
    for _ in range(L):
        agent.act()
    assert agent._should_train()
    agent.networks["main"].update_target(1.0)
    agent.fill_advantages()
    return agent


def _snapshot(net):
    return dict(w=net.params.weights.clone(), m=net.adam.m.clone(), v=net.adam.v.clone(), state=net.adam.state.clone())


@functools.lru_cache(maxsize=None)
def _three_updates(B, switch, hook):
    """three minibatch updates through ClippedPPOAgent._minibatch_fb / _minibatch_finish from a fixed seed ->
    (snapshot after every update, loss scalars + norm of every update, signal sums, updates that ran as early + late)"""
    import torch
    from coach_amd import _rlx
    from coach_amd.agents.clipped_ppo_agent import ClippedPPOAgent
    dev = torch.device("cuda:0")
    n_env, L = (64, 3) if B == 64 else (8, 4)
    saved = ClippedPPOAgent.ADAM_UNDER_CONV_DW
    ClippedPPOAgent.ADAM_UNDER_CONV_DW = switch
    try:
        agent = _agent(dev, B, n_env, L)
        net = agent.networks["main"]
        n = agent.memory.num_transitions()
        assert n >= 3 * B
        full = np.zeros(agent.perm_dev.numel(), dtype=np.int32)
        full[:n] = np.random.RandomState(5).permutation(n)
        agent._perm.push(full)
        net.set_clip_rescaler(1.0)
        epoch = agent._gather_epoch(n)
        agent.scalar_acc.zero_()
        snaps, scalars = [], []
        for i in range(3):
            if hook:
                _rlx.GEMM_HOOK = [].append
            try:
                agent._minibatch_fb(B, None, i=i, epoch=epoch)
                agent._minibatch_finish(1.0)
            finally:
                _rlx.GEMM_HOOK = None
            snaps.append(_snapshot(net))
            scalars.append(net.scalars[:6].clone())
        agent.check_status()
        return snaps, scalars, agent.scalar_acc.clone(), net.adam.split_steps
    finally:
        ClippedPPOAgent.ADAM_UNDER_CONV_DW = saved


def _assert_same(a, b, what):
    import torch
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("B", [2, 3, 8, 64])       # 3: one half-empty image pair; 64: the benchmark's minibatch
def test_riders_leave_what_the_one_launch_step_leaves(rlx, dev, B):
    import torch
    on, off = _three_updates(B, True, False), _three_updates(B, False, False)
    assert off[3] == 0
    assert on[3] == 3, "the early step did not ride on the convolution weight-gradient launch at this batch"
    for i in range(3):
        _assert_same(on[0][i], off[0][i], "update %d" % i)
        assert torch.equal(on[1][i], off[1][i]), i                 # loss scalars and gradient norm
    assert torch.equal(on[2], off[2])                              # their running sums
    assert not torch.equal(off[0][0]["w"], off[0][1]["w"])


@pytest.mark.parametrize("B", [3, 64])
def test_recorder_hook_keeps_the_plain_path(rlx, dev, B):
    hooked, off = _three_updates(B, True, True), _three_updates(B, False, False)
    assert hooked[3] == 0                                          # no launch that could be replayed applied Adam
    _assert_same(hooked[0][0], off[0][0], "first update under GEMM_HOOK")
    _assert_same(hooked[0][2], off[0][2], "third update under GEMM_HOOK")


def test_finish_with_another_scale_raises(rlx, dev):
    from coach_amd.agents.clipped_ppo_agent import ClippedPPOAgent
    saved = ClippedPPOAgent.ADAM_UNDER_CONV_DW
    ClippedPPOAgent.ADAM_UNDER_CONV_DW = True
    try:
        agent = _agent(dev, 8, 8, 4)
        net = agent.networks["main"]
        n = agent.memory.num_transitions()
        agent._perm.push(np.arange(agent.perm_dev.numel(), dtype=np.int32) % n)
        net.set_clip_rescaler(1.0)
        epoch = agent._gather_epoch(n)
        agent._minibatch_fb(8, None, i=0, epoch=epoch)
        with pytest.raises(ValueError, match="gradient scale"):
            agent._minibatch_finish(0.5)
    finally:
        ClippedPPOAgent.ADAM_UNDER_CONV_DW = saved


def test_captured_epochs_match(rlx, dev):
    """train_network with hipGraphs (first epoch eager, second captured, third replayed): the split's device lists are
    built before the capture, and the replayed riders leave what the one-launch step leaves."""
    import random
    import torch
    from coach_amd.agents.clipped_ppo_agent import ClippedPPOAgent
    out = {}
    saved = ClippedPPOAgent.ADAM_UNDER_CONV_DW
    try:
        for switch in (True, False):
            ClippedPPOAgent.ADAM_UNDER_CONV_DW = switch
            agent = _agent(dev, 8, 8, 4, use_graphs=True)
            n = agent.memory.num_transitions()
            random.seed(11)
            res = agent.train_network(list(range(n)), 3)
            torch.cuda.synchronize()
            net = agent.networks["main"]
            out[switch] = (_snapshot(net), torch.stack([r.clone() for r in res]), net.adam.split_steps)
    finally:
        ClippedPPOAgent.ADAM_UNDER_CONV_DW = saved
    assert out[True][2] > 0 and out[False][2] == 0
    _assert_same(out[True][0], out[False][0], "after three epochs")
    assert torch.equal(out[True][1], out[False][1])
