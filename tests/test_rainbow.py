"""Rainbow DQN on the device: rlx_rainbow_head_loss, rlx_rainbow_argmax / rlx_rainbow_egreedy (csrc/rainbow.hip) and
rlx_nstep_episode_store (csrc/nstep_store.hip) against the numpy restatement (tests/rainbow_ref.py, itself pinned to the
reference by tests/test_rainbow_ref.py) and against the kernels they share arithmetic with; the n-step prioritized memory
against the restatement's host loop and the reference's recorded trace; RainbowNet against a host composition of twin
layers; the agent's loop.

Tolerances: merged logits, a*, m, the zero pattern of the gradients and everything integer are compared exactly.  The
loss, the per-action losses and the PER errors differ from the restatement by the device's logf and fp32 summation order:
tests/tolerances.py's LOSS fits them, OUT fits the gradients (p - m and its per-atom means)."""
import numpy as np
import pytest

import c51_ref as C
import rainbow_ref as R
from tolerances import LOSS, OUT

pytestmark = pytest.mark.gpu

SUPPORTS = {"c51": (-10.0, 10.0), "wide": (0.0, 200.0)}
DISCOUNT, N_STEP = 0.99, 3


def _t(x, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _workspace(dev):
    import torch
    return torch.zeros(256, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)


def _launch(rlx, dev, streams, z, actions, returns, boot, discount_n, ws, ticket, grad_scale=1.0, optional=True,
            pad=0):
    """streams: (v, x, v_next_target, x_next_target, v_next_online, x_next_online), v [B, N], x [B, A, N].  pad: extra
    columns behind every row (leading dimensions larger than the rows)."""
    import torch
    B, A, N = streams[1].shape
    AN = A * N

    def padded(a, cols):
        out = np.full((B, cols + pad), np.nan, dtype=np.float32)
        out[:, :cols] = a.reshape(B, cols)
        return _t(out, dev)
    dv = torch.full((B, N + pad), float("nan"), dtype=torch.float32, device=dev)
    dx = torch.full((B, AN + pad), float("nan"), dtype=torch.float32, device=dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    o = dict(m=torch.zeros(B, N, dtype=torch.float32, device=dev), a_star=torch.zeros(B, dtype=torch.int32, device=dev),
             ce=torch.zeros(B, A, dtype=torch.float32, device=dev),
             merged=torch.zeros(B, AN, dtype=torch.float32, device=dev),
             dlogits=torch.full((B, AN), float("nan"), dtype=torch.float32, device=dev),
             err=torch.full((B,), float("nan"), dtype=torch.float64, device=dev)) if optional else {}
    args = []
    for i in range(3):
        args += [padded(streams[2 * i], N), N + pad, padded(streams[2 * i + 1], AN), AN + pad]
    rlx.rainbow_head_loss(*args, _t(z, dev), _t(np.asarray(actions).astype(np.int32), dev),
                          _t(np.asarray(returns, dtype=np.float64), dev), _t(np.asarray(boot).astype(np.uint8), dev),
                          float(discount_n), N, A, B, float(grad_scale), dv, N + pad, dx, AN + pad, o.get("err"), ws,
                          ticket, loss, status, o.get("m"), o.get("a_star"), o.get("ce"), o.get("merged"),
                          o.get("dlogits"), 0)
    torch.cuda.synchronize()
    out = dict(loss=loss.cpu().numpy()[0], status=int(status.item()), dv=dv.cpu().numpy()[:, :N],
               dx=dx.cpu().numpy()[:, :AN].reshape(B, A, N))
    if optional:
        out.update(a_star=o["a_star"].cpu().numpy(), m=o["m"].cpu().numpy(), action_losses=o["ce"].cpu().numpy(),
                   merged=o["merged"].cpu().numpy().reshape(B, A, N),
                   dlogits=o["dlogits"].cpu().numpy().reshape(B, A, N), errors=o["err"].cpu().numpy())
    return out


def _inputs(rng, B, A, N, support):
    z = C.support(*SUPPORTS[support], N)
    streams = []
    for _ in range(3):
        streams += [(rng.randn(B, N) * 2).astype(np.float32), (rng.randn(B, A, N) * 2).astype(np.float32)]
    actions = rng.randint(0, A, size=B)
    # returns on the support's scale; the wide support gets what three rewards of 1 give, as CartPole does
    boot = rng.rand(B) >= 0.3
    if support == "wide":
        full = R.nstep_returns(np.ones(7, np.float32), N_STEP, DISCOUNT)      # [2.9701 x 5, 1.99, 1]
        returns = full[rng.randint(0, 7, size=B)]
    else:
        returns = rng.randn(B) * 2
    boot[0] = True
    if B > 1:                                        # a row of an episode shorter than n: one reward, no bootstrap
        boot[1] = False
        returns[1] = 1.0
    return z, streams, actions, returns, boot


@pytest.mark.parametrize("support", sorted(SUPPORTS))
@pytest.mark.parametrize("N", [2, 51, 256])
@pytest.mark.parametrize("A", [2, 6, 18])
@pytest.mark.parametrize("B", [1, 32, 37])
def test_loss_kernel_equals_the_restatement(rlx, dev, B, A, N, support):
    rng = np.random.RandomState(B * 1000 + A * 10 + N)
    z, streams, actions, returns, boot = _inputs(rng, B, A, N, support)
    ws, ticket = _workspace(dev)
    dn = DISCOUNT ** N_STEP
    k = _launch(rlx, dev, streams, z, actions, returns, boot, dn, ws, ticket, pad=3)
    assert C.overhangs(z) == (N == 256 and support == "c51")
    r = R.update(*streams, z, actions, returns, boot, dn, overhang="drop" if C.overhangs(z) else "raise")
    rows = np.arange(B)
    print("\n  B %d A %d N %d %s: loss %.6g (twin %.6g, rel %.2e), max |dlogits - twin| %.2e, |dv - twin| %.2e, "
          "|dx - twin| %.2e, max rel error diff %.2e"
          % (B, A, N, support, k["loss"], r["loss"], abs(k["loss"] - r["loss"]) / abs(r["loss"]),
             np.abs(k["dlogits"] - r["dlogits"]).max(), np.abs(k["dv"] - r["dv"]).max(),
             np.abs(k["dx"] - r["dx"]).max(),
             (np.abs(k["errors"] - r["errors"]) / np.maximum(np.abs(r["errors"]), 1e-30)).max()))
    assert k["status"] == 0 and int(ticket.item()) == 0
    assert np.array_equal(_bits(k["merged"]), _bits(r["merged"]))
    assert np.array_equal(k["a_star"], r["a_star"])
    assert np.array_equal(_bits(k["m"]), _bits(r["m"]))
    off = np.ones((B, A), bool)
    off[rows, actions] = False
    for name in ("dlogits", "dv", "dx"):
        assert not np.isnan(k[name]).any()
        assert np.array_equal(k[name] == 0.0, r[name] == 0.0), name
    assert np.all(k["dlogits"][off] == 0.0) and np.any(k["dlogits"][rows, actions] != 0.0)
    np.testing.assert_allclose(k["loss"], r["loss"], **LOSS)
    np.testing.assert_allclose(k["action_losses"], r["action_losses"], **LOSS)
    np.testing.assert_allclose(k["errors"], r["errors"], **LOSS)
    for name in ("dlogits", "dv", "dx"):
        np.testing.assert_allclose(k[name], r[name], **OUT)
    assert k["errors"].dtype == np.float64
    assert np.array_equal(k["errors"], k["action_losses"][rows, actions].astype(np.float64))
    # a second launch, without the optional outputs: the same bytes, the ticket back at zero
    again = _launch(rlx, dev, streams, z, actions, returns, boot, dn, ws, ticket, optional=False, pad=3)
    assert int(ticket.item()) == 0
    for name in ("loss", "dv", "dx"):
        assert again[name].tobytes() == k[name].tobytes(), name


@pytest.mark.parametrize("B,A,N", [(37, 6, 51), (5, 18, 256), (32, 2, 2)])
def test_merge_and_its_gradient_equal_the_dueling_kernels_per_atom(rlx, dev, B, A, N):
    """merged logits == rlx_dueling_combine and (dv, dx) == rlx_dueling_combine_backward on dlogits_out, with every
    (row, atom) pair as one row of those kernels — bit for bit."""
    import torch
    rng = np.random.RandomState(7 + N)
    z, streams, actions, returns, boot = _inputs(rng, B, A, N, "c51")
    ws, ticket = _workspace(dev)
    k = _launch(rlx, dev, streams, z, actions, returns, boot, DISCOUNT ** N_STEP, ws, ticket, grad_scale=0.5)
    v, x = streams[0], streams[1]
    adv = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(B * N, A)             # row b*N + j, column a
    q = torch.zeros(B * N, A, dtype=torch.float32, device=dev)
    rlx.dueling_combine(_t(v.reshape(B * N), dev), _t(adv, dev), B * N, A, q, 0)
    y = q.cpu().numpy().reshape(B, N, A).transpose(0, 2, 1)
    assert np.array_equal(_bits(k["merged"]), _bits(y))
    dq = np.ascontiguousarray(k["dlogits"].transpose(0, 2, 1)).reshape(B * N, A)
    dv = torch.zeros(B * N, dtype=torch.float32, device=dev)
    dadv = torch.zeros(B * N, A, dtype=torch.float32, device=dev)
    rlx.dueling_combine_backward(_t(dq, dev), B * N, A, dv, dadv, 0)
    assert np.array_equal(_bits(k["dv"]), _bits(dv.cpu().numpy().reshape(B, N)))
    assert np.array_equal(_bits(k["dx"]), _bits(dadv.cpu().numpy().reshape(B, N, A).transpose(0, 2, 1)))


@pytest.mark.parametrize("support", sorted(SUPPORTS))
@pytest.mark.parametrize("B,A,N", [(37, 6, 51), (32, 2, 51), (5, 18, 256), (3, 4, 2)])
def test_one_step_case_equals_the_c51_kernel_on_the_merged_logits(rlx, dev, B, A, N, support):
    """online(s') == target(s'), returns == rewards, bootstrap == 1 - game_over, discount_n == discount: a*, m, dlogits,
    the loss and the errors are rlx_c51_head_loss's on the merged logits, bit for bit."""
    import torch
    rng = np.random.RandomState(B + A + N)
    z, streams, actions, _, _ = _inputs(rng, B, A, N, support)
    streams[4], streams[5] = streams[2], streams[3]
    rewards = np.ones(B, np.float32) if support == "wide" else rng.randn(B).astype(np.float32)
    go = rng.rand(B) < 0.3
    ws, ticket = _workspace(dev)
    k = _launch(rlx, dev, streams, z, actions, rewards.astype(np.float64), ~go, DISCOUNT, ws, ticket)
    y, y_next = R.merge(streams[0], streams[1]), R.merge(streams[2], streams[3])
    assert np.array_equal(_bits(k["merged"]), _bits(y))
    AN = A * N
    d = torch.full((B, AN), float("nan"), dtype=torch.float32, device=dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    m = torch.zeros(B, N, dtype=torch.float32, device=dev)
    a_star = torch.zeros(B, dtype=torch.int32, device=dev)
    ce = torch.zeros(B, A, dtype=torch.float32, device=dev)
    err = torch.zeros(B, dtype=torch.float64, device=dev)
    rlx.c51_head_loss(_t(y.reshape(B, AN), dev), AN, _t(y_next.reshape(B, AN), dev), AN, _t(z, dev),
                      _t(actions.astype(np.int32), dev), _t(rewards, dev), _t(go.astype(np.uint8), dev), DISCOUNT, N, A,
                      B, 1.0, d, AN, err, ws, ticket, loss, status, m, a_star, ce, 0)
    torch.cuda.synchronize()
    assert np.array_equal(k["a_star"], a_star.cpu().numpy())
    assert np.array_equal(_bits(k["m"]), _bits(m.cpu().numpy()))
    assert np.array_equal(_bits(k["dlogits"]), _bits(d.cpu().numpy().reshape(B, A, N)))
    assert np.array_equal(_bits(k["action_losses"]), _bits(ce.cpu().numpy()))
    assert k["loss"].tobytes() == loss.cpu().numpy()[0].tobytes()
    assert np.array_equal(_bits(k["errors"]), _bits(err.cpu().numpy()))


def test_acting_kernels_equal_the_categorical_ones_on_the_merged_logits(rlx, dev):
    import torch
    rng = np.random.RandomState(11)
    for n_env, A, N, support in ((5, 2, 51, "c51"), (9, 6, 51, "wide"), (4, 18, 2, "c51"), (3, 4, 256, "c51"),
                                 (3, 18, 256, "wide")):
        z = C.support(*SUPPORTS[support], N)
        v = (rng.randn(n_env, N) * 2).astype(np.float32)
        x = (rng.randn(n_env, A, N) * 2).astype(np.float32)
        x[0, 1] = x[0, 0]                                  # exact ties: the tie uniforms decide / the first one wins
        x[1, :] = x[1, 0]
        y = R.merge(v, x)
        assert np.array_equal(y[1, 0], y[1, A - 1])
        u = rng.rand(n_env)
        u[:3] = 0.9
        ra = rng.randint(0, A, size=n_env).astype(np.int32)
        tie = rng.rand(n_env, A)
        zd, yd = _t(z, dev), _t(y.reshape(n_env, A * N), dev)
        vd, xd = _t(v, dev), _t(x.reshape(n_env, A * N), dev)

        def outs():
            return (torch.zeros(n_env, A, dtype=torch.float64, device=dev),
                    torch.full((n_env,), -1, dtype=torch.int32, device=dev))
        (q0, a0), (q1, a1), (q2, a2), (q3, a3) = outs(), outs(), outs(), outs()
        rlx.categorical_argmax(yd, A * N, zd, N, n_env, A, q0, a0, 0)
        rlx.rainbow_argmax(vd, N, xd, A * N, zd, N, n_env, A, q1, a1, 0)
        rlx.categorical_egreedy(yd, A * N, zd, N, _t(u, dev), _t(ra, dev), _t(tie, dev), 0.5, n_env, A, q2, a2, 0)
        rlx.rainbow_egreedy(vd, N, xd, A * N, zd, N, _t(u, dev), _t(ra, dev), _t(tie, dev), 0.5, n_env, A, q3, a3, 0)
        q = q1.cpu().numpy()
        assert np.array_equal(_bits(q), _bits(q0.cpu().numpy())) and torch.equal(a0, a1)
        assert np.array_equal(_bits(q3.cpu().numpy()), _bits(q2.cpu().numpy())) and torch.equal(a2, a3)
        assert np.array_equal(q, C.q_values_device_order(C.softmax(y), z))
        assert a1.cpu().numpy().tolist() == np.argmax(q, axis=1).tolist()
        assert a3.cpu().numpy().tolist() == C.egreedy(q, u, ra, tie, 0.5).tolist()
        assert int(a1[1].item()) == 0 and q[1, 0] == q[1, A - 1]              # an exact tie takes the first action
        a4 = torch.full((n_env,), -1, dtype=torch.int32, device=dev)          # without the optional output
        rlx.rainbow_argmax(vd, N, xd, A * N, zd, N, n_env, A, None, a4, 0)
        assert torch.equal(a1, a4)


def test_loss_kernel_flags_an_action_out_of_range_and_refuses_large_shapes(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    rng = np.random.RandomState(2)
    B, A, N = 4, 3, 8
    z, streams, _, returns, boot = _inputs(rng, B, A, N, "c51")
    actions = np.array([0, 3, 1, -1])
    ws, ticket = _workspace(dev)
    k = _launch(rlx, dev, streams, z, actions, returns, boot, DISCOUNT ** N_STEP, ws, ticket)
    assert k["status"] == 1 and int(ticket.item()) == 0
    for b in (1, 3):
        assert np.all(k["dlogits"][b] == 0) and np.all(k["dv"][b] == 0) and np.all(k["dx"][b] == 0)
        assert k["errors"][b] == 0.0
    assert np.any(k["dv"][0] != 0) and np.any(k["dx"][2] != 0)
    zd = _t(C.support(-10.0, 10.0, 4), dev)
    ld = 19 * 257
    for n_atoms, n_actions, batch in ((4, 19, 1), (257, 1, 1), (1, 2, 1), (4, 2, 257)):
        big = torch.zeros(max(batch, 1), ld, dtype=torch.float32, device=dev)
        with pytest.raises(RlxError):
            rlx.rainbow_head_loss(big, ld, big, ld, big, ld, big, ld, big, ld, big, ld, zd, ticket, zd, ticket, 0.97,
                                  n_atoms, n_actions, batch, 1.0, big, ld, big, ld, None, ws, ticket, ws, ticket, None,
                                  None, None, None, None, 0)
    big = torch.zeros(1, ld, dtype=torch.float32, device=dev)
    with pytest.raises(RlxError):          # a value stream narrower than the atoms
        rlx.rainbow_head_loss(big, 3, big, ld, big, ld, big, ld, big, ld, big, ld, zd, ticket, zd, ticket, 0.97, 4, 2,
                              1, 1.0, big, ld, big, ld, None, ws, ticket, ws, ticket, None, None, None, None, None, 0)
    with pytest.raises(RlxError):
        rlx.rainbow_egreedy(big, ld, big, ld, zd, 4, zd, ticket, zd, 0.5, 1, 19, None, ticket, 0)
    with pytest.raises(RlxError):
        rlx.rainbow_argmax(big, ld, big, ld, zd, 257, 1, 2, None, ticket, 0)


# ----------------------------------------------------------------------------------------------- the episode store
def _episode(rng, T, D):
    obs = rng.randn(T + 1, D).astype(np.float32)
    return dict(obs=obs[:-1], next_obs=obs[1:] + np.float32(0.5), action=rng.randint(0, 5, size=T).astype(np.int32),
                reward=rng.randn(T).astype(np.float32), game_over=(np.arange(T) == T - 1).astype(np.uint8))


@pytest.mark.parametrize("T", [1, 2, 3, 4, 7])
def test_episode_store_kernel_equals_the_restatement(rlx, dev, T):
    """one launch per episode: every column, the redirected next states, the flags; the returns column has the bits of
    rlx_episode_nstep_returns; the destination wraps the ring's end; rows outside it are untouched."""
    import torch
    rng = np.random.RandomState(T)
    D, L, n_env, env, rows = 5, 9, 3, 1, 10
    ep = _episode(rng, T, D)
    st = dict(obs=np.zeros((n_env, L, D), np.float32), next_obs=np.zeros((n_env, L, D), np.float32),
              action=np.zeros((n_env, L), np.int32), reward=np.zeros((n_env, L), np.float32),
              game_over=np.zeros((n_env, L), np.uint8))
    for key in st:
        st[key][...] = 77                              # other envs' rows and the rows behind T must not be read
        st[key][env, :T] = ep[key]
    dst0 = rows - 2                                    # T > 2 wraps
    ring = dict(obs=torch.full((rows, D), -5.0, device=dev), next_obs=torch.full((rows, D), -5.0, device=dev),
                action=torch.full((rows,), -5, dtype=torch.int32, device=dev), reward=torch.full((rows,), -5.0, device=dev),
                game_over=torch.full((rows,), 9, dtype=torch.uint8, device=dev),
                ret=torch.full((rows,), -5.0, dtype=torch.float64, device=dev),
                boot=torch.full((rows,), 9, dtype=torch.uint8, device=dev))
    rlx.nstep_episode_store(_t(st["obs"], dev), _t(st["next_obs"], dev), _t(st["action"], dev), _t(st["reward"], dev),
                            _t(st["game_over"], dev), env, n_env, L, T, N_STEP, DISCOUNT, D, 1, ring["obs"],
                            ring["next_obs"], ring["action"], ring["reward"], ring["game_over"], ring["ret"],
                            ring["boot"], dst0, rows, 0)
    nxt, boot, ret = R.process_episode(ep["reward"], N_STEP, DISCOUNT)
    dst = (dst0 + np.arange(T)) % rows
    got = {k: v.cpu().numpy() for k, v in ring.items()}
    for key in ("obs", "action", "reward", "game_over"):
        assert np.array_equal(got[key][dst], ep[key]), key
    want_next = np.stack([ep["obs"][nxt[k]] if boot[k] else ep["next_obs"][T - 1] for k in range(T)])
    assert np.array_equal(got["next_obs"][dst], want_next)
    assert np.array_equal(got["boot"][dst], boot.astype(np.uint8))
    assert np.array_equal(_bits(got["ret"][dst]), _bits(ret))
    compact = torch.zeros(T, dtype=torch.float64, device=dev)
    rlx.episode_nstep_returns(_t(ep["reward"], dev), None, compact, 0, T, 0, 1, T, DISCOUNT, N_STEP, 0)
    assert np.array_equal(_bits(got["ret"][dst]), _bits(compact.cpu().numpy()))
    rest = np.setdiff1d(np.arange(rows), dst)
    assert np.all(got["obs"][rest] == -5.0) and np.all(got["boot"][rest] == 9) and np.all(got["ret"][rest] == -5.0)


def test_episode_store_kernel_refuses_what_does_not_fit(rlx, dev):
    import torch
    from coach_amd._rlx import RlxError
    f = torch.zeros(64, dtype=torch.float32, device=dev)
    i = torch.zeros(64, dtype=torch.int32, device=dev)
    b = torch.zeros(64, dtype=torch.uint8, device=dev)
    d = torch.zeros(64, dtype=torch.float64, device=dev)
    # (env, n_env, stage_len, length, n_step, ring rows, dst0)
    for env, n_env, L, T, n, rows, dst0 in ((0, 1, 4, 5, 3, 8, 0), (0, 1, 8, 5, 3, 4, 0), (1, 1, 8, 2, 3, 8, 0),
                                            (0, 1, 8, 2, 0, 8, 0), (0, 1, 8, 2, 3, 8, 8), (0, 1, 8, 0, 3, 8, 0)):
        with pytest.raises(RlxError):
            rlx.nstep_episode_store(f, f, i, f, b, env, n_env, L, T, n, DISCOUNT, 2, 1, f, f, i, f, b, d, b, dst0, rows, 0)


# ------------------------------------------------------------------------------------------- the n-step memory
def _memory(dev, n_env, cap=16, L=8, D=1):
    from coach_amd.memories.memory import MemoryGranularity
    from coach_amd.memories.non_episodic.nstep_prioritized_experience_replay import NStepPrioritizedExperienceReplay
    from coach_amd.schedules import ConstantSchedule
    return NStepPrioritizedExperienceReplay((MemoryGranularity.Transitions, cap), alpha=0.5, beta=ConstantSchedule(0.4),
                                            n_step=N_STEP, discount=DISCOUNT, max_episode_length=L, device=dev,
                                            n_env=n_env, observation_shape=(D,))


def _mem_step(mem, ref, dev, cur, actions, rewards, overs, next_obs, reset_obs, dones):
    """one vector step into the device memory and the restatement's host loop -> the envs' next current states"""
    mem.store(_t(np.asarray(actions, np.int32), dev), _t(np.asarray(rewards, np.float32), dev),
              _t(np.asarray(overs, np.uint8), dev), _t(np.asarray(next_obs, np.float32), dev),
              _t(np.asarray(reset_obs, np.float32), dev), dones_host=np.asarray(dones, bool))
    ref.step(cur, actions, rewards, overs, next_obs, dones)
    return np.where(np.asarray(dones, bool)[:, None], reset_obs, next_obs).astype(np.float32)


def _assert_ring_equals(mem, ref):
    cols = {"obs": mem.obs, "next_obs": mem.next_obs, "action": mem.action, "reward": mem.reward,
            "game_over": mem.game_over, "n_step_discounted_rewards": mem.n_step_discounted_rewards,
            "should_bootstrap_next_state": mem.should_bootstrap_next_state}
    rows = [r for r in range(mem.rows) if ref.ring[r] is not None]
    assert rows and mem.rows == ref.rows and mem.committed_total == ref.stored
    for key, col in cols.items():
        got, want = col.cpu().numpy()[rows], ref.column(key, rows)
        if want.dtype.kind == "f":
            assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), key
        else:
            assert np.array_equal(got, want), key


def test_memory_equals_the_reference_trace_with_one_env(dev, golden):
    """the recorded trace (make_golden_rainbow.py): five episodes of 4, 7, 3, 1 and 2 transitions into 16 leaves — the
    last two past the ring's end — sampled after the third and the fifth with priority updates in between."""
    import random
    import torch
    g = golden("rainbow")
    lengths, rewards = g["mem_lengths"].tolist(), g["mem_rewards"]
    mem = _memory(dev, 1)
    ref = R.EpisodeStore(1, mem.rows, N_STEP, DISCOUNT)
    assert mem.rows == 17 and mem.power_of_2_size == 16
    cur = np.array([[0.0]], np.float32)
    mem.reset(_t(cur, dev))
    first = 0
    for e, T in enumerate(lengths):
        for k in range(T):
            done = k == T - 1
            assert np.array_equal(mem.current_states().cpu().numpy(), cur)
            before = mem.num_transitions()
            cur = _mem_step(mem, ref, dev, cur, [k % 2], [rewards[first + k]], [done],
                            [[-(first + T) if done else first + k + 1]], [[first + T]], [done])
            if not done:                       # nothing is visible, pending or deferred before the episode ends
                assert mem.num_transitions() == before and mem.pending == 0 and mem.staged_transitions() == k + 1
        first += T
        assert mem.num_transitions() == g["mem_num_transitions"][e] and mem.staged_transitions() == 0
        mem.check_status()
        _assert_ring_equals(mem, ref)
        if e in (2, 4):
            p = "mem%d_" % e
            for tag, seed in (("", 10 + e), ("2", 20 + e)):
                random.seed(seed)
                b = mem.sample(8)
                assert np.array_equal(b.info("idx").cpu().numpy(), g[p + "idx" + tag])
                assert np.array_equal(_bits(b.info("weight").cpu().numpy()), _bits(g[p + "weight" + tag]))
                ids = b.states()["observation"].cpu().numpy()[:, 0]
                assert ids.tolist() == g[p + "state_ids" + tag].tolist()
                rows = [next(r for r in range(mem.rows) if ref.ring[r] is not None and ref.ring[r]["obs"][0] == i)
                        for i in ids]
                for key in ("n_step_discounted_rewards", "should_bootstrap_next_state"):
                    assert np.array_equal(b.info(key).cpu().numpy(), ref.column(key, rows)), key
                assert np.array_equal(b.next_states()["observation"].cpu().numpy(), ref.column("next_obs", rows))
                if tag == "":
                    mem.update_priorities(b.info("idx"), _t(g[p + "errors"], dev))
            assert mem.maximal_priority == float(g[p + "max_priority"])
            assert float(mem.sum_tree[0].item()) == float(g[p + "sum_total"])
    torch.cuda.synchronize()


def test_memory_with_three_envs_ties_a_wrap_and_a_dropped_episode(dev):
    """episodes of 1, 2, 4 / 3, 4 / 7 transitions: the envs finish on different steps, two tie on step 3 and all three on
    step 7 (stored in env order); 21 transitions wrap the 19-row ring; an open episode that is dropped never appears."""
    rng = np.random.RandomState(3)
    n_env, D = 3, 2
    mem = _memory(dev, n_env, D=D)
    ref = R.EpisodeStore(n_env, mem.rows, N_STEP, DISCOUNT)
    assert mem.rows == 19
    ends = [{1, 3, 7}, {3, 7}, {7}]
    state = {"cur": rng.randn(n_env, D).astype(np.float32)}
    mem.reset(_t(state["cur"], dev))

    def step(dones):
        nxt, rst = rng.randn(n_env, D).astype(np.float32), rng.randn(n_env, D).astype(np.float32)
        state["cur"] = _mem_step(mem, ref, dev, state["cur"], rng.randint(0, 4, size=n_env),
                                 rng.randn(n_env).astype(np.float32), dones, nxt, rst, dones)
    for t in range(1, 8):
        step([t in e for e in ends])
        assert mem.num_transitions() == min(16, 2 * ref.stored) and mem.committed_total == ref.stored
        assert np.array_equal(mem.current_states().cpu().numpy(), state["cur"])
    assert ref.stored == 21
    _assert_ring_equals(mem, ref)
    # every written leaf carries the maximal priority 1 ** alpha: the root is the number of live leaves
    assert float(mem.sum_tree[0].item()) == 16.0
    step([False] * 3)                                    # one open step per env ...
    assert mem.staged_transitions() == 3
    mem.drop_pending()                                   # ... which a reset in the middle of the episode discards
    ref.drop()
    state["cur"] = rng.randn(n_env, D).astype(np.float32)
    mem.reset(_t(state["cur"], dev))
    assert mem.staged_transitions() == 0 and mem.committed_total == 21
    step([False] * 3)
    step([True, False, True])
    assert ref.stored == 25 and mem.staged_transitions() == 2
    _assert_ring_equals(mem, ref)
    mem.check_status()


def test_memory_refusals(dev):
    from coach_amd.memories.memory import MemoryGranularity
    from coach_amd.memories.non_episodic.nstep_prioritized_experience_replay import NStepPrioritizedExperienceReplay as M
    size = (MemoryGranularity.Transitions, 16)
    with pytest.raises(ValueError, match="frame-dedup ring"):
        M(size, n_step=3, discount=0.99, max_episode_length=8, device=dev, n_env=1, observation_shape=(84, 84), stack=4)
    with pytest.raises(ValueError, match="n_step >= 2"):
        M(size, n_step=1, discount=0.99, max_episode_length=8, device=dev, n_env=1, observation_shape=(2,))
    mem = M((MemoryGranularity.Transitions, 4), n_step=3, discount=0.99, max_episode_length=8, device=dev, n_env=1,
            observation_shape=(1,))
    z = lambda dt: _t(np.zeros((1,), dt), dev)
    o = _t(np.zeros((1, 1), np.float32), dev)
    mem.reset(o)
    for k in range(5):
        mem.store(z(np.int32), z(np.float32), z(np.uint8), o, o, dones_host=np.array([False]))
    with pytest.raises(ValueError, match="longer than the replay ring"):
        mem.store(z(np.int32), z(np.float32), z(np.uint8), o, o, dones_host=np.array([True]))
    with pytest.raises(ValueError, match="host flags"):
        mem.store(z(np.int32), z(np.float32), z(np.uint8), o, o)


# ------------------------------------------------------------------------------------------------- the network
class _Plain(object):
    """the twin of a G.Dense layer with noisy_agent_ref._Noisy's interface, fp64"""

    def __init__(self, layer):
        self.l = layer

    def forward(self, w, x, key, noise_pass, counter):
        from oracle.nn import act
        l = self.l
        self.x, self.w = np.asarray(x, dtype=np.float64), w
        self.y = act(self.x @ w[l.kname].astype(np.float64) + w[l.bname].astype(np.float64), l.act)
        return self.y

    def backward(self, dy, grads):
        import noisy_ref
        l = self.l
        dz = dy * noisy_ref.act_deriv(self.y, l.act)
        grads[l.kname], grads[l.bname] = self.x.T @ dz, dz.sum(0)
        return dz @ self.w[l.kname].astype(np.float64).T


class RainbowUpdateRef(object):
    """one update of RainbowNet on the host: twin layers (fed the device's noise where the network is noisy),
    rainbow_ref.update, TF1 Adam per tensor."""

    def __init__(self, net, key):
        from noisy_agent_ref import _Noisy
        from oracle.optim import AdamTF1
        twin = _Noisy if net.noisy else _Plain
        self.net, self.key = net, key
        self.online = {k: v[0].copy() for k, v in net.params.named_arrays().items()}
        self.target = {k: v[0].copy() for k, v in net.params.named_arrays(net.target).items()}
        self.torso = [twin(l) for l in net.torso.layers]
        self.v1, self.v2, self.a1, self.a2 = (twin(l) for l in (net.v_fc, net.v_out, net.a_fc, net.a_out))
        self.adam = {k: AdamTF1(v.size, net.adam.lr, net.adam.beta1, net.adam.beta2, net.adam.eps)
                     for k, v in self.online.items()}
        self.step = 0

    def _forward(self, w, obs, noise_pass):
        c, x = self.step, np.asarray(obs, dtype=np.float64)
        for d in self.torso:
            x = d.forward(w, x, self.key, noise_pass, c)
        v = self.v2.forward(w, self.v1.forward(w, x, self.key, noise_pass, c), self.key, noise_pass, c)
        a = self.a2.forward(w, self.a1.forward(w, x, self.key, noise_pass, c), self.key, noise_pass, c)
        B = v.shape[0]
        return v.astype(np.float32), a.astype(np.float32).reshape(B, self.net.A, self.net.N)

    def update(self, obs, next_obs, actions, returns, boot, discount_n):
        vn, xn = self._forward(self.online, next_obs, "online_next")
        vt, xt = self._forward(self.target, next_obs, "target")
        v, x = self._forward(self.online, obs, "online")            # last: its saved tensors serve the backward pass
        r = R.update(v, x, vt, xt, vn, xn, self.net.z_values, actions, returns, boot, discount_n)
        grads, B = {}, len(actions)
        dx = self.v1.backward(self.v2.backward(r["dv"].astype(np.float64), grads), grads) + \
            self.a1.backward(self.a2.backward(r["dx"].reshape(B, -1).astype(np.float64), grads), grads)
        for d in reversed(self.torso):
            dx = d.backward(dx, grads)
        assert set(grads) == set(self.online)
        for k, g in grads.items():
            self.adam[k].step(self.online[k].reshape(-1), np.asarray(g, dtype=np.float64).astype(np.float32).reshape(-1))
        self.step += 1
        return float(r["loss"]), r


@pytest.mark.parametrize("noisy", [True, False])
def test_network_update_equals_the_host_composition(dev, noisy):
    """three learn_from_batch updates of RainbowNet at CartPole's shape (4 -> Dense 256 -> two streams of 512 -> 51 and
    2 x 51 logits, B 32): the first update's loss within LOSS, every parameter after the three Adam steps within WEIGHTS,
    all four tensors of every noisy layer moved."""
    import torch
    from coach_amd.nn.networks import RainbowNet
    from tolerances import WEIGHTS
    B, A, N, dn = 32, 2, 51, DISCOUNT ** N_STEP
    net = RainbowNet(dev, (4,), A, N, v_min=-10.0, v_max=10.0, middleware="Empty", noisy=noisy, seed=3,
                     learning_rate=2.5e-4)
    net.noise_seed, net.noise_rank = 1234, 0
    names = set(net.params.entries)
    hn = "main/rainbow_q_values_head/"
    tensors = ("weight_mean", "bias_mean", "weight_stddev", "bias_stddev") if noisy else ("kernel", "bias")
    assert {hn + s + "/" + f + "/" + t for s in ("state_value", "action_advantage") for f in ("fc1", "fc2")
            for t in tensors} <= names
    assert len(net.noisy_layers) == (5 if noisy else 0) and net._fused is None and net._act is None
    ref = RainbowUpdateRef(net, (1234, 0))
    start = {k: v.copy() for k, v in ref.online.items()}
    rng = np.random.RandomState(17)
    errors = torch.zeros(B, dtype=torch.float64, device=dev)
    a_star = torch.zeros(B, dtype=torch.int32, device=dev)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for step in range(3):
        obs, nxt = (rng.randn(B, 4).astype(np.float32) for _ in range(2))
        actions = rng.randint(0, A, size=B).astype(np.int32)
        returns, boot = rng.randn(B) * 2, (rng.rand(B) >= 0.3).astype(np.uint8)
        loss = net.learn_from_batch(d(obs), d(nxt), B, d(actions), d(returns), d(boot), dn, per_errors=errors,
                                    target_actions_out=a_star)
        net.check_status()
        ref_loss, r = ref.update(obs, nxt, actions, returns, boot, dn)
        print("noisy %s update %d: loss %.7g, restated %.7g" % (noisy, step, float(loss.item()), ref_loss))
        if step == 0:
            np.testing.assert_allclose(float(loss.item()), ref_loss, **LOSS)
            np.testing.assert_allclose(errors.cpu().numpy(), r["errors"], **LOSS)
            net.update_target(1.0)                                 # the later updates see a target of its own
            ref.target = {k: v.copy() for k, v in ref.online.items()}
    got = net.params.named_arrays()
    assert set(got) == set(ref.online)
    for l in net.noisy_layers:
        for name in (l.wmname, l.bmname, l.wsname, l.bsname):
            assert not np.array_equal(start[name], got[name][0]), name
    for name, arr in ref.online.items():
        err = np.abs(got[name][0].astype(np.float64) - arr)
        bound = WEIGHTS["atol"] + WEIGHTS["rtol"] * np.abs(arr)
        print("  %-60s worst |error| %.3e, worst error / bound %.3f" % (name, err.max(), (err / bound).max()))
    for name, arr in ref.online.items():
        assert not np.array_equal(start[name], got[name][0]), name
        np.testing.assert_allclose(got[name][0], arr, err_msg=name, **WEIGHTS)


# --------------------------------------------------------------------------------------------------- the agent
def _agent(dev, seed=5, noisy=True, n_step=N_STEP, memory=None, kind="vector"):
    from coach_amd.agents.rainbow_agent import (RainbowDQNAgent, RainbowDQNAgentParameters,
                                                    RainbowDQNNetworkParameters)
    from coach_amd.core_types import EnvironmentSteps
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    from coach_amd.exploration_policies.e_greedy import EGreedyParameters
    from coach_amd.memories.memory import MemoryGranularity
    p = RainbowDQNAgentParameters()
    p.seed = seed
    if not noisy:                                        # an EGreedy policy over a plain network
        p.network_wrappers = {"main": RainbowDQNNetworkParameters()}
        p.exploration = EGreedyParameters()
    if memory is not None:
        p.memory = memory
    p.algorithm.atoms, p.algorithm.v_min, p.algorithm.v_max, p.algorithm.n_step = 11, -2.0, 8.0, n_step
    p.network_wrappers["main"].batch_size = 16
    p.memory.max_size = (MemoryGranularity.Transitions, 64)
    p.algorithm.num_consecutive_playing_steps = EnvironmentSteps(1)
    p.algorithm.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(7)
    if kind == "image":
        envp = SyntheticVectorEnvironmentParameters("image", 1, (84, 84), 3, episode_length=5, seed=3)
    else:
        envp = SyntheticVectorEnvironmentParameters("vector", 1, (6,), 3, episode_length=5, seed=3)
    return RainbowDQNAgent(p, SyntheticVectorEnvironment(envp, dev), dev)


def _run(a, heatup=20, steps=10, seed=9):
    import random
    from coach_amd.core_types import RunPhase
    if seed is not None:
        random.seed(seed); np.random.seed(seed)
    a.phase = RunPhase.HEATUP
    for _ in range(heatup):
        a.act()
    a.phase = RunPhase.TRAIN
    for _ in range(steps):
        a.step_and_train()
    a.check_status()


def test_agent_refusals(dev):
    from coach_amd.memories.non_episodic.experience_replay import ExperienceReplayParameters
    with pytest.raises(ValueError, match="frame-dedup ring"):
        _agent(dev, kind="image")
    with pytest.raises(ValueError, match="n_step >= 2"):
        _agent(dev, n_step=1)
    with pytest.raises(ValueError, match="n-step prioritized replay"):
        _agent(dev, memory=ExperienceReplayParameters())
    import importlib
    gm = importlib.import_module("coach_amd.presets.Atari_Rainbow").make(level="breakout", num_envs=1)
    gm.device = dev
    with pytest.raises(ValueError, match="frame-dedup ring"):
        gm.create_graph()


def test_agent_loop_equals_the_host_loop(dev, monkeypatch):
    """n_env = 1, episodes of 5 steps: nothing is stored or trained before the first episode ends; then the replay's
    contents equal the restatement's host loop fed the same transitions, every sampled batch of leaves equals a host
    tree's for the same draws, and the priorities after every update are update_priorities on the kernel's error
    buffer: (error + epsilon) ** alpha, bit for bit."""
    import random
    import torch
    from coach_amd.core_types import RunPhase
    from test_rainbow_ref import _host_tree_sample
    a = _agent(dev)
    mem, net = a.memory, a.networks["main"]
    assert type(mem).__name__ == "NStepPrioritizedExperienceReplay" and net.noisy and not a._step_graph_ok()
    ref = R.EpisodeStore(1, mem.rows, N_STEP, DISCOUNT)
    cap, alpha, eps = mem.power_of_2_size, mem.alpha, mem.epsilon
    pr, draws = R.HostPriorities(cap, alpha, eps), []
    store0, upd0, rand0 = mem.store, mem.update_priorities, random.random

    def store(actions, rewards, overs, next_obs, reset_obs, **kw):
        cur = mem.cur_state.cpu().numpy().copy()
        pr.store(ref.step(cur, actions.cpu().numpy(), rewards.cpu().numpy(), overs.cpu().numpy(),
                          next_obs.cpu().numpy(), kw["dones_host"]))
        return store0(actions, rewards, overs, next_obs, reset_obs, **kw)

    def update_priorities(idx, errors):
        assert errors is a.td_errors
        i, e = idx.cpu().numpy(), errors.cpu().numpy()
        assert np.all(e >= 0) and np.all(np.isfinite(e))
        want, _ = _host_tree_sample(pr.leaves, np.array(draws[-len(i):]), pr.listed, 0.4)
        assert np.array_equal(i, want)
        pr.update(i, e)
        upd0(idx, errors)
        n = min(pr.stored, cap)                           # the leaves written so far
        assert np.array_equal(_bits(mem.sum_tree[cap - 1:cap - 1 + n].cpu().numpy()), _bits(pr.leaves[:n]))
        assert np.array_equal(_bits(mem.max_tree[cap - 1:cap - 1 + n].cpu().numpy()), _bits(pr.priority[:n]))
        assert mem.maximal_priority == pr.max_p

    def rand():
        u = rand0()
        draws.append(u)
        return u
    monkeypatch.setattr(mem, "store", store)
    monkeypatch.setattr(mem, "update_priorities", update_priorities)
    monkeypatch.setattr(random, "random", rand)
    random.seed(9); np.random.seed(9)
    a.phase = RunPhase.TRAIN
    for k in range(4):                                   # an open episode: no transition, no update
        a.step_and_train()
        assert mem.num_transitions() == 0 and mem.staged_transitions() == k + 1 and a.training_iteration == 0
    a.phase = RunPhase.HEATUP
    for _ in range(16):
        a.act()
    assert mem.num_transitions() == 40 and mem.committed_total == 20 and a.training_iteration == 0
    a.phase = RunPhase.TRAIN
    state, pystate = np.random.get_state(), random.getstate()
    for _ in range(4):                                   # acting consumes no host draw (no update falls on these steps'
        a.act()                                          # act() half)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and random.getstate() == pystate
    for _ in range(21):
        a.step_and_train()
    a.check_status()
    assert a.training_iteration == 21 and len(draws) == 21 * 16
    _assert_ring_equals(mem, ref)
    assert mem.num_transitions() == min(cap, 2 * ref.stored)
    q = a._q_act.cpu().numpy()
    assert q.dtype == np.float64 and np.array_equal(a.actions.cpu().numpy(), np.argmax(q, axis=1).astype(np.int32))


def test_importance_weights_have_no_effect(dev, monkeypatch):
    """the head's loss_type is empty: the weights the replay computes are read and never multiplied in"""
    import torch
    a, b = _agent(dev), _agent(dev)
    collate0 = b.memory.collate

    def scaled(drawn, size):
        batch = collate0(drawn, size)
        batch._info["weight"] = batch._info["weight"] * 0.25
        return batch
    monkeypatch.setattr(b.memory, "collate", scaled)
    _run(a)
    _run(b)
    assert a.training_iteration == b.training_iteration == 10
    assert torch.equal(a.networks["main"].params.weights, b.networks["main"].params.weights)
    assert torch.equal(a.memory.sum_tree, b.memory.sum_tree)


def test_checkpoint_round_trip_continues_bit_identically(dev, tmp_path):
    """saved at an episode's end (staged open episodes are not part of a checkpoint); the continuation runs through a
    whole episode, its store and the updates behind it"""
    import torch
    from coach_amd.checkpoint import restore_checkpoint, save_checkpoint
    a = _agent(dev)
    _run(a)
    assert a.memory.staged_transitions() == 0
    save_checkpoint(a, str(tmp_path))
    b = _agent(dev)
    restore_checkpoint(b, str(tmp_path))      # (also puts the host generators, reseeded by b's constructor, back)
    assert torch.equal(a.networks["main"].noise_counters, b.networks["main"].noise_counters)
    outs = []
    for agent in (a, b):
        for _ in range(6):
            agent.act()
            agent.train()
        net, mem = agent.networks["main"], agent.memory
        outs.append([agent._q_act.clone(), net.loss.clone(), net.params.weights.clone(), mem.sum_tree.clone(),
                     mem.max_tree.clone(), mem.obs.clone(), mem.next_obs.clone(), mem.n_step_discounted_rewards.clone(),
                     mem.should_bootstrap_next_state.clone()])
        if agent is a:
            restore_checkpoint(b, str(tmp_path))             # (the host generators go back to the checkpoint's state)
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert a.training_iteration == b.training_iteration == 16 and a.memory.committed_total == b.memory.committed_total == 35


def test_egreedy_over_a_plain_network_trains(dev):
    a = _agent(dev, noisy=False)
    assert not a.networks["main"].noisy
    state = np.random.get_state()
    _run(a, seed=None)
    assert np.isfinite(float(a.networks["main"].loss.item())) and a.training_iteration == 10
    after = np.random.get_state()
    assert not np.array_equal(state[1], after[1]) or state[2] != after[2]          # the policy's host draws
