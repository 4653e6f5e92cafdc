"""The fused TD3 and SAC updates (csrc/ac_fused.hip, csrc/rowchain.hpp) against the fp64-checked oracle (oracle/ac_nets.py)
at the shape edges of their kernels, for both update paths (fused: the short launch chain; otherwise layer by layer).

What the cases reach that tests/test_ac_nets.py does not:
  * a batch that is no multiple of the row block (4 rows for TD3, 8 for SAC): a workgroup owns rows >= B, and every
    operand of mlp_dw_adam_kernel must stay ZERO there (its contract: rows padded to 128, columns to 64, never written
    outside [B][cols]) -- one unguarded store to a padding row or column is a wrong weight gradient and nothing else;
  * B > 128: the second and third 128-row chunk of the weight-gradient launch, with 2 rows and with 1 row in the last;
  * widths that are no multiple of 64 or 16 (padding columns, the pad16 tails of dense_fwd / dense_bwdT, uneven column
    slices), the smallest and the largest widths the shape checks accept, networks of different widths;
  * clip_critic_targets, use_non_zero_discount_for_terminal_states, the soft target update inside the Adam launch and
    the write_grads form of the fused TD3 update (what data-parallel training runs);
  * a NaN in ONE of the twin Q streams: np.minimum keeps it, and so must every minimum on the device.

Every case first asserts that the shape is one the fused path takes (so that the fused=False run is the layer-by-layer
chain at a shape the fused one serves, and the fused=True run did not fall back).  Tolerances are those of
tests/test_ac_nets.py for the same quantities; each test prints its figures (`pytest -s`) before it asserts.  The oracle
runs once per case and is shared by the two paths (the device networks start from the same seeded weights: checked)."""
import numpy as np
import pytest

from oracle import ac_nets as O
from test_ac_nets import _agent, _B, _batch, _check_weights, _t

F32 = np.float32
MIX = 0.005

_REF = {}                  # case -> the oracle's run (initial weights, per-update inputs and results, the oracle networks)


def _same_arrays(a, b):
    return a.keys() == b.keys() and all(len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))
                                        for k in a)


def _cached(key, init, make):
    hit = _REF.get(key)
    if hit is None or not all(_same_arrays(x, y) for x, y in zip(hit["init"], init)):
        hit = _REF[key] = dict(make(), init=init)
    return hit


def _measured(name, value):
    print("MEASURED %s %.4g" % (name, value))


def _weight_err(net, onet):
    w = net.params.named_arrays()
    return max(float(np.abs(w[name][t] - arr).max()) for name, towers in onet.weights().items() for t, arr in towers.items())


def _check_targets(net, onet, atol):
    """the device's target buffer against the oracle's target copy (kernels and biases: what mix_target moves)"""
    w = net.params.named_arrays(buf=net.target)
    for lt, (name, tower, _) in zip(onet.target_layers, onet.layers):
        np.testing.assert_allclose(w[name + "/kernel"][tower], lt.W, rtol=0, atol=atol, err_msg="target %s[%d]" % (name, tower))
        np.testing.assert_allclose(w[name + "/bias"][tower], lt.b, rtol=0, atol=atol, err_msg="target %s[%d]" % (name, tower))


# ------------------------------------------------------------------------------------------------------------ TD3
#             D,  A,  B,   actor (h1, h2), critic (h1, h2)
TD3_SMALLEST = (3, 1, 1, (64, 128), (64, 128))        # the smallest shape td3_check accepts: one row of a 4-row block, A = 1,
#                                                       minimum widths, every column slice exactly 32 columns
TD3_RAGGED = (5, 2, 7, (68, 132), (132, 140))         # a ragged last row block; widths = 4 mod 16 (the pad16 tails of dense_fwd
#                                                       / dense_bwdT); uneven slices 32/32/32/36; D + A no multiple of 4
TD3_PRESET_101 = (17, 6, 101, (400, 300), (400, 300))  # the preset, one row more than test_ac_nets: block 25 owns rows 100..103
TD3_WIDEST = (40, 16, 130, (512, 512), (512, 512))    # A and the widths at their maxima (kMaxWidth); the second 128-row chunk
#                                                       of the weight-gradient launch with 2 live rows
TD3_THREE_CHUNKS = (23, 3, 257, (64, 128), (512, 132))  # three chunks, the last of one row; actor and critic of different widths
TD3_SHAPES = [TD3_SMALLEST, TD3_RAGGED, TD3_PRESET_101, TD3_WIDEST, TD3_THREE_CHUNKS]
CLIP = (-0.5, 0.5)


def _td3_agent(dev, monkeypatch, shape, fused, clip=None, non_zero_terminal=False):
    from coach_amd.agents.td3_agent import TD3Agent, TD3AgentParameters
    monkeypatch.setattr(TD3Agent, "FUSED_UPDATE", fused)
    D, A, B, aw, cw = shape
    p = TD3AgentParameters()
    an, cn = p.network_wrappers["actor"], p.network_wrappers["critic"]
    an.observation_embedder_scheme, an.middleware_scheme = (aw[0],), (aw[1],)
    cn.middleware_scheme = tuple(cw)
    p.algorithm.clip_critic_targets = clip
    p.algorithm.use_non_zero_discount_for_terminal_states = non_zero_terminal
    ag = _agent(dev, TD3Agent, p, D, A, B)
    ag._fused()
    assert ag._fused_td3 is not None, "the fused update does not take this shape"
    assert (ag._fused() is not None) == fused
    return ag


def _td3_reference(ag, shape, clip=None, non_zero_terminal=False):
    """Four updates of the oracle from the agent's initial weights (actor step and target mix every second one), with the
    conditions the options need checked on the oracle's own numbers: clip -- at least 10 % of the rows on each bound in
    every update (a third of the rewards is pushed above 2, a third below -2); non_zero_terminal -- at least one done
    row per batch (row 0 is one)."""
    D, A, B = shape[:3]
    actor, critic = ag.networks["actor"], ag.networks["critic"]
    init = (actor.params.named_arrays(), critic.params.named_arrays())

    def make():
        oa = O.ActorOracle(init[0], 1.0, lr=1e-3)
        oc = O.CriticOracle(init[1], streams=2, lr=1e-3)
        rng = np.random.RandomState(4)
        steps = []
        for it in range(1, 5):
            s, a, r, done, ns = _batch(rng, B, D, A)
            noise = rng.normal(0, 0.2, (B, A))
            k = np.arange(B)
            if clip is not None:
                r[k % 3 == 0] = 2 + np.abs(r[k % 3 == 0])
                r[k % 3 == 1] = -2 - np.abs(r[k % 3 == 1])
            if non_zero_terminal:
                done[0] = True
            batch = (s, a, r, done, ns)
            res = O.td3_update(oa, oc, batch, noise, it, ag.low, ag.high, clip=clip, non_zero_terminal=non_zero_terminal)
            assert np.isfinite(res["targets"]).all() and np.isfinite(res["loss"])
            if clip is not None:
                assert (res["targets"] == F32(clip[0])).mean() >= 0.1 and (res["targets"] == F32(clip[1])).mean() >= 0.1
            if non_zero_terminal:
                assert done.sum() >= 1
            if it % 2 == 0:
                oa.mix_target(MIX); oc.mix_target(MIX)
            steps.append((batch, noise, res))
        return dict(oa=oa, oc=oc, steps=steps)
    return _cached(("td3", shape, clip, non_zero_terminal), init, make)


def _adam_slots(net):
    return [net.params.weights, net.target, net.adam.m, net.adam.v, net.adam.state]


def _td3_run(dev, ag, shape, ref, form="adam"):
    """form "adam": the loop of test_td3_update_matches_oracle (the soft target update as its own call);
    "mix": the soft target update applied inside the networks' Adam passes (mix= of _critic_device / _actor_device);
    "write_grads": the fused launches leave the gradients in the networks' grads buffers and the flat Adam launch applies
    them (+ the target mix), as data-parallel training runs it (td3_agent.py, `wg`)."""
    import torch
    actor, critic = ag.networks["actor"], ag.networks["critic"]
    tag = "%s %s fused=%s" % (shape, form, ag._fused() is not None)
    for it, (batch, noise, r) in enumerate(ref["steps"], 1):
        db = _B(dev, batch)
        ag.noise.copy_(_t(noise, dev))
        even = it % 2 == 0
        mix = MIX if even else None
        if form == "write_grads":
            fused = ag._fused()
            for net, update, kw in ((critic, fused.critic_update, {"with_norm": True}), (actor, fused.actor_update, {})):
                if net is actor and not even:
                    continue
                before = [x.clone() for x in _adam_slots(net)]
                update(db, mix, write_grads=True)
                # the gradients went to net.params.grads: weights, target and the Adam slots are untouched until the step
                assert all(torch.equal(x, y) for x, y in zip(before, _adam_slots(net)))
                net.apply_gradients(ag._grad_scale("critic" if net is critic else "actor"), mix_rate=mix, **kw)
        elif form == "mix":
            ag._critic_device(db, mix=mix)
            if even:
                ag._actor_device(db, mix=mix)
        else:
            ag._critic_device(db)
            if even:
                ag._actor_device(db)
                ag.update_target_networks(MIX)
        got, loss = ag.td_targets.cpu().numpy(), float(critic.loss[:2].sum())
        _measured("td3 targets abs err [%s it %d]" % (tag, it), np.abs(got - r["targets"]).max())
        _measured("td3 loss rel err [%s it %d]" % (tag, it), abs(loss - r["loss"]) / abs(r["loss"]))
        np.testing.assert_allclose(got, r["targets"], rtol=2e-4, atol=1e-5)
        np.testing.assert_allclose(loss, r["loss"], rtol=2e-4)
    _measured("td3 actor weights abs err [%s]" % tag, _weight_err(actor, ref["oa"]))
    _measured("td3 critic weights abs err [%s]" % tag, _weight_err(critic, ref["oc"]))
    _check_weights(actor, ref["oa"])
    _check_weights(critic, ref["oc"])
    _check_targets(actor, ref["oa"], 2e-5)
    _check_targets(critic, ref["oc"], 2e-5)
    ag.check_status()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("shape", TD3_SHAPES)
def test_td3_update_matches_oracle_at_shape_edges(dev, shape, fused, monkeypatch):
    ag = _td3_agent(dev, monkeypatch, shape, fused)
    _td3_run(dev, ag, shape, _td3_reference(ag, shape))


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("option", ["clip", "non_zero_terminal"])
@pytest.mark.parametrize("shape", [TD3_RAGGED, TD3_PRESET_101])
def test_td3_target_options_match_oracle(dev, shape, option, fused, monkeypatch):
    """clip_critic_targets = (-0.5, 0.5) with at least a tenth of the rows on each bound, and
    use_non_zero_discount_for_terminal_states with done rows in every batch (conditions: _td3_reference)."""
    kw = dict(clip=CLIP) if option == "clip" else dict(non_zero_terminal=True)
    ag = _td3_agent(dev, monkeypatch, shape, fused, **kw)
    _td3_run(dev, ag, shape, _td3_reference(ag, shape, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("shape", [TD3_RAGGED, TD3_PRESET_101])
def test_td3_soft_target_update_inside_the_adam_pass(dev, shape, fused, monkeypatch):
    """mix_rate of the Adam launch (mlp_dw_adam_kernel's `mix`; the flat Adam launch on the layer-by-layer path): the
    oracle still mixes after the update, and the device's target buffers must equal its target copy."""
    ag = _td3_agent(dev, monkeypatch, shape, fused)
    _td3_run(dev, ag, shape, _td3_reference(ag, shape), form="mix")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [TD3_RAGGED, TD3_PRESET_101])
def test_td3_fused_write_grads_form(dev, shape, monkeypatch):
    """The write_grads form exists on the fused path alone (the layer-by-layer chain always leaves its gradients in
    grads): same assertions as the Adam-in-launch form, and nothing but grads moves before apply_gradients."""
    ag = _td3_agent(dev, monkeypatch, shape, True)
    _td3_run(dev, ag, shape, _td3_reference(ag, shape), form="write_grads")


@pytest.mark.gpu
@pytest.mark.parametrize("fused,paired", [(False, False), (False, True), (True, False)])
def test_td3_min_keeps_a_nan_of_one_stream(dev, fused, paired, monkeypatch):
    """A NaN in the head bias of the TARGET critic's stream 0 alone: Q_target_1 is NaN in every row, Q_target_2 is finite.
    np.minimum keeps the NaN, so q_min, the TD targets and the critic loss are NaN in the oracle; `a <= b ? a : b`
    returned the finite stream and the update went on as if nothing had happened.  paired: the layer-by-layer path whose
    minimum is taken inside rlx_ac_critic_losses."""
    shape = TD3_RAGGED
    D, A, B = shape[:3]
    ag = _td3_agent(dev, monkeypatch, shape, fused)
    actor, critic = ag.networks["actor"], ag.networks["critic"]
    oa = O.ActorOracle(actor.params.named_arrays(), 1.0, lr=1e-3)
    oc = O.CriticOracle(critic.params.named_arrays(), streams=2, lr=1e-3)
    head0 = next(i for i, (_, _, l) in enumerate(oc.layers) if l is oc.heads[0])
    oc.target_layers[head0].b[0] = np.nan
    critic.params.w("critic/v_head/output/bias", 0, buf=critic.target)[0] = float("nan")
    rng = np.random.RandomState(4)
    batch = _batch(rng, B, D, A)
    noise = rng.normal(0, 0.2, (B, A))
    with np.errstate(invalid="ignore"):
        q_next = oc.forward(batch[4], oa.forward(batch[4], target=True), target=True)
        assert np.isnan(q_next[0]).all() and np.isfinite(q_next[1]).all()
        r = O.td3_update(oa, oc, batch, noise, 1, ag.low, ag.high)
    assert np.isnan(r["q_min"]).all() and np.isnan(r["targets"]).all() and np.isnan(r["loss"])
    ag.noise.copy_(_t(noise, dev))
    ag._critic_device(_B(dev, batch, paired))
    assert np.isnan(ag.q_min.cpu().numpy()).all()
    assert np.isnan(ag.td_targets.cpu().numpy()).all()
    assert np.isnan(float(critic.loss[:2].sum()))


# ------------------------------------------------------------------------------------------------------------ SAC
#             D,  A,  B,   policy (h1, h2), V (h1, h2), q_hidden
SAC_SMALLEST = (3, 1, 1, (128, 128), (128, 128), 128)      # the smallest accepted shape; one row of an 8-row block
SAC_RAGGED = (11, 3, 130, (132, 140), (140, 132), 192)     # a ragged 8-row block; the second dW chunk with 2 rows; widths no
#                                                            multiple of 64 or 16; policy and V widths that differ and sit BELOW q_hidden
SAC_WIDE_POLICY = (23, 5, 37, (384, 384), (256, 256), 128)  # policy and V widths ABOVE pad64(q_hidden)
SAC_WIDE_V1 = (23, 5, 37, (128, 128), (192, 128), 128)     # v_mlp.h1 > q_hidden alone (h1VT, the target V's first layer)
SAC_SHAPES = [SAC_SMALLEST, SAC_RAGGED, SAC_WIDE_POLICY, SAC_WIDE_V1]


def _sac_agent(dev, monkeypatch, shape, fused):
    from coach_amd.agents.soft_actor_critic_agent import SoftActorCriticAgent, SoftActorCriticAgentParameters
    monkeypatch.setattr(SoftActorCriticAgent, "FUSED_UPDATE", fused)
    D, A, B, pw, vw, H = shape
    p = SoftActorCriticAgentParameters()
    p.algorithm.resample_noise_per_pass = True
    pn, qn, vn = (p.network_wrappers[k] for k in ("policy", "q", "v"))
    pn.embedder_scheme, pn.middleware_scheme = (pw[0],), (pw[1],)
    vn.embedder_scheme, vn.middleware_scheme = (vw[0],), (vw[1],)
    qn.network_layers_sizes = (H, H)
    ag = _agent(dev, SoftActorCriticAgent, p, D, A, B)
    ag._fused()
    assert ag._fused_sac is not None, "the fused update does not take this shape"
    assert (ag._fused() is not None) == fused
    return ag


def _sac_reference(ag, shape):
    D, A, B = shape[:3]
    init = tuple(ag.networks[k].params.named_arrays() for k in ("policy", "q", "v"))

    def make():
        op, oq, ov = O.SACPolicyOracle(init[0]), O.SACQOracle(init[1]), O.SACValueOracle(init[2])
        rng = np.random.RandomState(5)
        steps = []
        for it in range(4):
            batch = _batch(rng, B, D, A)
            z = rng.standard_normal((3, B, A))
            res = O.sac_update(op, oq, ov, batch, z, resample=True)
            assert np.isfinite(res["value_targets"]).all() and np.isfinite(res["loss"]) and np.isfinite(res["v_loss"])
            ov.mix_target(MIX)
            steps.append((batch, z, res))
        return dict(op=op, oq=oq, ov=ov, steps=steps)
    return _cached(("sac", shape), init, make)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("shape", SAC_SHAPES)
def test_sac_update_matches_oracle_at_shape_edges(dev, shape, fused, monkeypatch):
    """The assertions of test_sac_update_matches_oracle.  SAC_WIDE_POLICY / SAC_WIDE_V1: rlx_sac_fused_supported accepts
    the five widths independently, so every workspace buffer that holds a policy / V layer has to have that layer's
    padded width.  With all of them sized and strided by pad64(q_hidden) (128 here) a 384-wide row of h1P / h2P / dz2P /
    dh1Pp ran 256 floats into the next two rows (rows written by other workgroups of the same launch, in no order) and
    the padding columns the weight-gradient launch relies on were no padding at all; h1VT [B][q_hidden] took rows of
    v_mlp.h1 = 192 floats at stride 192 and its last rows ran into zP.  All of it inside the workspace: no fault, wrong
    V_target(s'), wrong policy / V gradients."""
    ag = _sac_agent(dev, monkeypatch, shape, fused)
    ref = _sac_reference(ag, shape)
    pol, qn, vn = ag.networks["policy"], ag.networks["q"], ag.networks["v"]
    tag = "%s fused=%s" % (shape, fused)
    for it, (batch, z, r) in enumerate(ref["steps"]):
        ag.normals.copy_(_t(z, dev))
        ag._learn_device(_B(dev, batch))
        np.testing.assert_allclose(ag.dq_da.cpu().numpy(), r["dq_da"], rtol=2e-3, atol=1e-7)
        # the log-probability's conditioning: d log(1 - t^2 + eps) = 2 |t| dt / (1 - t^2 + eps), dt = 2 ulp of tanh
        t = r["actions"].astype(np.float64)
        cond = (2 * np.abs(t) * 2.4e-7 / (1 - t * t + 1e-6)).sum(axis=1)
        vt = ag.value_targets.cpu().numpy()
        _measured("sac value targets err over bound [%s it %d]" % (tag, it),
                  (np.abs(vt - r["value_targets"]) / (2e-4 * np.abs(r["value_targets"]) + 2e-5 + cond)).max())
        assert np.all(np.abs(vt - r["value_targets"]) <= 2e-4 * np.abs(r["value_targets"]) + 2e-5 + cond), \
            np.abs(vt - r["value_targets"]).max()
        td = ag.td_targets.cpu().numpy()
        _measured("sac td targets abs err [%s it %d]" % (tag, it), np.abs(td - r["td_targets"]).max())
        _measured("sac q loss rel err [%s it %d]" % (tag, it), abs(float(qn.loss[:2].sum()) - r["loss"]) / abs(r["loss"]))
        _measured("sac v loss rel err [%s it %d]" % (tag, it), abs(float(vn.loss) - r["v_loss"]) / abs(r["v_loss"]))
        np.testing.assert_allclose(td, r["td_targets"], rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose(float(qn.loss[:2].sum()), r["loss"], rtol=3e-4)
        assert float(qn.loss[2]) == float(qn.loss[0] + qn.loss[1])
        np.testing.assert_allclose(float(vn.loss), r["v_loss"], rtol=3e-4)
        ag.update_target_networks(MIX)
    for name, net, onet in (("policy", pol, ref["op"]), ("q", qn, ref["oq"]), ("v", vn, ref["ov"])):
        _measured("sac %s weights abs err [%s]" % (name, tag), _weight_err(net, onet))
    _check_weights(pol, ref["op"], atol=5e-5)
    _check_weights(qn, ref["oq"], atol=5e-5)
    _check_weights(vn, ref["ov"], atol=5e-5)
    _check_targets(vn, ref["ov"], 5e-5)
    ag.check_status()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
def test_sac_min_keeps_a_nan_of_one_tower(dev, fused, monkeypatch):
    """A NaN in the q_output bias of Q tower 0 alone: Q_1(s, a ~ pi) is NaN in every row, Q_2 finite; np.minimum keeps
    the NaN, so the V targets (min - log pi) are NaN in every row.  The gradient of the minimum goes to the side the
    value came from (tower 0: its hidden layers are finite), so dQ/da is finite and comparable."""
    shape = SAC_RAGGED
    D, A, B = shape[:3]
    ag = _sac_agent(dev, monkeypatch, shape, fused)
    pol, qn, vn = ag.networks["policy"], ag.networks["q"], ag.networks["v"]
    qn.params.w("q/q_head/q_output/bias", 0)[0] = float("nan")
    op, oq, ov = O.SACPolicyOracle(pol.params.named_arrays()), O.SACQOracle(qn.params.named_arrays()), \
        O.SACValueOracle(vn.params.named_arrays())
    rng = np.random.RandomState(5)
    batch = _batch(rng, B, D, A)
    z = rng.standard_normal((3, B, A))
    with np.errstate(invalid="ignore"):
        qv = oq.forward(batch[0], op.forward(batch[0], z[0])["actions"])
        assert np.isnan(qv[0]).all() and np.isfinite(qv[1]).all()
        r = O.sac_update(op, oq, ov, batch, z, resample=True)
    assert np.isnan(r["value_targets"]).all() and np.isfinite(r["dq_da"]).all()
    ag.normals.copy_(_t(z, dev))
    ag._learn_device(_B(dev, batch))
    assert np.isnan(ag.value_targets.cpu().numpy()).all()
    np.testing.assert_allclose(ag.dq_da.cpu().numpy(), r["dq_da"], rtol=2e-3, atol=1e-7)
