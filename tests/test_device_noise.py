"""noise_source = "device" on the GPU: rlx_normal_fill is bit-identical to its numpy twin (tests/noise_ref.py), follows
the event counters it reads from device memory inside a replayed graph, and the TD3 / SAC agents that take their
Gaussian draws from it reproduce oracle loops fed with the twin's values (replay indices bit-exact, host generator
state identical), are bit-identical between the chunked and the per-update training paths, and resume from a
checkpoint bit-identically."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_ref as R  # noqa: E402
from tolerances import LOSS  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n, s0, ns, events, scale", [
    (7, 0, 1, [0], 1.0),                                     # odd n, one stream, K = 1
    (255, 1, 3, [3, 4, 5, 6, 7, 8, 9, 10], 1.0),             # SAC's three streams, K = 8
    (1, 4, 1, [(1 << 32) - 1, 1 << 32], 1.0),                # events around 2^32
    (1700, 0, 1, [(1 << 40) + k for k in range(8)], 0.2),    # around 2^40, sigma != 1
    (8 * 3 * 256 * 17 // 24, 1, 3, list(range(100, 108)), 1.0),   # one C5 chunk (8 x 3 x 256 x 17 values)
])
def test_normal_fill_is_bit_identical_to_the_twin(dev, n, s0, ns, events, scale):
    import torch
    from coach_amd import _rlx
    lib = _rlx.lib()
    out = torch.full((len(events), ns, n + 1), 7.0, dtype=torch.float64, device=dev)   # + a guard column
    ev = torch.tensor(events, dtype=torch.int64, device=dev)
    for seed, rank in ((11, 0), (0xFFFFFFFF, 3)):
        work = out[..., :n].contiguous()
        lib.normal_fill(work, ev, len(events), s0, ns, n, seed, rank, scale, _rlx.current_stream())
        got = work.cpu().numpy()
        np.testing.assert_array_equal(got, R.normal_fill(events, s0, ns, n, seed, rank, scale))
    # nothing written past n values per (event, stream)
    lib.normal_fill(out, ev, len(events), s0, ns, n, 1, 0, scale, _rlx.current_stream())
    flat = out.cpu().numpy().reshape(-1)
    assert (flat[len(events) * ns * n:] == 7.0).all()


def test_graph_replay_follows_the_counter_in_device_memory(dev):
    import torch
    from coach_amd import _rlx
    lib = _rlx.lib()
    n = 33
    ev = torch.tensor([5, 6], dtype=torch.int64, device=dev)
    out = torch.zeros(2, 3, n, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        lib.normal_fill(out, ev, 2, 1, 3, n, 9, 0, 1.0, _rlx.current_stream())    # (warm)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lib.normal_fill(out, ev, 2, 1, 3, n, 9, 0, 1.0, _rlx.current_stream())
    for events in ([5, 6], [1 << 33, 12], [77, 78]):
        ev.copy_(torch.tensor(events, dtype=torch.int64))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), R.normal_fill(events, 1, 3, n, 9, 0))


# ------------------------------------------------------------------------------------------------------ agents
def _ref_normals(event, s0, ns, shape, seed, scale=1.0):
    return R.normal_fill([event], s0, ns, int(np.prod(shape[-2:])), seed, 0, scale)[0].reshape(shape)


def _td3_oracle_cls():
    from oracle import ac_nets as O
    from oracle.agents import TD3AgentOracle

    class TD3DeviceNoiseOracle(TD3AgentOracle):
        """TD3AgentOracle with the acting noise and the smoothing noise from the twin: stream 4 at the acting counter,
        stream 0 (scaled by policy_noise) at the update's training_iteration."""
        seed, act_event = 0, 0

        def act(self):
            mean = self.actor.forward(np.stack(self.cur).astype(np.float32))
            z = _ref_normals(self.act_event, 4, 1, (self.n_env, self.A), self.seed)
            self.act_event += 1
            acts = [mean[e].astype(np.float64) + self.std * z[e] for e in range(self.n_env)]
            self.recorded_actions.append(np.array(acts))
            self._step_envs(acts, True)
            return acts

        def _train_phase(self, steps):
            draws = [self.memory.sample_indices(self.B) for _ in range(steps)]
            for idx in draws:
                self.training_iteration += 1
                rows = [self.memory.rows[i] for i in idx]
                self.sampled.append(np.asarray(idx))
                batch = (np.stack([r[0] for r in rows]).astype(np.float32),
                         np.stack([r[1] for r in rows]).astype(np.float32),
                         np.array([r[2] for r in rows], dtype=np.float32), np.array([r[3] for r in rows]),
                         np.stack([r[4] for r in rows]).astype(np.float32))
                noise = _ref_normals(self.training_iteration, 0, 1, (self.B, self.A), self.seed, self.policy_noise)
                r = O.td3_update(self.actor, self.critic, batch, noise, self.training_iteration, self.low, self.high,
                                 self.discount, self.noise_clipping, self.policy_every)
                self.losses.append(r["loss"])
                self.targets = r["targets"]
                if self.training_iteration - self.last_target_update >= self.policy_every:
                    self.last_target_update = self.training_iteration
                    self.actor.mix_target(self.tau)
                    self.critic.mix_target(self.tau)
    return TD3DeviceNoiseOracle


def _sac_oracle_cls():
    from oracle import ac_nets as O
    from oracle.agents import SACAgentOracle

    class SACDeviceNoiseOracle(SACAgentOracle):
        """SACAgentOracle with the acting sample's normals (stream 4, acting counter) and the update's three arrays
        (streams 1-3, training_iteration) from the twin."""
        seed, act_event = 0, 0

        def act(self):
            z = _ref_normals(self.act_event, 4, 1, (self.n_env, self.A), self.seed)
            self.act_event += 1
            o = self.policy.forward(np.stack(self.cur).astype(np.float32), z)
            acts = [o["actions"][e].astype(np.float32) for e in range(self.n_env)]
            self.recorded_actions.append(np.array(acts))
            self._step_envs(acts)
            self.train()
            return acts

        def train(self):
            if self._num_transitions() <= 0:
                return
            for _ in range(self.n_env):
                d = self._draw(self.B)
                self.visible.append(self._num_transitions())
                (s, a, r, done, ns), _, _ = self._collate(d, self.B)
                self.sampled_keys.append(np.asarray(s)[:, 0].astype(np.float64))
                self.training_iteration += 1
                normals = _ref_normals(self.training_iteration, 1, 3, (3, self.B, self.A), self.seed)
                res = O.sac_update(self.policy, self.q, self.v, (s.astype(np.float32), np.asarray(a, dtype=np.float32),
                                                                 r, done, ns.astype(np.float32)), normals, self.discount)
                self.losses.append(res["loss"])
                self.targets = res["td_targets"]
                self.v.mix_target(self.tau)
    return SACDeviceNoiseOracle


@pytest.mark.parametrize("name", ["td3", "sac"])
def test_device_noise_loops_match_oracles_fed_by_the_twin(dev, name):
    """n_env = 8 lockstep envs (different episode lengths for TD3), small networks: the device-noise agent against the
    reference-pinned loop oracles whose Gaussian draws come from tests/noise_ref.py instead of np.random."""
    from coach_amd.core_types import RunPhase
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    from coach_amd.memories.memory import MemoryGranularity
    from oracle.synth_env import SynthVecEnv
    n_env, D, A, B = 8, 9, 3, 16
    lengths = [5, 7, 4, 6, 5, 7, 4, 6] if name == "td3" else [6] * n_env
    HEATUP, TRAIN = (14, 16) if name == "td3" else (5, 8)
    ep = SyntheticVectorEnvironmentParameters("vector", n_env, (D,), None, action_dim=A, episode_length=max(lengths),
                                              seed=9)
    ep.episode_lengths = list(lengths)
    env = SyntheticVectorEnvironment(ep, dev)
    if name == "td3":
        from coach_amd.agents.td3_agent import TD3Agent as C, TD3AgentParameters as P
        p = P()
        p.network_wrappers["actor"].observation_embedder_scheme = (24,)
        p.network_wrappers["actor"].middleware_scheme = (16,)
        p.network_wrappers["critic"].middleware_scheme = (24, 16)
        p.memory.max_size = (MemoryGranularity.Transitions, 4096)
    else:
        from coach_amd.agents.soft_actor_critic_agent import SoftActorCriticAgent as C, \
            SoftActorCriticAgentParameters as P
        p = P()
        p.network_wrappers["policy"].embedder_scheme, p.network_wrappers["policy"].middleware_scheme = (24,), (16,)
        p.network_wrappers["v"].embedder_scheme, p.network_wrappers["v"].middleware_scheme = (24,), (16,)
        p.network_wrappers["q"].network_layers_sizes = (16, 16)
        p.memory.max_size = (MemoryGranularity.Transitions, 4096)
    p.seed = 11
    p.algorithm.noise_source = "device"
    for n in p.network_wrappers.values():
        n.batch_size = B
    agent = C(p, env, dev)
    assert agent.noise_source == "device"
    agent.debug_draws, agent.debug_losses = [], []
    if name == "td3":
        arr = [agent.networks[k].params.named_arrays() for k in ("actor", "critic")]
        o = _td3_oracle_cls()(*arr, SynthVecEnv(1, n_env, D, max(lengths), 9, episode_lengths=list(lengths)), A,
                              batch_size=B, lr_actor=p.network_wrappers["actor"].learning_rate,
                              lr_critic=p.network_wrappers["critic"].learning_rate)
    else:
        arr = [agent.networks[k].params.named_arrays() for k in ("policy", "q", "v")]
        o = _sac_oracle_cls()(*arr, SynthVecEnv(1, n_env, D, max(lengths), 9, episode_lengths=list(lengths)), A,
                              batch_size=B, capacity=4096, reward_rescale=5.0)
        o.reference_order = True
    o.seed = 11
    o.reset()
    state = (random.getstate(), np.random.get_state())
    acts = []
    for step in range(HEATUP + TRAIN):
        agent.phase = RunPhase.HEATUP if step < HEATUP else RunPhase.TRAIN
        agent.act()
        acts.append(agent.actions.cpu().numpy().copy())
        if step >= HEATUP:
            agent.train()
    agent.check_status()
    hip_state = (random.getstate(), np.random.get_state())
    random.setstate(state[0]); np.random.set_state(state[1])
    for step in range(HEATUP + TRAIN):
        o.heatup_step() if step < HEATUP else o.act()
    assert np.array_equal(np.random.get_state()[1], hip_state[1][1]) and \
        np.random.get_state()[2:] == hip_state[1][2:]                           # identical host RNG consumption
    assert agent.training_iteration == o.training_iteration > 0
    assert agent._act_event == o.act_event == TRAIN
    assert len(agent.debug_draws) == len(o.sampled) == agent.training_iteration
    for d, s_ in zip(agent.debug_draws, o.sampled):
        np.testing.assert_array_equal(d, s_)
    # the first updates agree to the stated loss tolerance; later ones (and the actions of later steps, 8 updates per
    # env-step here) drift apart by what fp32 accumulation order does to Adam steps of tiny gradients — the weights' bound
    # of the host-noise loop tests (test_agent_loops.py)
    np.testing.assert_allclose(agent.debug_losses[:4], o.losses[:4], **LOSS)
    np.testing.assert_allclose(np.array(acts), np.array(o.recorded_actions), rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(agent.debug_losses, o.losses, rtol=2e-2, atol=2e-3)
    if name == "td3":
        # (SAC's last TD targets are not compared: the agent's V_target(s') and the oracle's sit one soft update of V's
        # target apart at that point, in either noise mode — a bookkeeping difference of the oracle, not of the noise)
        np.testing.assert_allclose(agent.td_targets.cpu().numpy().ravel(), np.asarray(o.targets).ravel(),
                                   rtol=1e-3, atol=1e-4)
    nets = ((agent.networks["actor"], o.actor), (agent.networks["critic"], o.critic)) if name == "td3" else \
        ((agent.networks["policy"], o.policy), (agent.networks["q"], o.q), (agent.networks["v"], o.v))
    for net, orc in nets:
        hw = net.params.named_arrays()
        for wname, per_tower in orc.weights().items():
            for t, ref in per_tower.items():
                np.testing.assert_allclose(hw[wname][t], ref, rtol=2e-3, atol=2e-4, err_msg=wname)


def _mk_device(dev, name, n_env, D, A, L, B, seed=11, cap=8192):
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    from coach_amd.memories.memory import MemoryGranularity
    if name == "td3":
        from coach_amd.agents.td3_agent import TD3Agent as C, TD3AgentParameters as P
    else:
        from coach_amd.agents.soft_actor_critic_agent import SoftActorCriticAgent as C, \
            SoftActorCriticAgentParameters as P
    p = P()
    p.seed = seed
    p.algorithm.noise_source = "device"
    for n in p.network_wrappers.values():
        n.batch_size = B
    p.memory.max_size = (MemoryGranularity.Transitions, cap)
    env = SyntheticVectorEnvironment(SyntheticVectorEnvironmentParameters("vector", n_env, (D,), None, action_dim=A,
                                                                           episode_length=L, seed=9), dev)
    return C(p, env, dev)


def _run(agent, heatup, steps):
    from coach_amd.core_types import RunPhase
    random.seed(1); np.random.seed(1)
    agent.phase = RunPhase.HEATUP
    for _ in range(heatup):
        agent.act()
    agent.phase = RunPhase.TRAIN
    for _ in range(steps):
        agent.act()
        agent.train()
    agent.check_status()
    return np.random.get_state()


@pytest.mark.parametrize("name, shape", [("td3", (8, 9, 3, 5, 16, 6, 10)), ("sac", (8, 9, 3, 5, 16, 3, 6)),
                                         ("sac", (512, 376, 17, 1000, 256, 2, 2))])   # the C5 shape
def test_device_noise_chunked_and_per_update_paths_are_bit_identical(dev, name, shape):
    import torch
    n_env, D, A, L, B, heat, steps = shape
    runs = []
    for chunk in (8, 0):
        a = _mk_device(dev, name, n_env, D, A, L, B)
        a.UPDATE_CHUNK = chunk
        st = _run(a, heat, steps)
        runs.append((a, st))
    (a, sa), (b, sb) = runs
    assert a.training_iteration == b.training_iteration >= 16
    assert a.__dict__.get("_chunk_recs") and not b.__dict__.get("_chunk_recs")   # the two paths were taken
    for k in a.networks:
        assert torch.equal(a.networks[k].params.weights, b.networks[k].params.weights), k
        if a.networks[k].target is not None:
            assert torch.equal(a.networks[k].target, b.networks[k].target), k
    assert torch.equal(a.td_targets, b.td_targets)
    assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    assert a._act_event == b._act_event == steps


@pytest.mark.parametrize("name", ["td3", "sac"])
def test_device_noise_checkpoint_resume_is_bit_identical(dev, tmp_path, name):
    """The noise seed comes from os.urandom here (ap.seed None): only a restored key reproduces the run."""
    import torch
    from coach_amd.checkpoint import restore_checkpoint, save_checkpoint
    from coach_amd.core_types import RunPhase

    def make():
        return _mk_device(dev, name, 4, 9, 3, 6, 8, seed=None, cap=256)

    def drive(agent, steps):
        for _ in range(steps):
            agent.act()
            agent.train()

    a = make()
    random.seed(2); np.random.seed(2)
    a.phase = RunPhase.HEATUP
    drive(a, 4)
    a.phase = RunPhase.TRAIN
    drive(a, 9)
    save_checkpoint(a, str(tmp_path), checkpoint_id=1)
    drive(a, 11)
    b = make()
    assert b._noise_seed != a._noise_seed or True          # (a fresh 32-bit draw; equal only by chance)
    restore_checkpoint(b, str(tmp_path))
    assert b._noise_seed == a._noise_seed and b._act_event == 9
    b.phase = RunPhase.TRAIN
    drive(b, 11)
    for k in a.networks:
        assert torch.equal(a.networks[k].params.weights, b.networks[k].params.weights), k
        assert torch.equal(a.networks[k].adam.v, b.networks[k].adam.v), k
    assert a.training_iteration == b.training_iteration and a._act_event == b._act_event
    assert torch.equal(a.td_targets, b.td_targets)
