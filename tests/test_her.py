"""BitFlip on the device and Hindsight Experience Replay on the MI355X: rlx_bitflip_* and rlx_her_relabel_episode against
their numpy restatements (tests/bit_flip_ref.py, tests/her_ref.py) bit for bit, the hindsight memory with three envs
finishing on different steps and with one env on the reference's own cases (tests/golden/her.npz), the refusals, the
episode-counted training cadence of the BitFlip presets, and the reference's two golden bars."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import bit_flip_ref as BR
import her_ref as HR
from coach_amd.memories.episodic.episodic_hindsight_experience_replay import (
    EpisodicHindsightExperienceReplay, EpisodicHindsightExperienceReplayParameters, HindsightGoalSelectionMethod)
from coach_amd.memories.memory import MemoryGranularity
from coach_amd.spaces import GoalsSpace, InverseDistanceFromGoal, ReachingGoal

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------- rlx_bitflip_*
def _make_env(dev, n_env, L, max_steps, mean_zero, seed):
    from coach_amd.environments.bit_flip_vector_environment import (BitFlipVectorEnvironment,
                                                                    BitFlipVectorEnvironmentParameters)
    return BitFlipVectorEnvironment(BitFlipVectorEnvironmentParameters(n_env, L, max_steps, mean_zero, seed), dev)


def _solving_or_stalling_actions(ref):
    """even (env + episode): flip the first bit that differs (reaches the goal); odd: flip bit 0 for ever (times out)."""
    L, acts = ref.L, []
    for e in range(ref.n):
        diff = np.nonzero(ref.bits[e, :L] != ref.bits[e, L:])[0]
        acts.append(int(diff[0]) if (e + int(ref.episode[e])) % 2 == 0 and diff.size else 0)
    return np.array(acts, dtype=np.int32)


@pytest.mark.parametrize("mean_zero", [False, True])
@pytest.mark.parametrize("n_env", [1, 5])
@pytest.mark.parametrize("L", [1, 8, 20, 33])
def test_bitflip_kernels_equal_the_numpy_twin(dev, L, n_env, mean_zero):
    max_steps = L + 2 if mean_zero else None                  # a custom limit / the default (bit_length)
    env = _make_env(dev, n_env, L, max_steps, mean_zero, seed=77)
    ref = BR.VectorBitFlip(n_env, L, max_steps, mean_zero, seed=77)
    assert np.array_equal(env.reset_internal_state().cpu().numpy(), ref.reset())       # episode 0's draws
    reached = timed_out = 0
    for step in range(3 * L + 2):
        if step == L + 1:                                     # a forced reset: every env starts its NEXT episode
            assert np.array_equal(env.reset_internal_state().cpu().numpy(), ref.reset(next_episode=True))
        a = _solving_or_stalling_actions(ref)
        r_next, r_reset, r_rew, r_done = ref.step(a)
        nxt, rst, rew, done = env.step(torch.from_numpy(a).to(dev))
        assert np.array_equal(nxt.cpu().numpy(), r_next), step
        assert np.array_equal(rst.cpu().numpy(), r_reset), step
        assert np.array_equal(rew.cpu().numpy(), r_rew) and np.array_equal(done.cpu().numpy(), r_done), step
        assert np.array_equal(env.episode.cpu().numpy(), ref.episode), step
        assert np.array_equal(env.step_in_episode.cpu().numpy(), ref.steps), step
        assert np.array_equal(env.bits.cpu().numpy(), ref.bits) and np.array_equal(env.dones_host, r_done != 0)
        reached += int(((r_done != 0) & (r_rew == 0)).sum())
        timed_out += int(((r_done != 0) & (r_rew != 0)).sum())
    assert reached > 0 and (timed_out > 0 or L == 1)          # at L = 1 every flip reaches the goal
    env.check_status()


def test_bitflip_forced_goal_redraw_equals_the_twin(dev):
    """an (env, episode 0) whose first goal draw equals its state, found on the CPU: the device redraws like the twin"""
    for L in (1, 2):
        seed, e, ep = BR.find_forced_redraw(L, 5, episodes=(0,))
        assert BR.draw_episode(seed, e, ep, L)[2] >= 1
        env = _make_env(dev, 5, L, None, False, seed)
        ref = BR.VectorBitFlip(5, L, None, False, seed)
        obs, expect = env.reset_internal_state().cpu().numpy(), ref.reset()
        assert np.array_equal(obs, expect) and not np.array_equal(obs[e, :L], obs[e, L:])


def test_bitflip_out_of_range_action_sets_the_status_bit_and_flips_nothing(dev):
    env = _make_env(dev, 3, 8, None, False, seed=5)
    env.reset_internal_state()
    before = env.bits.cpu().numpy().copy()
    env.step(torch.tensor([8, -1, 1 << 30], dtype=torch.int32, device=dev))
    assert np.array_equal(env.bits.cpu().numpy(), before) and int(env.status.item()) == 2
    assert env.step_in_episode.cpu().tolist() == [1, 1, 1]
    with pytest.raises(RuntimeError, match="outside"):
        env.check_status()


def test_bitflip_parameters_refuse_no_limit_and_carry_the_slice_table(dev):
    from coach_amd.environments import gym_environment as G
    p = G.GymVectorEnvironment(level=G.BIT_FLIP_LEVEL)
    p.additional_simulator_parameters = {"bit_length": 6, "mean_zero": True}
    env = G.create(p, dev)
    assert env.p.observation_slices == {"desired_goal": (0, 6), "state": (6, 12)} and env.p.episode_length == 6
    assert env.p.num_actions == 6 and env.p.observation_shape == (12,) and env.p.mean_zero
    p.additional_simulator_parameters = {"bit_length": 6, "max_steps": 0}
    with pytest.raises(ValueError, match="max_steps"):
        G.create(p, dev)


# ------------------------------------------------------------------------------------------- rlx_her_relabel_episode
def _relabel_case(rlx, dev, T, k, first_step, ring_steps, D, goal_at, achieved_at, G, action_dim, metric, threshold,
                  n_base=None, n_env=3, env=1, seed=0):
    rng = np.random.RandomState(seed)
    n_base = T if n_base is None else n_base
    R = n_env * ring_steps
    rows = R * (1 + k)
    obs_e = (rng.randint(0, 3, size=(T, D)) * 0.5).astype(np.float32)
    nxt_e = (rng.randint(0, 3, size=(T, D)) * 0.5).astype(np.float32)
    if action_dim is None:
        act_e, act = rng.randint(0, 9, size=T).astype(np.int32), np.full(rows, -7, dtype=np.int32)
    else:
        act_e = rng.randn(T, action_dim).astype(np.float32)
        act = np.full((rows, action_dim), np.nan, dtype=np.float32)
    obs, nxt = np.full((rows, D), np.nan, np.float32), np.full((rows, D), np.nan, np.float32)
    rew, go = np.full(rows, np.nan, np.float32), np.full(rows, 255, np.uint8)
    real = ((first_step + np.arange(T)) % ring_steps) * n_env + env
    obs[real], nxt[real], act[real] = obs_e, nxt_e, act_e
    rew[real], go[real] = rng.randn(T).astype(np.float32), 0
    sel = rng.randint(0, T, size=n_base * k).astype(np.int32)
    before = [a.copy() for a in (obs, nxt, act, rew, go)]
    t = [torch.from_numpy(a).to(dev) for a in (obs, nxt, act, rew, go)]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    from coach_amd import _rlx
    code = _rlx.CONSTANTS["RLX_HER_EUCLIDEAN" if metric == HR.EUCLIDEAN else "RLX_HER_MANHATTAN"]
    rlx.her_relabel_episode(t[0], t[1], t[2], t[3], t[4], torch.from_numpy(sel).to(dev), first_step, T, n_base, k, env,
                            n_env, ring_steps, D, goal_at, achieved_at, G, act[0].nbytes if act.ndim > 1 else 4, code,
                            float(threshold), 1.5, -0.25, status, _rlx.current_stream())
    got = [x.cpu().numpy() for x in t]
    assert int(status.item()) == 0
    o, no, a, r, g = HR.relabel(obs_e, nxt_e, act_e, sel, n_base, k, goal_at, achieved_at, G, metric, threshold, 1.5,
                                -0.25)
    copies = (R + real[:n_base, None] * k + np.arange(k)[None, :]).reshape(-1)
    for have, want in zip(got, (o, no, a, r, g)):
        assert have[copies].tobytes() == want.tobytes()
    untouched = np.ones(rows, dtype=bool)
    untouched[copies] = False
    for have, was in zip(got, before):                        # real rows as they were, every other row still NaN / filler
        assert have[untouched].tobytes() == was[untouched].tobytes()
    assert np.isnan(got[0][untouched & ~np.isin(np.arange(rows), real)]).all()


@pytest.mark.parametrize("case", [
    dict(T=1, k=1, first_step=0, D=5, goal_at=0, achieved_at=2, G=2, action_dim=None),          # the smallest episode
    dict(T=6, k=2, first_step=12, D=5, goal_at=0, achieved_at=3, G=2, action_dim=None),         # T = the ring's limit
    dict(T=4, k=4, first_step=4, D=7, goal_at=4, achieved_at=1, G=3, action_dim=3),             # wraps the ring's end
    dict(T=5, k=1, first_step=3, D=9, goal_at=6, achieved_at=0, G=3, action_dim=3),             # goal slice last, wraps
    dict(T=3, k=3, first_step=1, D=70, goal_at=0, achieved_at=35, G=35, action_dim=None),       # wider than one wave
    dict(T=4, k=2, first_step=2, D=5, goal_at=3, achieved_at=1, G=2, action_dim=None, n_base=3),  # Future: last skipped
], ids=lambda c: "T%d-k%d-D%d" % (c["T"], c["k"], c["D"]))
@pytest.mark.parametrize("metric,threshold", [(HR.EUCLIDEAN, 0.0), (HR.EUCLIDEAN, 0.75), (HR.MANHATTAN, 0.5)])
def test_relabel_kernel_equals_the_restatement_and_touches_no_other_row(rlx, dev, case, metric, threshold):
    _relabel_case(rlx, dev, ring_steps=6, metric=metric, threshold=threshold, seed=case["T"] * 10 + case["k"], **case)


def test_relabel_kernel_flags_a_selected_step_outside_the_episode(rlx, dev):
    from coach_amd import _rlx
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    obs, nxt, act, rew, go = z(12, 4), z(12, 4), z(12, dt=torch.int32), z(12), z(12, dt=torch.uint8)
    status = z(1, dt=torch.int32)
    sel = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    rlx.her_relabel_episode(obs, nxt, act, rew, go, sel, 0, 2, 2, 1, 0, 1, 6, 4, 0, 2, 2, 4, 0, 0.0, 2.0, -1.0, status,
                            _rlx.current_stream())
    assert int(status.item()) == 4 and float(rew[6].item()) == 2.0 and float(rew[7].item()) == 0.0   # copy 1: not written
    with pytest.raises(_rlx.RlxError, match="bad episode"):
        rlx.her_relabel_episode(obs, nxt, act, rew, go, sel, 0, 7, 2, 1, 0, 1, 6, 4, 0, 2, 2, 4, 0, 0.0, 0.0, -1.0,
                                status, _rlx.current_stream())


# ------------------------------------------------------------------------------------------------------- the memory
def _space(metric="Euclidean", threshold=0.0, rewards=(0.0, -1.0), goal_name="achieved"):
    return GoalsSpace(goal_name=goal_name, reward_type=ReachingGoal(threshold, rewards[0], rewards[1]),
                      distance_metric=GoalsSpace.DistanceMetric[metric])


def _memory(dev, max_size, k, method, slices, D, n_env, Tmax, action_dim=None, **space):
    return EpisodicHindsightExperienceReplay(
        (MemoryGranularity.Transitions, max_size), k, HindsightGoalSelectionMethod[method], _space(**space),
        observation_slices=slices, max_episode_length=Tmax, device=dev, n_env=n_env, observation_shape=(D,),
        action_dim=action_dim, min_episode_length=1)


def _listed(mem):
    n = mem.num_transitions_in_complete_episodes()
    if n == 0:
        return None
    b = mem.gather(mem.physical_rows(np.arange(n)), n)
    return {"obs": b["state"].cpu().numpy(), "next_obs": b["next_state"].cpu().numpy(),
            "action": b["action"].cpu().numpy(), "reward": b["reward"].cpu().numpy(),
            "game_over": b["game_over"].cpu().numpy()}


def _same(listed, flat):
    for key in ("obs", "next_obs", "action", "reward", "game_over"):
        assert listed[key].tobytes() == flat[key].astype(listed[key].dtype).tobytes(), key


@pytest.mark.parametrize("c", range(24))
def test_memory_with_one_env_lists_what_the_reference_memory_lists(dev, c):
    """tests/golden/her.npz: the reference's own flat list after every store, and its use of the host stream"""
    her = np.load(os.path.join(GOLDEN, "her.npz"))
    case = json.loads(str(her["cases"]))[c]
    layout = json.loads(str(her["layouts"]))[case["layout"]]
    mem = _memory(dev, case["max_size"], case["k"], case["method"], layout, 5, 1, 7, metric=case["metric"],
                  threshold=case["threshold"], rewards=case["rewards"])
    np.random.seed(1000 + c)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
    for s, T in enumerate(her["episode_lengths"].tolist()):
        p = "c%d_s%d_" % (c, s)
        obs, nxt = her[p + "in_obs"], her[p + "in_next_obs"]
        for t in range(T):
            mem.reset(up(obs[t:t + 1], torch.float32))           # the fabricated episodes' states are independent draws
            mem.store(up(her[p + "in_action"][t:t + 1], torch.int32), up(her[p + "in_reward"][t:t + 1], torch.float32),
                      up(her[p + "in_game_over"][t:t + 1], torch.uint8), up(nxt[t:t + 1], torch.float32),
                      up(obs[t:t + 1], torch.float32), dones_host=np.array([t == T - 1]))
        _same(_listed(mem), {k: her[p + k] for k in ("obs", "next_obs", "action", "reward", "game_over")})
        state = np.random.get_state()
        assert np.random.random() == float(her[p + "peek"])
        np.random.set_state(state)
    mem.check_status()


@pytest.mark.parametrize("method,k,action_dim", [("Final", 1, None), ("Future", 2, 3), ("Episode", 3, None)])
def test_memory_with_three_envs_equals_the_restatement(dev, method, k, action_dim):
    """episodes end on different steps (and two on the same one); extended episodes are evicted as wholes; the ring of real
    rows wraps several times"""
    n_env, D, Tmax, steps = 3, 6, 4, 40
    slices = {"other": (0, 1), "achieved": (1, 3), "desired_goal": (3, 5), "tail": (5, 6)}
    lengths = ([2, 3, 1, 4], [3, 1, 4, 2], [4, 4, 2])          # per env, cycled
    rng = np.random.RandomState(k)
    mem = _memory(dev, 30, k, method, slices, D, n_env, Tmax, action_dim, metric="Manhattan", threshold=0.5)
    ref = HR.HindsightReplay(30, k, method, 3, 1, 2, HR.MANHATTAN, 0.5)
    draw_obs = lambda: (rng.randint(0, 3, size=(n_env, D)) * 0.5).astype(np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cur = draw_obs()
    mem.reset(up(cur))
    open_eps = [[] for _ in range(n_env)]
    ep_i, t_in = [0] * n_env, [0] * n_env
    feed, checks = [], []                                      # (episode columns) in completion order; device snapshots
    np.random.seed(123)
    for step in range(steps):
        act = rng.randint(0, 5, size=n_env).astype(np.int32) if action_dim is None else \
            rng.randn(n_env, action_dim).astype(np.float32)
        rew = (rng.randint(-4, 5, size=n_env) * 0.25).astype(np.float32)
        nxt, rst = draw_obs(), draw_obs()
        done = np.zeros(n_env, dtype=bool)
        for e in range(n_env):
            t_in[e] += 1
            done[e] = t_in[e] == lengths[e][ep_i[e] % len(lengths[e])]
            open_eps[e].append((cur[e].copy(), nxt[e].copy(), act[e].copy(), rew[e], np.uint8(done[e])))
        mem.store(up(act), up(rew), up(done.astype(np.uint8)), up(nxt), up(rst), dones_host=done)
        for e in np.nonzero(done)[0]:                          # completion order, ties in env order
            feed.append([np.array(col) for col in zip(*open_eps[e])])
            open_eps[e], t_in[e] = [], 0
            ep_i[e] += 1
        cur = np.where(done[:, None], rst, nxt)
        if done.any():
            state = np.random.get_state()
            checks.append((len(feed), _listed(mem), mem.num_transitions_in_complete_episodes(),
                           mem.num_complete_episodes(), np.random.random()))
            np.random.set_state(state)
    draws_dev = mem.sample_indices(16)
    batch = mem.sample(8)
    got = {"obs": batch.states(["observation"])["observation"].cpu().numpy()} \
        if hasattr(batch, "states") else None
    with pytest.raises((KeyError, ValueError)):
        batch.info("n_step_discounted_rewards")                # this memory does not provide the column
    mem.check_status()
    # the restatement, fed the same episodes in the same order from the same stream
    np.random.seed(123)
    fed = 0
    for n_fed, listed, n_tr, n_ep, peek in checks:
        while fed < n_fed:
            ref.store_episode(*feed[fed])
            fed += 1
        assert n_tr == ref.num_transitions_in_complete_episodes() and n_ep == ref.num_complete_episodes()
        _same(listed, ref.flat())
        state = np.random.get_state()
        assert np.random.random() == peek
        np.random.set_state(state)
    assert np.array_equal(draws_dev, ref.sample_indices(16))
    idx = ref.sample_indices(8)
    assert np.array_equal(np.asarray(batch.info("logical_idx")), idx)
    if got is not None:
        assert got["obs"].tobytes() == ref.flat()["obs"][idx].tobytes()
    assert len(checks) > 8 and ref.num_transitions_in_complete_episodes() <= 30 < sum(f[0].shape[0] for f in feed)
    assert mem._gstep > 2 * mem._ring_steps or mem._gstep == steps


def test_memory_drops_an_open_episode_on_reset_and_stores_nothing_while_evaluating(dev):
    slices = {"desired_goal": (0, 2), "state": (2, 4)}
    mem = _memory(dev, 40, 1, "Final", slices, 4, 2, 3, goal_name="state")
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    args = (z(2, dt=torch.int32), z(2), z(2, dt=torch.uint8), z(2, 4), z(2, 4))
    mem.reset(z(2, 4))
    mem.store(*args, dones_host=np.array([False, False]))
    mem.drop_open_episode()
    mem.store(*args, dones_host=np.array([True, False]))
    assert mem.episode_lengths() == [2] and mem.open_transitions() == 1         # one real row + its copy
    mem.begin_evaluation(z(2, 4))
    mem.store(*args, record=False, dones_host=np.array([True, True]))
    with pytest.raises(RuntimeError, match="evaluation"):
        mem.store(*args, dones_host=np.array([True, True]))
    mem.end_evaluation(z(2, 4))
    assert mem.num_transitions_in_complete_episodes() == 2


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_what_is_supported(dev):
    slices = {"desired_goal": (0, 2), "achieved": (2, 4)}
    kw = dict(observation_slices=slices, max_episode_length=3, device=dev, n_env=1, observation_shape=(4,))
    size = (MemoryGranularity.Transitions, 12)
    M = HindsightGoalSelectionMethod
    with pytest.raises(ValueError, match="Final, Future, Episode"):
        EpisodicHindsightExperienceReplay(size, 1, M.Random, _space(), **kw)
    for metric in (GoalsSpace.DistanceMetric.Cosine, lambda a, b: 0.0):
        with pytest.raises(ValueError, match="Euclidean and Manhattan"):
            EpisodicHindsightExperienceReplay(size, 1, M.Final, GoalsSpace("achieved", ReachingGoal(0), metric), **kw)
    with pytest.raises(ValueError, match="ReachingGoal"):
        EpisodicHindsightExperienceReplay(size, 1, M.Final, GoalsSpace("achieved", InverseDistanceFromGoal(0.1),
                                                                       GoalsSpace.DistanceMetric.Euclidean), **kw)
    with pytest.raises(ValueError, match="scalar"):
        EpisodicHindsightExperienceReplay(size, 1, M.Final, GoalsSpace("achieved", ReachingGoal(np.zeros(2)),
                                                                       GoalsSpace.DistanceMetric.Euclidean), **kw)
    with pytest.raises(ValueError, match="no slice named"):
        EpisodicHindsightExperienceReplay(size, 1, M.Final, _space(goal_name="state"), **kw)
    mem = EpisodicHindsightExperienceReplay(size, 1, M.Final, _space(), **kw)
    with pytest.raises(ValueError, match="cannot store a single transition"):
        mem.store(object())


def test_pal_refuses_the_hindsight_memory_and_embedder_names_must_be_the_environments_slices(dev):
    from coach_amd.architectures.embedder_parameters import InputEmbedderParameters
    from coach_amd.base_parameters import EmbedderScheme
    gm = importlib.import_module("coach_amd.presets.CartPole_PAL").make()
    gm.device = dev
    gm.agent_params.memory = EpisodicHindsightExperienceReplayParameters()
    with pytest.raises(ValueError, match="hindsight replay does not provide"):
        gm.create_graph()
    gm = importlib.import_module("coach_amd.presets.BitFlip_DQN").make(bit_length=4)
    gm.device = dev
    gm.agent_params.network_wrappers["main"].input_embedders_parameters = {
        "state": InputEmbedderParameters(scheme=EmbedderScheme.Empty),
        "achieved_goal": InputEmbedderParameters(scheme=EmbedderScheme.Empty)}
    with pytest.raises(ValueError, match="do not match the environment's observation slices"):
        gm.create_graph()
    gm = importlib.import_module("coach_amd.presets.CartPole_DQN").make()
    gm.device = dev
    gm.agent_params.network_wrappers["main"].input_embedders_parameters = {
        "state": InputEmbedderParameters(scheme=EmbedderScheme.Empty),
        "desired_goal": InputEmbedderParameters(scheme=EmbedderScheme.Empty)}
    with pytest.raises(ValueError, match="do not match the environment's observation slices"):
        gm.create_graph()


# --------------------------------------------------------------------------------------------------------- cadence
def test_her_preset_trains_40_updates_per_16_finished_episodes_and_mixes_the_target_twice(dev):
    """BitFlip_DQN_HER at 4 bits, two envs.  The rule (agent.py:662-699 per finished episode): a phase of 40 updates when
    at least 16 episodes finished since the last phase; the marker moves to the current count.  Two envs may finish on
    the same step, so the count can pass 16 or 32 without stopping there: the test restates the rule on the counts it
    observes, and where the counts do stop at 16 and 32 that is `training_iteration == 80 after exactly 32 episodes`."""
    from coach_amd.core_types import RunPhase
    gm = importlib.import_module("coach_amd.presets.BitFlip_DQN_HER").make(num_envs=2, bit_length=4)
    gm.device = dev
    gm.visualization_parameters.dump_csv = False
    gm.create_graph()
    agent = gm.agent
    assert isinstance(agent.memory, EpisodicHindsightExperienceReplay) and agent.memory.k == 1
    assert (agent.memory._goal_at, agent.memory._achieved_at, agent.memory._goal_dim) == (0, 4, 4)
    gm._set_phase(RunPhase.TRAIN)
    net = agent.networks["main"]
    marker = phases = 0
    counts = []
    while phases < 2:
        agent.act()
        count = agent._train_episodes_finished
        counts.append(count)
        due = count - marker >= 16
        old_target, before = net.target.clone(), agent.training_iteration
        agent.train()
        if due:
            marker, phases = count, phases + 1
            # 40 updates, then ONE mix at rate 0.05 with the online weights the 40th update left
            expect = 0.95 * old_target.double() + 0.05 * net.params.weights.double()
            err = (net.target.double() - expect).abs().max().item()
            scale = max(old_target.abs().max().item(), net.params.weights.abs().max().item())
            assert err <= 4 * 2.0 ** -24 * scale, (err, scale)          # three fp32 roundings of values <= scale
            assert not torch.equal(net.target, old_target)
        else:
            assert torch.equal(net.target, old_target)
        assert agent.training_iteration == 40 * phases, (counts, agent.training_iteration)
        if count < 16:
            assert agent.training_iteration == 0 and before == 0        # no update before the 16th episode
    print("finished-episode counts per step: %s" % counts)
    assert agent.training_iteration == 80
    if 16 in counts and 32 in counts:
        assert counts[-1] == 32                                        # the second phase ran at exactly 32 episodes
    assert agent.memory.num_complete_episodes() == counts[-1]
    agent.check_status()
    gm.environment.check_status()


# --------------------------------------------------------------------------------------- the reference's own bars
def _bar(dev, name, num_envs):
    """improve() until ONE evaluation period's mean reward reaches the preset's threshold or the episode budget is
    spent.  (The reference's windowed rule divides the sum of fewer than 10 evaluations by 10, which negative rewards
    pass at the first evaluation; the plain mean asked for here is the stricter reading of the same bar.)"""
    import time
    gm = importlib.import_module("coach_amd.presets." + name).make(num_envs=num_envs, agent_seed=0)
    gm.device = dev
    pv = gm.preset_validation_params
    t0 = time.time()
    evals = lambda: [float(r["Evaluation Reward"]) for r in gm.logger.rows if r.get("Evaluation Reward", "") != ""]
    episodes = lambda: max([int(r["Episode #"]) for r in gm.logger.rows if r.get("Episode #", "") != ""] or [0])
    gm.improve(should_stop=lambda: evals()[-1] >= pv.min_reward_threshold or
               episodes() >= pv.max_episodes_to_achieve_reward)
    st = gm.validation_status()
    best = max(evals())
    print("%s (%d envs): evaluation reward %.2f after %d episodes (bar %.1f within %d), best %.2f, %d training "
          "iterations, %.1f s; reference rule passed: %s" % (
              name, num_envs, evals()[-1], episodes(), pv.min_reward_threshold, pv.max_episodes_to_achieve_reward, best,
              gm.agent.training_iteration, time.time() - t0, st["passed"]))
    assert torch.isfinite(gm.agent.networks["main"].params.weights).all()
    return evals()[-1] >= pv.min_reward_threshold and st["passed"]


def test_bit_flip_dqn_preset_reaches_the_reference_bar(dev):
    """presets/BitFlip_DQN.py:55-58: -7.9 within 10 000 episodes at 8 bits.  ONE run, one env, agent seed 0 — the only seed
    tried, and it passed (1 of 1).  On the MI355X: "BitFlip_DQN (1 envs): evaluation reward -7.50 after 5600 episodes (bar
    -7.9 within 10000), best -7.50, 14000 training iterations, 6.8 s; reference rule passed: True"."""
    assert _bar(dev, "BitFlip_DQN", 1)


def test_bit_flip_dqn_her_preset_reaches_the_reference_bar(dev):
    """presets/BitFlip_DQN_HER.py:67-70: -15 within 10 000 episodes at 20 bits.  ONE run, one env as in the reference,
    agent seed 0 — the only seed tried, and it passed (1 of 1).  On the MI355X: "HER one env: eval [-20.0, -20.0, -10.8]
    after 3200 episodes, 8000 iterations, 9.0 s" (the first two evaluations, at 800 and 1600 episodes, never reach the
    goal).  The same run with 16 envs — one vector episode is then one playing phase — takes 1.4 s: "BitFlip_DQN_HER
    (16 envs): evaluation reward -11.77 after 3201 episodes (bar -15.0 within 10000), best -11.77, 7840 training
    iterations, 1.4 s; reference rule passed: True"."""
    assert _bar(dev, "BitFlip_DQN_HER", 1)
