"""UCB over Q ensembles and the ExplorationChain on the MI355X: rlx_ucb_egreedy against tests/ucb_ref.py bit for bit,
rlx_chain_reset / rlx_chain_step against tests/exploration_chain_ref.py, a BootstrappedDQNAgent explored by UCB on the
chain (its host draws counted by hand: no head draw), the four presets constructing and stepping, an episode budget of
improve() counted in episodes, and one learning run of ExplorationChain_UCB_Q_ensembles against a bar derived from the
chain's rewards."""
import importlib

import numpy as np
import pytest
import torch

import exploration_chain_ref as CR
import ucb_ref as UR

pytestmark = pytest.mark.gpu
CHAIN_LEVEL = 'rl_coach.environments.toy_problems.exploration_chain:ExplorationChain'


def _t(x, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t if dtype is None else t.to(dtype)


# ---------------------------------------------------------------------------------------------------- rlx_ucb_egreedy
def _row(kind, K, A, rng):
    q = (rng.randn(K, A) * rng.choice([1e-3, 1.0, 1e3])).astype(np.float32)
    if kind == "equal":                                       # every head and action equal: std 0, the tie draw decides
        q[:] = np.float32(0.25)
    elif kind == "inf":
        q[rng.randint(K), rng.randint(A)] = np.inf
    elif kind == "nan":
        q[rng.randint(K), A - 1] = np.nan
    return q


def _ucb(rlx, dev, q, lamb, use_std, u, ra, tie, eps, pad=3, with_std=True):
    n, K, A = q.shape
    ld = K * A + pad
    rows = np.full((n, ld), np.nan, dtype=np.float32)         # NaN in the padding: nothing beyond K*A may be read
    rows[:, :K * A] = q.reshape(n, K * A)
    vals = torch.full((n, A), -7.0, dtype=torch.float32, device=dev)
    std = torch.full((n, A), -7.0, dtype=torch.float32, device=dev) if with_std else None
    acts = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rlx.ucb_egreedy(_t(rows, dev), ld, K, float(lamb), int(use_std), _t(np.asarray(u, np.float64), dev),
                    _t(np.asarray(ra, np.int32), dev), _t(np.asarray(tie, np.float64), dev), float(eps), n, A, vals, std,
                    acts, 0)
    return acts.cpu().numpy(), vals.cpu().numpy(), None if std is None else std.cpu().numpy()


@pytest.mark.parametrize("A", [2, 18])
@pytest.mark.parametrize("K", [1, 2, 20, 32])
@pytest.mark.parametrize("n_env", [1, 3])
def test_ucb_kernel_equals_the_restatement_bit_for_bit(rlx, dev, n_env, K, A):
    """values, std and action == tests/ucb_ref.py (NaNs match as NaNs: IEEE 754 leaves their sign and payload open), with
    ld = K*A + 3 and NaN in the padding, use_std on and off, lamb 0.1 and 10, std_out given and NULL; with three envs a
    forced-explore env next to greedy ones in the same call."""
    rng = np.random.RandomState(100 * n_env + 10 * K + A)
    layouts = [("random", "equal", "inf"), ("nan", "random", "equal")] if n_env == 3 else \
        [("random",), ("equal",), ("inf",), ("nan",)]
    for kinds in layouts:
        q = np.stack([_row(kind, K, A, rng) for kind in kinds])
        u = rng.uniform(0.4, 1.0, n_env)                      # greedy at epsilon 0.3 ...
        ra = np.full(n_env, 12345, dtype=np.int32)            # ... and a greedy env never takes the random action
        if n_env == 3:
            u[0], ra[0] = 0.1, rng.randint(A)                 # env 0 explores
        tie = rng.random_sample((n_env, A))
        for lamb in (0.1, 10):
            for use_std in (True, False):
                ref_vals, ref_std = UR.values(q, lamb, use_std)
                with np.errstate(all="ignore"):
                    ref_acts = UR.egreedy(ref_vals, u, ra, tie, 0.3)
                for with_std in (True, False):
                    acts, vals, std = _ucb(rlx, dev, q, lamb, use_std, u, ra, tie, 0.3, with_std=with_std)
                    where = (kinds, lamb, use_std, with_std)
                    assert UR.same_bits(vals, ref_vals), where
                    assert acts.tolist() == ref_acts.tolist(), where
                    if with_std and use_std:
                        assert UR.same_bits(std, ref_std), where
                    elif with_std:
                        assert (std == -7.0).all(), where      # not written without use_std
                if n_env == 3:
                    assert ref_acts[0] == ra[0] and 12345 not in ref_acts[1:].tolist()
                if "equal" in kinds:
                    e = kinds.index("equal")
                    assert len(set(ref_vals[e].tolist())) == 1 and (n_env == 3 and e == 0 or
                                                                    ref_acts[e] == int(np.argmax(tie[e])))
                if "nan" in kinds and use_std:
                    assert np.isnan(ref_vals[kinds.index("nan"), A - 1])
                if "inf" in kinds and use_std:
                    assert np.isnan(ref_vals[kinds.index("inf")]).any()     # inf - inf in the deviations


def test_ucb_kernel_bonus_changes_the_choice_and_refuses_large_shapes(rlx, dev):
    from coach_amd._rlx import RlxError
    # two heads agree on action 0 = 1.0; they disagree on action 1 (0.0 and 1.6: mean 0.8, std 0.8)
    q = np.array([[[1.0, 0.0], [1.0, 1.6]]], dtype=np.float32)
    u, ra, tie = [1.0], [0], [[0.5, 0.5]]
    greedy = _ucb(rlx, dev, q, 10, False, u, ra, tie, 0.0)
    bonus = _ucb(rlx, dev, q, 10, True, u, ra, tie, 0.0)
    assert greedy[0].tolist() == [0] and bonus[0].tolist() == [1]
    assert greedy[1].tolist() == [[1.0, np.float32(0.8)]] and bonus[2].tolist() == [[0.0, np.float32(0.8)]]
    z = torch.zeros(4096, dtype=torch.float32, device=dev)
    d = torch.zeros(64, dtype=torch.float64, device=dev)
    i = torch.zeros(64, dtype=torch.int32, device=dev)
    for K, A, ld in ((33, 2, 66), (2, 19, 38), (2, 2, 3), (0, 2, 4)):
        with pytest.raises(RlxError, match="bad shape"):
            rlx.ucb_egreedy(z, ld, K, 0.1, 1, d, i, d, 0.0, 1, A, z, z, i, 0)
    with pytest.raises(RlxError, match="null"):
        rlx.ucb_egreedy(z, 4, 2, 0.1, 1, d, i, d, 0.0, 1, 2, None, z, i, 0)


# ------------------------------------------------------------------------------------------------------ rlx_chain_*
def _make_env(dev, n_env, **kw):
    from coach_amd.environments.exploration_chain_vector_environment import (
        ExplorationChainVectorEnvironment, ExplorationChainVectorEnvironmentParameters)
    return ExplorationChainVectorEnvironment(ExplorationChainVectorEnvironmentParameters(n_env, **kw), dev)


@pytest.mark.parametrize("kind", ["Therm", "OneHot"])
@pytest.mark.parametrize("L", [4, 20])
@pytest.mark.parametrize("n_env", [1, 5])
def test_chain_kernels_equal_the_numpy_twin(dev, n_env, L, kind):
    """two full episodes: even envs walk into the left wall and then to the right end and into the right wall, odd envs
    go right from the start; start state 1 and, with five envs, L - 1"""
    max_steps = L + 7
    for start in ((1,) if n_env == 1 else (1, L - 1)):
        env = _make_env(dev, n_env, chain_length=L, start_state=start, max_steps=max_steps, observation_type=kind,
                        left_state_reward=0.1, right_state_reward=2.7)
        ref = CR.VectorExplorationChain(n_env, L, start, max_steps, kind == "Therm", 0.1, 2.7)
        assert np.array_equal(env.reset_internal_state().cpu().numpy(), ref.reset())
        walls, ends, paid = set(), 0, set()
        for step in range(2 * max_steps):
            t = step % max_steps
            a = np.array([(0 if t < 3 else 1) if e % 2 == 0 else 1 for e in range(n_env)], dtype=np.int32)
            before = ref.state.copy()
            r_next, r_reset, r_rew, r_done = ref.step(a)
            nxt, rst, rew, done = env.step(_t(a, dev))
            assert np.array_equal(nxt.cpu().numpy(), r_next), step
            assert np.array_equal(rew.cpu().numpy(), r_rew) and np.array_equal(done.cpu().numpy(), r_done), step
            assert np.array_equal(env.chain_state.cpu().numpy(), ref.state), step
            assert np.array_equal(env.step_in_episode.cpu().numpy(), ref.steps), step
            assert np.array_equal(env.dones_host, r_done != 0)             # the host's counter says the same
            paid |= set(r_rew.tolist())
            if r_done.any():
                assert r_done.all() and np.array_equal(rst.cpu().numpy(), r_reset) and t == max_steps - 1
                ends += 1
            else:
                walls |= {int(x) for x in a[ref.state == before]}
        assert ends == 2 and (walls == {0, 1} or (start == L - 1 and walls == {1}))
        if start == 1:                                        # the fp32 nearest the constructor's values, and 0 in between
            assert paid == {0.0, float(np.float32(0.1)), float(np.float32(2.7))}
        env.check_status()


def test_chain_single_step_episodes_and_forced_reset(dev):
    env = _make_env(dev, 3, chain_length=4, start_state=1, max_steps=1, observation_type="OneHot")
    first = env.reset_internal_state().cpu().numpy()
    assert first.tolist() == [[0, 1, 0, 0]] * 3
    for _ in range(2):
        nxt, rst, rew, done = env.step(torch.tensor([0, 1, 0], dtype=torch.int32, device=dev))
        assert nxt.cpu().tolist() == [[1, 0, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]] and done.cpu().tolist() == [1, 1, 1]
        assert rew.cpu().numpy().tolist() == [np.float32(1 / 1000), 0.0, np.float32(1 / 1000)]
        assert np.array_equal(rst.cpu().numpy(), first) and env.dones_host.all()
    env = _make_env(dev, 2, chain_length=6, start_state=2, max_steps=5)
    env.reset_internal_state()
    for _ in range(3):
        env.step(torch.ones(2, dtype=torch.int32, device=dev))
    assert env.chain_state.cpu().tolist() == [5, 5] and env.t_host.tolist() == [3, 3]
    assert env.reset_internal_state().cpu().tolist() == [[1, 1, 1, 0, 0, 0]] * 2       # Therm is the default
    assert env.chain_state.cpu().tolist() == [2, 2] and env.step_in_episode.cpu().tolist() == [0, 0]
    assert env.t_host.tolist() == [0, 0] and not env.dones_host.any()


def test_chain_out_of_range_action_sets_the_status_bit_and_moves_nothing(dev):
    env = _make_env(dev, 3, chain_length=8, start_state=3, max_steps=5)
    env.reset_internal_state()
    env.check_status()
    env.step(torch.tensor([2, -1, 1 << 30], dtype=torch.int32, device=dev))
    assert env.chain_state.cpu().tolist() == [3, 3, 3] and int(env.status.item()) == 2
    assert env.step_in_episode.cpu().tolist() == [1, 1, 1]
    with pytest.raises(RuntimeError, match="outside"):
        env.check_status()
    with pytest.raises(TypeError, match="int32"):
        env.step(torch.zeros(3, dtype=torch.int64, device=dev))


def test_gym_environment_create_builds_the_chain_for_both_parameter_classes(dev):
    from coach_amd.environments import gym_environment as G
    from coach_amd.environments.exploration_chain_vector_environment import ExplorationChainVectorEnvironment
    for cls in (G.GymVectorEnvironment, G.GymEnvironmentParameters):
        p = cls(level=CHAIN_LEVEL)
        p.additional_simulator_parameters = {'chain_length': 6, 'max_steps': 9, 'start_state': 2}
        p.num_envs = 2
        env = G.create(p, dev)
        assert isinstance(env, ExplorationChainVectorEnvironment)
        assert (env.p.num_envs, env.p.observation_shape, env.p.num_actions, env.p.episode_length) == (2, (6,), 2, 9)
        assert env.reset_internal_state().cpu().tolist() == [[1, 1, 1, 0, 0, 0]] * 2
        p.additional_simulator_parameters = {'chain_length': 6, 'max_steps': 9, 'mean_zero': True}
        with pytest.raises(ValueError, match="mean_zero"):
            G.create(p, dev)
        p.additional_simulator_parameters = {'chain_length': 6}
        with pytest.raises(ValueError, match="max_steps"):
            G.create(p, dev)


# -------------------------------------------------------------------------------------------------------- the agent
def _agent(dev, exploration, n_env=2, K=3, L=5, max_steps=6, eps=0.3, p=0.6, seed=5):
    from coach_amd.agents.bootstrapped_dqn_agent import BootstrappedDQNAgent, BootstrappedDQNAgentParameters
    from coach_amd.core_types import EnvironmentSteps
    from coach_amd.memories.memory import MemoryGranularity
    from coach_amd.schedules import ConstantSchedule
    ap = BootstrappedDQNAgentParameters()
    ap.seed = seed
    net = ap.network_wrappers["main"]
    net.batch_size = 8
    net.heads_parameters[0].num_output_head_copies = K
    net.heads_parameters[0].rescale_gradient_from_head_by_factor = 1.0 / K
    ap.exploration = exploration
    if hasattr(exploration, "architecture_num_q_heads"):
        ap.exploration.architecture_num_q_heads = K
        ap.exploration.bootstrapped_data_sharing_probability = p
    ap.exploration.epsilon_schedule = ConstantSchedule(eps)
    ap.memory.max_size = (MemoryGranularity.Transitions, 60)
    ap.algorithm.num_consecutive_playing_steps = EnvironmentSteps(1)
    ap.algorithm.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(7)
    env = _make_env(dev, n_env, chain_length=L, start_state=1, max_steps=max_steps)
    return BootstrappedDQNAgent(ap, env, dev)


def test_ucb_agent_acts_stores_updates_and_draws_no_head(dev):
    """Two envs, K = 3, batch 8, data-sharing probability 0.6, epsilon 0.3.  The host stream after 8 heat-up and 30
    training steps equals a hand count of the reference's calls with UCB: per step and env one binomial(1, p, K) (observe),
    the heat-up's random action or EGreedy's draws (explore: choice(A); greedy: random(A); then rand()), one more
    binomial at once for an env whose episode ended, and the replay's randint per update -- and NO randint(K) head draw
    at an episode's start, which Bootstrapped makes."""
    from coach_amd.core_types import RunPhase
    from coach_amd.exploration_policies.ucb import UCB, UCBParameters
    a = _agent(dev, UCBParameters())
    pol, K, A, n, p, eps = a.exploration_policy, 3, 2, 2, 0.6, 0.3
    assert isinstance(pol, UCB) and a.ucb and not hasattr(pol, "selected_head")
    log = []                                                  # ("act", phase, dones) / ("replay", n, size), in call order
    sample = a.memory.sample_indices
    a.memory.sample_indices = lambda size: (log.append(("replay", a.memory.num_transitions(), size)), sample(size))[1]
    np.random.seed(21)
    u = pol.current_random_value.copy()
    seen_std = []
    for step in range(38):
        a.phase = RunPhase.HEATUP if step < 8 else RunPhase.TRAIN
        a.act()
        log.append(("act", a.phase, a.env.dones_host.copy()))
        if a.phase == RunPhase.TRAIN:
            # the launch acted on mean + lamb * std of the heads' values it was given
            q = a._q_act.cpu().numpy().reshape(n, K, A)
            vals, std = UR.values(q, pol.lamb, True)
            assert UR.same_bits(a.last_action_values.cpu().numpy(), vals) and UR.same_bits(pol.std.cpu().numpy(), std)
            assert np.array_equal(np.asarray(pol.get_control_param()), std.mean(axis=1))
            seen_std.append(float(std.max()))
            a.train()
    after = np.random.get_state()
    assert a.training_iteration == 60 and a._heads_dev is None and max(seen_std) > 0   # one update per env-step
    a.check_status()
    a.env.check_status()
    # the hand count
    np.random.seed(21)
    explored = greedy = terminal = 0
    for item in log:
        if item[0] == "replay":
            np.random.randint(item[1], size=item[2])
            continue
        _, phase, dones = item
        for e in range(n):
            np.random.binomial(1, p, K)                       # observe: the previous (or initial) response
        for e in range(n):
            if phase == RunPhase.HEATUP:
                np.random.choice(A)                           # the heat-up's random action
                continue
            if u[e] < eps:
                np.random.choice(A)
                explored += 1
            else:
                np.random.random(A)
                greedy += 1
            u[e] = np.random.rand()
        for e in np.nonzero(dones)[0]:
            np.random.binomial(1, p, K)                       # observe of the terminal response
            terminal += 1
    ref = np.random.get_state()
    assert explored > 0 and greedy > 0 and terminal >= 10 and sum(1 for i in log if i[0] == "replay") == 60
    assert np.array_equal(after[1], ref[1]) and after[2:] == ref[2:]
    # TEST acts on the mean (no bonus, no vote) and leaves std as TRAIN's last launch wrote it
    std_before = pol.std.clone()
    a.phase = RunPhase.TEST
    a.act()
    q = a._q_act.cpu().numpy().reshape(n, K, A)
    mean, _ = UR.values(q, pol.lamb, False)
    assert UR.same_bits(a.last_action_values.cpu().numpy(), mean) and torch.equal(pol.std, std_before)
    assert not np.isin(a.last_action_values.cpu().numpy(), [0.0, 1.0]).all()     # (not the vote's one-hot vector)
    assert pol.get_control_param() == 0


def test_bootstrapped_agent_still_draws_its_heads_and_plain_egreedy_is_refused(dev):
    from coach_amd.exploration_policies.bootstrapped import BootstrappedParameters
    from coach_amd.exploration_policies.e_greedy import EGreedyParameters
    b = _agent(dev, BootstrappedParameters())
    assert not b.ucb and hasattr(b.exploration_policy, "selected_head")
    from coach_amd.core_types import RunPhase
    b.phase = RunPhase.TRAIN
    b.act()
    assert b._heads_dev is not None
    with pytest.raises(ValueError, match="BootstrappedParameters.*UCBParameters"):
        _agent(dev, EGreedyParameters())


def _small(gm, dev):
    from coach_amd.memories.memory import MemoryGranularity
    gm.device = dev
    gm.visualization_parameters.dump_csv = False
    gm.agent_params.memory.max_size = (MemoryGranularity.Transitions, 512)
    for net in gm.agent_params.network_wrappers.values():
        net.batch_size = 16
    return gm


@pytest.mark.parametrize("name", ["ExplorationChain_UCB_Q_ensembles", "ExplorationChain_Bootstrapped_DQN",
                                  "ExplorationChain_Dueling_DDQN", "Atari_UCB_with_Q_Ensembles"])
def test_presets_construct_and_step(dev, name):
    """the preset's own agent and environment (a small memory and batch), heat-up, training steps and one evaluation"""
    from coach_amd.core_types import RunPhase
    mod = importlib.import_module("coach_amd.presets." + name)
    atari = name.startswith("Atari")
    gm = _small(mod.make(level="breakout", num_envs=2) if atari else mod.make(num_envs=2), dev)
    if atari:
        gm.env_params.episode_length = 8
    gm.create_graph()
    agent, env = gm.agent, gm.environment
    if atari:
        assert type(env).__name__ == "SyntheticVectorEnvironment" and agent.K == 10 and agent.A == 4
    else:
        assert type(env).__name__ == "ExplorationChainVectorEnvironment"
        assert (env.p.chain_length, env.p.episode_length, env.p.start_state, env.therm) == (20, 27, 1, 1)
        assert agent.A == 2 and getattr(agent, "K", 20) == 20
    if "UCB" in name:
        assert agent.ucb and float(agent.exploration_policy.lamb) == (0.1 if atari else 10)
    gm._set_phase(RunPhase.HEATUP)
    for _ in range(10):
        agent.act()
    gm._set_phase(RunPhase.TRAIN)
    for _ in range(12):
        agent.act()
        agent.train()
    assert agent.training_iteration > 0
    ev = agent.evaluate_episodes(1)
    assert np.isfinite(ev) and torch.isfinite(agent.networks["main"].params.weights).all()
    agent.check_status()
    gm.check_status()


# ------------------------------------------------------------------------- improve_steps in episodes, the learning run
@pytest.mark.parametrize("name,kw,k,every", [("ExplorationChain_UCB_Q_ensembles", {}, 20, 10),
                                             ("BitFlip_DQN_HER", {"bit_length": 4}, 24, 8)])
def test_improve_counts_an_episode_budget_in_episodes(dev, name, kw, k, every):
    """improve_steps = EnvironmentEpisodes(k) ends improve() after k training episodes (graph_manager.py:536-539 counts
    in the unit given), not after k env-steps -- which would end the chain preset after its first period of 10 episodes
    and BitFlip_DQN_HER, whose budget is given in episodes too, after its first period of 8."""
    from coach_amd.core_types import EnvironmentEpisodes, RunPhase
    gm = _small(importlib.import_module("coach_amd.presets." + name).make(num_envs=1, **kw), dev)
    gm.schedule.improve_steps = EnvironmentEpisodes(k)
    gm.schedule.steps_between_evaluation_periods = EnvironmentEpisodes(every)
    gm.schedule.evaluation_steps = EnvironmentEpisodes(1)
    rows = gm.improve()
    assert gm.train_episodes == k == gm.agent._train_episodes_finished
    assert sum(1 for r in rows if r.get("Evaluation Reward", "") != "") == k // every
    assert gm.total_steps_counters[RunPhase.TRAIN] > k         # (more env-steps than episodes were played)


def test_ucb_q_ensembles_preset_finds_the_right_end(dev):
    """ExplorationChain_UCB_Q_ensembles, ONE run, one env, agent seed 0.  The bar is derived: an episode that never reaches
    the right end collects at most 27 * 0.001 = 0.027 (every step at the left end), and one step at the right end pays 1,
    so an evaluation episode whose return is >= 1.0 proves the right end was found; the optimum from start state 1 is
    10.0.  Asserted: such an evaluation episode within the preset's 2 000 training episodes.  The only run made, on the
    MI355X: "18 evaluations after 180 training episodes, first >= 1.0 at evaluation 18, best 10.000, 1215 training
    iterations, 1.0 s" (seventeen evaluations of 0.0 before it)."""
    import time
    gm = importlib.import_module("coach_amd.presets.ExplorationChain_UCB_Q_ensembles").make(num_envs=1, agent_seed=0)
    gm.device = dev
    gm.visualization_parameters.dump_csv = False
    evals = lambda: [float(r["Evaluation Reward"]) for r in gm.logger.rows if r.get("Evaluation Reward", "") != ""]
    t0 = time.time()
    gm.improve(should_stop=lambda: evals()[-1] >= 1.0)
    ev = evals()
    print("ExplorationChain_UCB_Q_ensembles: %d evaluations after %d training episodes, first >= 1.0 at evaluation %s, "
          "best %.3f, %d training iterations, %.1f s; curve %s" % (
              len(ev), gm.train_episodes, next((i + 1 for i, r in enumerate(ev) if r >= 1.0), None), max(ev),
              gm.agent.training_iteration, time.time() - t0, [round(r, 3) for r in ev]))
    assert gm.train_episodes <= 2000
    assert torch.isfinite(gm.agent.networks["main"].params.weights).all()
    assert max(ev) >= 1.0
