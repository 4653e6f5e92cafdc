"""Pendulum-v0 and Acrobot-v1 on the device (csrc/classic_control.hip) and the full-range sin / cos under them
(csrc/libm_sincos_full.hpp).  gym is not installed: the reference is the restatement below of gym 0.12.5's pendulum.py /
acrobot.py ("book" dynamics, one rk4 step of 0.2 s) in Python floats with math.sin / math.cos, the host libm.
Tolerance of the fp64 states: atol 1e-12 — the states are O(1) to O(100) and a step is a few dozen (Acrobot: a few
hundred) flops on sin / cos within 1 ulp, so 1e-12 is hundreds of ulps above rounding and six orders of magnitude below
what a wrong constant, order or modulo produces.
"""
import math

import numpy as np
import pytest

PI, F64, F32 = math.pi, np.float64, np.float32
pytestmark = pytest.mark.gpu


def pendulum_ref(th, thdot, a):
    """-> (newth, newthdot, reward) of pendulum.py `step`; a is the raw action, clipped in fp32 and widened"""
    u = float(min(max(F32(a), F32(-2.0)), F32(2.0)))
    an = ((th + PI) % (2 * PI)) - PI                                         # angle_normalize: Python's floored modulo
    costs = an * an + .1 * (thdot * thdot) + .001 * (u * u)
    newthdot = thdot + (-3 * 10. / (2 * 1.) * math.sin(th + PI) + 3. / (1. * 1. ** 2) * u) * .05
    return th + newthdot * .05, min(max(newthdot, -8.), 8.), -costs


def _dsdt(s, a):
    m1 = m2 = l1 = I1 = I2 = 1.
    lc1, lc2, g = 0.5, 0.5, 9.8
    theta1, theta2, dtheta1, dtheta2 = s
    d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * math.cos(theta2)) + I1 + I2
    d2 = m2 * (lc2 ** 2 + l1 * lc2 * math.cos(theta2)) + I2
    phi2 = m2 * lc2 * g * math.cos(theta1 + theta2 - PI / 2.)
    phi1 = - m2 * l1 * lc2 * (dtheta2 * dtheta2) * math.sin(theta2) \
        - 2 * m2 * l1 * lc2 * dtheta2 * dtheta1 * math.sin(theta2) \
        + (m1 * lc1 + m2 * l1) * g * math.cos(theta1 - PI / 2) + phi2
    ddtheta2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * (dtheta1 * dtheta1) * math.sin(theta2) - phi2) \
        / (m2 * lc2 ** 2 + I2 - d2 * d2 / d1)
    return (dtheta1, dtheta2, -(d2 * ddtheta2 + phi1) / d1, ddtheta2)


def acrobot_ref(s, action):
    """-> (next state, reward, terminal) of acrobot.py `step`"""
    a, dt = action - 1., .2
    k1 = _dsdt(s, a)
    k2 = _dsdt([y + dt / 2. * k for y, k in zip(s, k1)], a)
    k3 = _dsdt([y + dt / 2. * k for y, k in zip(s, k2)], a)
    k4 = _dsdt([y + dt * k for y, k in zip(s, k3)], a)
    ns = [y + dt / 6.0 * (a1 + 2 * a2 + 2 * a3 + a4) for y, a1, a2, a3, a4 in zip(s, k1, k2, k3, k4)]
    for j in (0, 1):                                                         # wrap(x, -pi, pi)
        while ns[j] > PI:
            ns[j] -= 2 * PI
        while ns[j] < -PI:
            ns[j] += 2 * PI
    ns[2], ns[3] = min(max(ns[2], -4 * PI), 4 * PI), min(max(ns[3], -9 * PI), 9 * PI)
    terminal = bool(-math.cos(ns[0]) - math.cos(ns[1] + ns[0]) > 1.)
    return ns, (0. if terminal else -1.), terminal


def _env(dev, kind, n, **kw):
    from coach_amd.environments import classic_control_vector_environment as cc
    env = getattr(cc, kind + "VectorEnvironment")(getattr(cc, kind + "VectorEnvironmentParameters")(n, **kw), dev)
    env.reset_internal_state()
    return env


def _step_from(env, states, actions):
    import torch
    env.state.copy_(torch.from_numpy(np.asarray(states, dtype=F64)))
    env.step(torch.from_numpy(actions).to(env.device))
    return env.next_state64.cpu().numpy(), env.reward.cpu().numpy(), env.next_obs.cpu().numpy()


def _sincos(fn, dev, x):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=F64)).to(dev)
    s, c, status = torch.empty_like(xd), torch.empty_like(xd), torch.zeros(1, dtype=torch.int32, device=dev)
    fn(xd, s, c, x.size, status, 0)
    return s.cpu().numpy(), c.cpu().numpy(), int(status.item())


def _ulps(a, b):
    o = lambda v: np.where(v.view(np.int64) < 0, np.int64(-2 ** 63) - v.view(np.int64), v.view(np.int64))
    return np.abs(o(a) - o(b))


def _around(x0, k):                                                          # x0 and its k neighbours on either side
    out = [x0]
    for _ in range(k):
        out = [np.nextafter(out[0], -np.inf)] + out + [np.nextafter(out[-1], np.inf)]
    return out


def _arguments(name):
    if name == "first_branch_boundary":
        x = _around(0.85546875, 3)                                           # high word 0x3feb6000
    elif name == "second_branch_boundary":
        x = _around(float.fromhex("0x1.368fdp+1"), 3)                        # high word 0x400368fd: 2.426265
    elif name == "multiples_of_half_pi":                                     # the reduction's cancellation cases
        ks = list(range(1, 65)) + [2 ** j for j in range(7, 20)] + [667544] + \
            np.random.RandomState(5).randint(65, 667544, size=400).tolist()
        x = [v for k in ks for v in _around(k * (PI / 2), 2)] + [np.nextafter(2.0 ** 20, 0.0)]
    elif name == "taylor_table_switch":                 # reduced to 0.126 <= |a| < 0.126016, where a * a < 0.01588 still
        x = [float.fromhex(h) for h in ("0x1.ac65fbe4321dp+16", "0x1.538b4546979c5p+7", "0x1.5d706ddd6e551p+9",
                                        "0x1.cf2e18f719759p+19", "0x1.2a6367ba18101p+9")]
    elif name == "random_100":
        x = (np.random.RandomState(6).random_sample(4000) * 200 - 100).tolist()
    else:                                                                    # zeros_and_denormals
        x = [0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 2.0 ** -27, 2.0 ** -26]
    return np.concatenate([np.array(x, dtype=F64), -np.array(x, dtype=F64)])


@pytest.mark.parametrize("name", ["first_branch_boundary", "second_branch_boundary", "multiples_of_half_pi",
                                  "taylor_table_switch", "random_100", "zeros_and_denormals"])
def test_full_range_sincos_within_one_ulp_of_libm(rlx, dev, name):
    x = _arguments(name)
    s, c, status = _sincos(rlx.libm_sincos_full, dev, x)
    ref_s, ref_c = np.array([math.sin(v) for v in x]), np.array([math.cos(v) for v in x])
    us, uc = _ulps(s, ref_s), _ulps(c, ref_c)
    print("%s: %d points, not bit-identical: sin %d cos %d" % (name, x.size, (us > 0).sum(), (uc > 0).sum()))
    assert status == 0 and us.max() <= 1 and uc.max() <= 1
    assert np.array_equal(np.signbit(s), np.signbit(ref_s))                  # -0.0 stays -0.0
    first = np.abs(x) < 0.85546875                                           # the table functions' domain: their bits
    if first.any():
        s0, c0, st = _sincos(rlx.libm_sincos, dev, x[first])
        assert st == 0 and s0.tobytes() == s[first].tobytes() and c0.tobytes() == c[first].tobytes()


@pytest.mark.parametrize("v", [2.0 ** 20, -2.0 ** 20, 3e6, 1e22])
def test_full_range_sincos_flags_arguments_from_two_to_the_twenty(rlx, dev, v):
    s, c, status = _sincos(rlx.libm_sincos_full, dev, np.array([1.0, v]))
    assert status == 1 and abs(s[1] - math.sin(v)) < 1e-15 and abs(c[1] - math.cos(v)) < 1e-15


def test_pendulum_steps_equal_the_restatement(rlx, dev):
    below = np.nextafter(PI, 0.0)
    cases = [(th, thdot, u) for th in (0.0, PI, -PI, below, -below, 40.0, -40.0, 85.0, -85.0)
             for thdot in (0.0, 8.0, -8.0, 7.9, -7.9, 9.5, -9.5) for u in (0.0, 2.0, -2.0, 3.0, -3.0)]
    bad = [(1.0, 0.5, np.nan), (-85.0, 3.0, np.inf)]                         # non-finite actions: these two envs stay put
    rows, n = cases + bad, len(cases)                                        # 317 envs: five workgroups
    env = _env(dev, "Pendulum", len(rows))
    ns, reward, obs = _step_from(env, [c[:2] for c in rows], np.array([[c[2]] for c in rows], dtype=F32))
    ref = [pendulum_ref(*c) for c in cases]
    np.testing.assert_allclose(ns[:n], np.array([r[:2] for r in ref]), rtol=0, atol=1e-12)
    assert (np.abs(ns[:n, 1]) == 8.0).sum() >= 100                           # the velocity clip was exercised
    assert np.array_equal(reward[:n], np.array([r[2] for r in ref]).astype(F32))     # -cost: six flops, no sin / cos
    assert np.array_equal(ns[n:], [c[:2] for c in bad]) and not reward[n:].any() and int(env.status.item()) == 2
    s, c, status = _sincos(rlx.libm_sincos_full, dev, ns[:, 0])              # fp32 outputs: its own fp64, rounded
    assert status == 0 and np.array_equal(obs, np.stack([c, s, ns[:, 1]], axis=1).astype(F32))
    assert not env.game_over.any() and (env.step_in_episode == 1).all() and np.array_equal(env.state.cpu().numpy(), ns)


ACROBOT_STATES = [
    (0.0, 0.0, 0.0, 0.0), (PI - 1e-3, 0.1, 2.0, 0.0), (-PI + 1e-3, -0.1, -2.0, 0.0),    # hanging; theta1 crosses +-pi
    (0.2, PI - 1e-3, 0.0, 3.0), (-0.2, -PI + 1e-3, 0.0, -3.0),               # theta2 crosses +-pi
    (0.3, -0.2, 4 * PI, 9 * PI), (0.3, -0.2, -4 * PI, -9 * PI),              # velocities at the bounds
    (1.0, 2.0, 4 * PI + 1.0, 9 * PI + 2.0), (-1.0, -2.0, -4 * PI - 1.0, -9 * PI - 2.0),      # and beyond them
    # stepped from (t1, 0.1, 0.5, 0) the terminal line is crossed at t1 = 2.0168 / 2.0139 / 2.0112 under actions 0 / 1 / 2
    (2.0111, 0.1, 0.5, 0.0), (2.0169, 0.1, 0.5, 0.0),
]


def test_acrobot_steps_equal_the_restatement(rlx, dev):
    cases = [(s, a) for s in ACROBOT_STATES for a in (0, 1, 2)]
    env = _env(dev, "Acrobot", len(cases))
    ns, reward, obs = _step_from(env, [c[0] for c in cases], np.array([c[1] for c in cases], dtype=np.int32))
    ref = [acrobot_ref(list(s), a) for s, a in cases]
    np.testing.assert_allclose(ns, np.array([r[0] for r in ref]), rtol=0, atol=1e-12)
    terminal = np.array([r[2] for r in ref])
    assert terminal[-3:].all() and not terminal[-6:-3].any() and not terminal[:3].any()
    assert np.array_equal(reward, -1.0 + terminal) and np.array_equal(env.game_over.cpu().numpy() != 0, terminal)
    s, c, status = _sincos(rlx.libm_sincos_full, dev, ns[:, :2].T.copy())    # fp32 outputs: its own fp64, rounded
    assert np.array_equal(obs, np.stack([c[0], s[0], c[1], s[1], ns[:, 2], ns[:, 3]], axis=1).astype(F32))
    assert status == 0 and int(env.status.item()) == 0
    state, steps = env.state.cpu().numpy(), env.step_in_episode.cpu().numpy()
    assert np.array_equal(steps, ~terminal) and np.array_equal(env.episode.cpu().numpy(), terminal)
    assert np.array_equal(state[~terminal], ns[~terminal]) and (np.abs(state[terminal]) <= 0.1).all()
    assert np.array_equal(env.reset_obs.cpu().numpy()[terminal][:, 4:], state[terminal][:, 2:].astype(F32))


def test_a_bad_action_sets_status_bit_1_and_leaves_the_state(dev):
    env = _env(dev, "Acrobot", 3)
    states = np.array([ACROBOT_STATES[3], ACROBOT_STATES[4], ACROBOT_STATES[0]])        # none of them terminal
    ns, reward, _ = _step_from(env, states, np.array([3, -1, 2], dtype=np.int32))
    assert int(env.status.item()) == 2 and np.array_equal(ns[:2], states[:2]) and (env.step_in_episode == 1).all()
    assert np.abs(ns[2] - acrobot_ref(list(states[2]), 2)[0]).max() <= 1e-12 and reward.tolist() == [0.0, 0.0, -1.0]
    with pytest.raises(RuntimeError, match="outside"):
        env.check_status()


@pytest.mark.parametrize("kind,limit", [("Pendulum", 200), ("Acrobot", 500)])
def test_time_limit_and_resets(dev, kind, limit):
    """the TimeLimit; reset draws: in their intervals, a function of (seed, env id, episode) alone, forced or not"""
    import torch
    env, one = _env(dev, kind, 4, seed=77), _env(dev, kind, 1, seed=77)
    first = env.state.cpu().numpy()
    assert np.array_equal(first[0], one.state.cpu().numpy()[0]) and len({tuple(r) for r in first}) == 4
    high = np.array([PI, 1.0]) if kind == "Pendulum" else np.full(4, 0.1)
    assert env.p.episode_length == limit and (np.abs(first) <= high).all()
    actions = torch.zeros((4, 1), dtype=torch.float32, device=dev) if kind == "Pendulum" else \
        torch.ones(4, dtype=torch.int32, device=dev)
    env.state.zero_()                                                        # hanging at rest: nothing terminal
    env.step_in_episode.fill_(limit - 2)
    env.step(actions)
    assert not env.dones_host.any() and (env.step_in_episode == limit - 1).all() and (env.episode == 0).all()
    env.state.zero_()
    env.step(actions)
    second = env.state.cpu().numpy()
    assert env.dones_host.all() and not env.step_in_episode.any() and (env.episode == 1).all() and not env.status.any()
    assert (np.abs(second) <= high).all() and not np.array_equal(second, first)
    assert np.array_equal(env.reset_obs.cpu().numpy()[:, -1], second[:, -1].astype(F32))
    one.reset_internal_state()                                               # forced: episode 1 of env 0, the same draw
    assert int(one.episode.item()) == 1 and np.array_equal(one.state.cpu().numpy()[0], second[0])


@pytest.mark.parametrize("level", ["Pendulum-v0", "Acrobot-v1"])
def test_an_agent_acts_and_trains_on_the_level(dev, level):
    from coach_amd.agents.ddpg_agent import DDPGAgentParameters
    from coach_amd.agents.dqn_agent import DQNAgentParameters
    from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps
    from coach_amd.environments.gym_environment import GymVectorEnvironment
    from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters
    sched = ScheduleParameters()
    sched.heatup_steps, sched.improve_steps = EnvironmentSteps(96), EnvironmentSteps(48)
    sched.steps_between_evaluation_periods, sched.evaluation_steps = EnvironmentSteps(48), EnvironmentEpisodes(1)
    for synthetic in (True, False):
        env = GymVectorEnvironment(level=level)
        env.episode_length = 24
        if synthetic:
            env.register_var("synthetic", True)                              # the switch the CartPole levels have
        agent = DDPGAgentParameters() if level == "Pendulum-v0" else DQNAgentParameters()
        gm = BasicRLGraphManager(agent, env, sched, device=dev).create_graph()
        assert type(gm.environment).__name__ == ("Synthetic" if synthetic else level[:-3]) + "VectorEnvironment"
    gm.improve()                                                             # on the real level: the last one built
    assert gm.agent.training_iteration > 0 and gm.environment.p.action_dim == (1 if level == "Pendulum-v0" else None)
    gm.agent.check_status(), gm.environment.check_status()


def test_the_acrobot_batch_rl_preset_builds_its_agents(dev):
    from coach_amd.presets.Acrobot_DDQN_BCQ_BatchRL import make
    gm = make(dataset_size=2000, heatup_steps=200)
    gm.device = dev
    gm.create_graph()
    assert type(gm.environment).__name__ == "AcrobotVectorEnvironment"
    assert [type(a).__name__ for a in (gm.trained_agent, gm.experience_generating_agent)] == ["DDQNBCQAgent", "DDQNAgent"]
    for net in (gm.trained_agent.networks["main"], gm.experience_generating_agent.networks["main"]):
        for buf in (net.params.weights, net.target):                         # the Q head's output bias: constant -100
            assert net.params.w(net.q_head.bname, 0, buf).tolist() == [-100.0] * 3
