#!/usr/bin/env python
"""Generate tests/golden/ucb_chain.npz by running the REFERENCE's own UCB policy, PieceWiseSchedule and ExplorationChain
class under the stub-import harness (_refstub.py), in the manner of make_golden_bootstrapped_dqn.py.  Run from the repo
root in the build container (the reference tree must be present):

    python tests/golden/make_golden_ucb_chain.py

Recorded:
  * UCB.get_action in TRAIN and TEST for K in {1, 2, 20} x A in {2, 18} x lamb in {0.1, 10}, five envs each: env 0 random
    values, env 1 every head and action equal (the tie-break draw decides), env 2 actions 0 and A - 1 exactly tied in
    every head and above the rest, env 3 values of the order 1e3, env 4 explores (its values and std stay 0: the policy computes none).  The heads' values go in as the agent
    passes them, a list of K (1, A) fp32 arrays; np.random is seeded before every call and the seed stored, so the draws
    can be made again.  Stored as the policy left them: last_action_values and std (fp32), the chosen action;
  * a PieceWiseSchedule of three short linear pieces stepped across both switches (its current_value after every step,
    the index of the current piece and its step count);
  * ExplorationChain trajectories (observation, reward, done per step, two episodes each with a reset in between): both
    observation types x chain_length in {4, 20} x start_state in {0, 1, L - 1}, action lists that walk into both walls,
    rewards that fp32 does not hold exactly, and max_steps = 1.  `chain_cases` is the JSON text of the case table.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstub  # noqa: E402

_refstub.install()

from rl_coach.core_types import EnvironmentSteps, RunPhase  # noqa: E402

UCB_CASES = [(K, A, lamb) for K in (1, 2, 20) for A in (2, 18) for lamb in (0.1, 10)]
N_ENV = 5


def gen_ucb(out, rng):
    from rl_coach.exploration_policies.ucb import UCB
    from rl_coach.schedules import ConstantSchedule
    from rl_coach.spaces import DiscreteActionSpace
    for s, (K, A, lamb) in enumerate(UCB_CASES):
        q = (rng.randn(N_ENV, K, A) * 2.0).astype(np.float32)
        q[1] = 0.25
        q[2] *= np.float32(0.01)          # (the other actions' uncertainty bonus stays below the tied pair's at lamb = 10)
        top = np.abs(q[2]).max() + 1.0
        q[2, :, 0] = q[2, :, A - 1] = (top + rng.rand(K)).astype(np.float32)
        q[3] = (rng.randn(K, A) * 1e3).astype(np.float32)
        u = np.ones(N_ENV)
        u[N_ENV - 1] = -1.0
        for phase, name in ((RunPhase.TRAIN, "train"), (RunPhase.TEST, "test")):
            acts = np.zeros(N_ENV, np.int64)
            vals, stds = np.zeros((N_ENV, A), np.float32), np.zeros((N_ENV, A), np.float32)
            for e in range(N_ENV):
                np.random.seed(3000 + 100 * s + e)
                pol = UCB(DiscreteActionSpace(A), ConstantSchedule(0.5), 0.5, K, lamb)
                pol.phase = phase
                pol.current_random_value = float(u[e])
                np.random.seed(9000 + 100 * s + e)
                a, _ = pol.get_action([q[e, h][None] for h in range(K)])
                acts[e] = a
                if u[e] < 0.5:          # an exploring call computes no values (requires_action_values, ucb.py:79)
                    assert pol.last_action_values == 0 and pol.std == 0
                    continue
                v = np.asarray(pol.last_action_values)
                assert v.dtype == np.float32 and v.shape == (1, A), (v.dtype, v.shape)
                vals[e] = v[0]
                if phase == RunPhase.TRAIN:
                    sd = np.asarray(pol.std)
                    assert sd.dtype == np.float32 and sd.shape == (1, A)
                    stds[e] = sd[0]
                    assert pol.get_control_param() == np.mean(sd)
                else:
                    assert pol.std == 0 and pol.get_control_param() == 0
            out["ucb%d_%s_actions" % (s, name)], out["ucb%d_%s_values" % (s, name)] = acts, vals
            if name == "train":
                out["ucb%d_train_std" % s] = stds
        out["ucb%d_q" % s], out["ucb%d_u" % s], out["ucb%d_seed0" % s] = q, u, np.int64(9000 + 100 * s)
    out["ucb_cases"] = np.array(json.dumps(UCB_CASES))
    # select_head draws nothing
    np.random.seed(5)
    pol = UCB(DiscreteActionSpace(3), ConstantSchedule(0.5), 0.5, 10, 0.1)
    before = np.random.get_state()
    pol.select_head()
    assert np.array_equal(before[1], np.random.get_state()[1]) and before[2] == np.random.get_state()[2]


PIECES = ((1.0, 0.5, 4, 3), (0.5, 0.1, 5, 4), (0.1, 0.0, 2, 2))       # (initial, final, decay_steps, EnvironmentSteps)


def gen_schedule(out):
    from rl_coach.schedules import LinearSchedule, PieceWiseSchedule
    sch = PieceWiseSchedule([(LinearSchedule(a, b, n), EnvironmentSteps(m)) for a, b, n, m in PIECES])
    trace = [(float(sch.current_value), sch.current_schedule_idx, sch.current_schedule_step_count)]
    for _ in range(16):
        sch.step()
        trace.append((float(sch.current_value), sch.current_schedule_idx, sch.current_schedule_step_count))
    assert [t[1] for t in trace].count(1) > 2 and trace[-1][1] == 2
    out["schedule_pieces"] = np.array(PIECES, dtype=np.float64)
    out["schedule_values"] = np.array([t[0] for t in trace], dtype=np.float64)
    out["schedule_idx"] = np.array([t[1] for t in trace], dtype=np.int64)
    out["schedule_count"] = np.array([t[2] for t in trace], dtype=np.int64)


def chain_cases():
    cases = []
    for therm in (True, False):
        for L in (4, 20):
            for start in (0, 1, L - 1):
                if L == 4:
                    actions = [0, 0, 1, 1, 1, 1, 1, 0, 1]
                else:
                    actions = [0, 0, 0] + [1] * 22 + [0, 0]
                cases.append(dict(L=L, start=start, therm=therm, max_steps=len(actions), left=1 / 1000, right=1,
                                  actions=actions))
    cases.append(dict(L=4, start=1, therm=True, max_steps=1, left=1 / 1000, right=1, actions=[0]))
    cases.append(dict(L=5, start=3, therm=False, max_steps=1, left=0.1, right=2.7, actions=[1]))
    cases.append(dict(L=6, start=2, therm=True, max_steps=7, left=0.1, right=-2.7, actions=[0, 0, 0, 1, 1, 1, 0]))
    return cases


def gen_chain(out):
    from rl_coach.environments.toy_problems.exploration_chain import ExplorationChain
    cases = chain_cases()
    for c, case in enumerate(cases):
        kind = ExplorationChain.ObservationType.Therm if case["therm"] else ExplorationChain.ObservationType.OneHot
        env = ExplorationChain(chain_length=case["L"], start_state=case["start"], max_steps=case["max_steps"],
                               observation_type=kind, left_state_reward=case["left"],
                               right_state_reward=case["right"])
        obs, reward, done, first = [], [], [], []
        for episode in range(2):
            first.append(np.array(env.reset(), dtype=np.float64))
            for a in case["actions"]:
                o, r, d, _ = env.step(a)
                obs.append(np.array(o, dtype=np.float64))
                reward.append(float(r))
                done.append(bool(d))
            assert done[-1] and not any(done[-len(case["actions"]):-1]), case
        p = "chain%d_" % c
        out[p + "first"], out[p + "obs"] = np.array(first), np.array(obs)
        out[p + "reward"], out[p + "done"] = np.array(reward, dtype=np.float64), np.array(done)
    out["chain_cases"] = np.array(json.dumps(cases))
    for bad in (dict(chain_length=3), dict(chain_length=4, start_state=4), dict(chain_length=4, start_state=-1)):
        try:
            ExplorationChain(max_steps=3, **bad)
        except ValueError:
            continue
        raise AssertionError("the reference accepted %r" % (bad,))


def main():
    rng = np.random.RandomState(2210)
    out = {}
    gen_ucb(out, rng)
    gen_schedule(out)
    gen_chain(out)
    path = os.path.join(HERE, "ucb_chain.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KiB)" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
