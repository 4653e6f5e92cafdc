#!/usr/bin/env python
"""Generate tests/golden/bit_flip.npz by stepping the REFERENCE's own BitFlip class
(rl_coach/environments/toy_problems/bit_flip.py) under the stub-import harness (_refstub.py: gym is absent, the class
body does not need it), in the manner of make_golden_c51.py.  Run from the repo root in the build container:

    python tests/golden/make_golden_bit_flip.py

The class draws its start with Python's `random`; here the start state and goal are IMPOSED after construction and a
recorded action list is stepped until the class reports done.  Cases: L in {1, 8, 20} x mean_zero in {False, True} x
  early   the goal is reached after 2 steps (1 step at L = 1)
  last    state = ~goal and every bit is flipped once: reached at the last allowed step (max_steps = L)
  never   one bit is flipped back and forth until the limit (impossible at L = 1: any flip reaches the goal)
plus, at L = 8, a custom max_steps of 5 (timeout) and of 12 (reached at step 12 after wasted flips).
Recorded per case c (keys `c<c>_<name>`): state0, goal0, actions, and per step the emitted 'state', 'desired_goal' and
'achieved_goal' arrays, the reward and done.  `cases` is the JSON text of the case table.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstub  # noqa: E402

_refstub.install()

from rl_coach.environments.toy_problems.bit_flip import BitFlip  # noqa: E402


def case_table():
    rng = np.random.RandomState(5)
    cases = []
    for L in (1, 8, 20):
        for mean_zero in (False, True):
            goal = rng.randint(0, 2, size=L)
            kinds = ["early", "last"] + (["never"] if L > 1 else [])
            for kind in kinds:
                if kind == "early":
                    diff = [0] if L == 1 else [1, L - 1]
                    state = goal.copy()
                    state[diff] ^= 1
                    actions = diff
                elif kind == "last":
                    state, actions = 1 - goal, list(rng.permutation(L))
                else:
                    state = goal.copy()
                    state[0] ^= 1
                    actions = [L - 1] * L
                cases.append(dict(L=L, mean_zero=mean_zero, max_steps=None, kind=kind, state0=state.tolist(),
                                  goal0=goal.tolist(), actions=[int(a) for a in actions]))
    goal = rng.randint(0, 2, size=8)
    cases.append(dict(L=8, mean_zero=True, max_steps=5, kind="never", state0=(1 - goal).tolist(), goal0=goal.tolist(),
                      actions=[0, 1, 2, 3, 4]))
    cases.append(dict(L=8, mean_zero=False, max_steps=12, kind="last", state0=(1 - goal).tolist(), goal0=goal.tolist(),
                      actions=[3, 3, 3, 3, 0, 1, 2, 3, 4, 5, 6, 7]))
    return cases


def main():
    out = {}
    cases = case_table()
    for c, case in enumerate(cases):
        env = BitFlip(bit_length=case["L"], max_steps=case["max_steps"], mean_zero=case["mean_zero"])
        env.state, env.goal, env.steps = np.array(case["state0"]), np.array(case["goal0"]), 0
        rec = {"state": [], "desired_goal": [], "achieved_goal": [], "reward": [], "done": []}
        for a in case["actions"]:
            obs, reward, done, _ = env.step(a)
            for k in ("state", "desired_goal", "achieved_goal"):
                rec[k].append(np.array(obs[k], dtype=np.float64))
            rec["reward"].append(float(reward))
            rec["done"].append(bool(done))
            if done:
                break
        assert rec["done"][-1] and len(rec["done"]) == len(case["actions"]), case
        assert (rec["reward"][-1] == 0) == (case["kind"] != "never"), case
        p = "c%d_" % c
        for k, v in rec.items():
            out[p + k] = np.array(v)
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "bit_flip.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d cases, %d bytes)" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
