#!/usr/bin/env python
"""Generate tests/golden/her.npz by running the REFERENCE's own EpisodicHindsightExperienceReplay.store_episode on
fabricated episodes under the stub-import harness (_refstub.py), in the manner of make_golden_c51.py.  Run from the repo
root in the build container (the reference tree must be present):

    python tests/golden/make_golden_her.py

A case is one memory: k in {1, 4} x goal selection in {Final, Future, Episode} x (metric, threshold) in
{Euclidean, Manhattan} x {0, 0.5}; max_size = 10 (1 + k) transitions, so that whole extended episodes are evicted.
Episodes of T = 7, 1, 2, 7, 2, 1 transitions are stored one after the other (np.random.seed(1000 + case) first).
Observations are 5 values from {0, 0.5, 1} (every distance is exact in fp64 in any summation order) with the slice
table of the case: even cases [desired_goal (0, 2) | achieved (2, 4) | other (4, 5)], odd cases
[other (0, 1) | achieved (1, 3) | desired_goal (3, 5)]; odd cases also use the rewards (1.5, -0.25) instead of (0, -1).
Recorded per case c and store s (keys `c<c>_s<s>_<name>`): the memory's flat `transitions` list as columns (obs, next_obs,
action, reward, game_over), and `peek`: the value np.random.random() would return next (the stream is left untouched) —
it pins how much of the stream the store consumed.  `cases` is the JSON text of the case table.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstub  # noqa: E402

_refstub.install()

from rl_coach.core_types import Episode, Transition  # noqa: E402
from rl_coach.memories.episodic.episodic_hindsight_experience_replay import (  # noqa: E402
    EpisodicHindsightExperienceReplay, HindsightGoalSelectionMethod)
from rl_coach.memories.memory import MemoryGranularity  # noqa: E402
from rl_coach.spaces import GoalsSpace, ReachingGoal  # noqa: E402

EPISODE_LENGTHS = (7, 1, 2, 7, 2, 1)
D = 5
LAYOUTS = ({"desired_goal": (0, 2), "achieved": (2, 4), "other": (4, 5)},
           {"other": (0, 1), "achieved": (1, 3), "desired_goal": (3, 5)})


def case_table():
    cases = []
    for k in (1, 4):
        for method in ("Final", "Future", "Episode"):
            for metric in ("Euclidean", "Manhattan"):
                for threshold in (0.0, 0.5):
                    i = len(cases)
                    cases.append(dict(k=k, method=method, metric=metric, threshold=threshold, max_size=10 * (1 + k),
                                      layout=i % 2, rewards=[0.0, -1.0] if i % 2 == 0 else [1.5, -0.25]))
    return cases


def fabricate(rng, T):
    """one episode: obs, next_obs [T, D] fp32 from {0, .5, 1}, int actions, fp32-exact rewards, game_over on the last"""
    obs = (rng.randint(0, 3, size=(T, D)) * 0.5).astype(np.float32)
    nxt = (rng.randint(0, 3, size=(T, D)) * 0.5).astype(np.float32)
    act = rng.randint(0, 4, size=T).astype(np.int32)
    rew = (rng.randint(-4, 5, size=T) * 0.25).astype(np.float32)
    go = np.zeros(T, dtype=np.uint8)
    go[-1] = 1
    return obs, nxt, act, rew, go


def as_dict(vec, layout):
    return {name: vec[a:b].astype(np.float64) for name, (a, b) in layout.items()}


def as_vector(d, layout):
    v = np.zeros(D, dtype=np.float32)
    for name, (a, b) in layout.items():
        v[a:b] = d[name]
    return v


def columns(mem, layout):
    tr = mem.transitions
    return {"obs": np.array([as_vector(t.state, layout) for t in tr], dtype=np.float32).reshape(-1, D),
            "next_obs": np.array([as_vector(t.next_state, layout) for t in tr], dtype=np.float32).reshape(-1, D),
            "action": np.array([t.action for t in tr], dtype=np.int32),
            "reward": np.array([t.reward for t in tr], dtype=np.float32),
            "game_over": np.array([bool(t.game_over) for t in tr], dtype=np.uint8)}


def main():
    out = {}
    cases = case_table()
    for c, case in enumerate(cases):
        layout = LAYOUTS[case["layout"]]
        space = GoalsSpace(goal_name="achieved",
                           reward_type=ReachingGoal(distance_from_goal_threshold=case["threshold"],
                                                    goal_reaching_reward=case["rewards"][0],
                                                    default_reward=case["rewards"][1]),
                           distance_metric=GoalsSpace.DistanceMetric[case["metric"]])
        mem = EpisodicHindsightExperienceReplay((MemoryGranularity.Transitions, case["max_size"]), case["k"],
                                                HindsightGoalSelectionMethod[case["method"]], space)
        rng = np.random.RandomState(7000 + c)
        np.random.seed(1000 + c)
        for s, T in enumerate(EPISODE_LENGTHS):
            obs, nxt, act, rew, go = fabricate(rng, T)
            ep = Episode()
            for t in range(T):
                ep.insert(Transition(state=as_dict(obs[t], layout), action=int(act[t]), reward=float(rew[t]),
                                     next_state=as_dict(nxt[t], layout), game_over=bool(go[t])))
            mem.store_episode(ep)
            state = np.random.get_state()
            peek = np.random.random()
            np.random.set_state(state)
            p = "c%d_s%d_" % (c, s)
            for name, a in columns(mem, layout).items():
                out[p + name] = a
            out[p + "peek"] = np.float64(peek)
            out[p + "in_obs"], out[p + "in_next_obs"], out[p + "in_action"] = obs, nxt, act
            out[p + "in_reward"], out[p + "in_game_over"] = rew, go
            assert mem.num_transitions_in_complete_episodes() == len(mem.transitions) == mem.num_transitions()
    out["cases"] = np.array(json.dumps(cases))
    out["episode_lengths"] = np.array(EPISODE_LENGTHS, dtype=np.int32)
    out["layouts"] = np.array(json.dumps(LAYOUTS))
    path = os.path.join(HERE, "her.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d cases, %d bytes)" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
