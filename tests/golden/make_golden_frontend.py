#!/usr/bin/env python
"""Generate tests/golden/frontend.npz by running the REFERENCE's own Atari front end — GymEnvironment with its
MaxOverFramesAndFrameskipEnvWrapper, life handling, random no-op starts and FIRE presses (rl_coach/environments/
gym_environment.py, environment.py) — over FakeAtariEmulator, under the stub-import harness with the opt-in gym
stand-ins of _refstub.install_gym_front_end (a Wrapper, a TimeLimit, the space classes: ours; gym / ALE themselves stay
unpinned).  Run from the repo root in the build container (the reference tree must be present):

    python tests/golden/make_golden_frontend.py            # writes frontend.npz
    python tests/golden/make_golden_frontend.py --live 300 # reference against FrontEndOracle, 300 steps, writes nothing

Per configuration (CONFIGS below, stored as JSON under `configs`; tests/frontend_ref.py only builds the emulators and
counts the host draws — what steps them here is the reference): three reference environments over emulators of seed
0, 1, 2, built with seed=None (the constructor does not reseed `random`) and native rendering (no pygame window);
random.seed(host_seed) once, reset_internal_state(True) env by env, then a recorded action table, env 0..n-1 each step,
reset_internal_state(False) for an env right after the step that finished it — the order in which
EmulatorVectorEnvironment.step consumes host draws.  Recorded under `c<i>_`:
  actions [T,n]          first_frame [n,H,W,3], first_pos [n,2]   after the forced reset
  frame [T,n,H,W,3]      the maxed raw frame          reward, done [T,n]
  pos [T,n,2]            the emulator's (episode, t) after the step, to locate a mismatch
  reset_frame [D,H,W,3], reset_pos [D,2]              for the D (step, env) pairs with done, in trace order
  n_draws                calls of random.randint during the whole trace
Every configuration is one under which the reference terminates, and its trace must contain (asserted here) a real
emulator reset, a life-loss continuation (the reset steps the game instead of resetting it) and a frame skip that
stopped early with fewer than max_over_num_frames frames produced for the maximum (with max over 1: a `done` before
first_frame_to_max_over, where the last frame is kept).
"""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _refstub  # noqa: E402

FIRE = None                                   # FakeAtariEmulator's default meanings: action 1 is FIRE
NO_FIRE = ['NOOP', 'UP', 'RIGHT', 'LEFT']
SMALL = (4, 4, 3)                             # 48 bytes: the front end wants a multiple of 16

CONFIGS = [
    # the Atari preset's values: skip 4, max over 2, up to 30 no-op steps
    dict(name="train_preset", train=True, frame_skip=4, max_over=2, ris=30, max_episode_steps=400, shape=SMALL,
         steps=100, host_seed=10, meanings=FIRE, emu=dict(lives=3, life_every=97, game_len=600)),
    # TEST: a lost life presses FIRE instead of ending the episode; the game ends with a life left
    dict(name="test_preset", train=False, frame_skip=4, max_over=2, ris=30, max_episode_steps=400, shape=SMALL,
         steps=100, host_seed=11, meanings=FIRE, emu=dict(lives=3, life_every=61, game_len=150)),
    # first_frame_to_max_over = 0: every frame of a skip is kept
    dict(name="train_skip3_max3", train=True, frame_skip=3, max_over=3, ris=5, max_episode_steps=120, shape=SMALL,
         steps=100, host_seed=12, meanings=FIRE, emu=dict(lives=2, life_every=23, game_len=150)),
    dict(name="test_skip3_max3", train=False, frame_skip=3, max_over=3, ris=5, max_episode_steps=120, shape=SMALL,
         steps=100, host_seed=13, meanings=FIRE, emu=dict(lives=2, life_every=31, game_len=50)),
    # max over 1, no random no-ops
    dict(name="train_max1", train=True, frame_skip=4, max_over=1, ris=0, max_episode_steps=120, shape=SMALL,
         steps=100, host_seed=14, meanings=FIRE, emu=dict(lives=3, life_every=23, game_len=150)),
    # action 1 is not FIRE: nothing is pressed after a reset or a lost life
    dict(name="test_max1_no_fire", train=False, frame_skip=4, max_over=1, ris=5, max_episode_steps=120, shape=SMALL,
         steps=100, host_seed=15, meanings=NO_FIRE, emu=dict(lives=3, life_every=23, game_len=50)),
    # the time limit (not a multiple of the skip) ends episodes in the middle of a frame skip, with lives left
    dict(name="train_time_limit", train=True, frame_skip=4, max_over=2, ris=5, max_episode_steps=50, shape=SMALL,
         steps=100, host_seed=16, meanings=FIRE, emu=dict(lives=3, life_every=23, game_len=150), limit_mid_skip=True),
    # a larger frame, so that the device chain down-scales as well
    dict(name="test_12x16", train=False, frame_skip=4, max_over=2, ris=3, max_episode_steps=60, shape=(12, 16, 3),
         steps=40, host_seed=17, meanings=FIRE, emu=dict(lives=2, life_every=13, game_len=22)),
]


def actions_of(c, cfg, steps):
    n_actions = 4
    return np.random.RandomState(100 + c).randint(0, n_actions, size=(steps, 3)).astype(np.uint8)


def reference_trace(cfg, actions):
    """-> (arrays, events) from the reference's GymEnvironment."""
    from rl_coach.base_parameters import VisualizationParameters
    from rl_coach.core_types import RunPhase
    from rl_coach.environments.gym_environment import GymEnvironment

    import frontend_ref as FR
    emus = FR.emulators(cfg)
    envs, events = [], dict(real_resets=0, continuations=0, short_skips=0, rescued_skips=0, limit_mid_skip=0)
    for e, emu in enumerate(emus):
        level = "FakeAtari-%s-%d" % (cfg["name"], e)
        _refstub.register_level(level, emu, cfg["max_episode_steps"])
        env = GymEnvironment(level=level, frame_skip=cfg["frame_skip"], seed=None,
                             visualization_parameters=VisualizationParameters(native_rendering=True),
                             random_initialization_steps=cfg["ris"], max_over_num_frames=cfg["max_over"])
        assert env.is_atari_env and type(env.env).__name__ == "MaxOverFramesAndFrameskipEnvWrapper"
        env.phase = RunPhase.TRAIN if cfg["train"] else RunPhase.TEST
        _watch_skips(env, cfg, events)
        envs.append(env)

    def bare(env):
        return env.env.unwrapped

    calls, restore = FR.count_draws()
    try:
        random.seed(cfg["host_seed"])
        first = [env.reset_internal_state(True).next_state["observation"].copy() for env in envs]
        out = dict(first_frame=np.array(first), first_pos=np.array([(m.episode, m.t) for m in emus], np.int32),
                   frame=[], reward=[], done=[], pos=[], reset_frame=[], reset_pos=[])
        for a in actions:
            row = dict(frame=[], reward=[], done=[], pos=[])
            for e, env in enumerate(envs):
                resp = env.step(int(a[e]))
                row["frame"].append(resp.next_state["observation"].copy())
                row["reward"].append(float(resp.reward)); row["done"].append(bool(resp.game_over))
                row["pos"].append((emus[e].episode, emus[e].t))
                if resp.game_over:
                    out["reset_frame"].append(env.reset_internal_state(False).next_state["observation"].copy())
                    out["reset_pos"].append((emus[e].episode, emus[e].t))
            for k, v in row.items():
                out[k].append(v)
    finally:
        restore()
    events["real_resets"] = sum(bare(env).resets - 1 for env in envs)          # not the forced first one
    shape = tuple(cfg["shape"])
    out["frame"] = np.array(out["frame"], np.uint8)
    out["reward"] = np.array(out["reward"], np.float64)
    out["done"] = np.array(out["done"], bool)
    out["pos"] = np.array(out["pos"], np.int32)
    out["reset_frame"] = np.array(out["reset_frame"], np.uint8).reshape((-1,) + shape)
    out["reset_pos"] = np.array(out["reset_pos"], np.int32).reshape(-1, 2)
    out["n_draws"] = np.array(calls[0], np.int64)
    return out, events


def _watch_skips(env, cfg, events):
    """count, around the reference's own methods, the skips that stopped early and the resets that stepped the game on
    instead of resetting it (bookkeeping only: every call goes through to the reference unchanged)."""
    wrapper, limit, bare = env.env, env.env.env, env.env.unwrapped
    inner_step = wrapper.step
    first_kept = cfg["frame_skip"] - cfg["max_over"]

    def step(action):
        before, truncated = bare.steps, limit.truncations
        result = inner_step(action)
        taken = bare.steps - before
        if taken < cfg["frame_skip"]:
            assert result[2] and len(wrapper.observations_stack) == max(1, taken - first_kept) < max(2, cfg["max_over"])
            events["short_skips"] += 1
            events["rescued_skips"] += int(taken <= first_kept)
            events["limit_mid_skip"] += int(limit.truncations > truncated)
        return result
    wrapper.step = step

    # _restart_environment_episode either steps the game or resets it, then calls _random_noop: look there which it was
    restart, noop, entered = env._restart_environment_episode, env._random_noop, []

    def watched_restart(force_environment_reset=False):
        entered.append((bare.resets, bare.steps))
        return restart(force_environment_reset)

    def watched_noop():
        resets, steps = entered.pop()
        events["continuations"] += int(bare.resets == resets and bare.steps > steps)
        return noop()
    env._restart_environment_episode, env._random_noop = watched_restart, watched_noop


def check_events(cfg, events):
    assert events["real_resets"] >= 1 and events["continuations"] >= 1 and events["short_skips"] >= 1, (cfg["name"], events)
    if cfg["max_over"] == 1:
        assert events["rescued_skips"] >= 1, (cfg["name"], events)
    if cfg.get("limit_mid_skip"):
        assert events["limit_mid_skip"] >= 1, (cfg["name"], events)


def main():
    _refstub.install_gym_front_end()
    import frontend_ref as FR
    live = int(sys.argv[sys.argv.index("--live") + 1]) if "--live" in sys.argv else None
    out = {"configs": np.array(json.dumps(CONFIGS))}
    for c, cfg in enumerate(CONFIGS):
        actions = actions_of(c, cfg, live or cfg["steps"])
        ref, events = reference_trace(cfg, actions)
        check_events(cfg, events)
        if live:
            FR.compare_traces(FR.oracle_trace(cfg, actions), ref, cfg["name"])
            print("%-20s %d steps: FrontEndOracle equals the reference  %s" % (cfg["name"], live, events))
            continue
        print("%-20s %s  ends %d  draws %d" % (cfg["name"], events, int(ref["done"].sum()), int(ref["n_draws"])))
        out["c%d_actions" % c] = actions
        for k, v in ref.items():
            out["c%d_%s" % (c, k)] = v
    if live:
        return
    path = os.path.join(HERE, "frontend.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 300 * 1024, size
    print("wrote %s (%d configurations, %d bytes)" % (path, len(CONFIGS), size))


if __name__ == "__main__":
    main()
