"""Shared by tests/test_frontend_reference.py and tests/golden/make_golden_frontend.py: the configurations of
tests/golden/frontend.npz as data, and the driver that runs oracle.frontend.FrontEndOracle through one of them in the
order the reference trace was recorded (env 0..n-1 each step, an env's reset right after the step that finished it:
the order in which EmulatorVectorEnvironment.step consumes host draws)."""
import random

import numpy as np

from oracle.frontend import FrontEndOracle

N_ENV = 3


def emulators(cfg):
    from coach_amd.environments.emulator_frontend import FakeAtariEmulator
    return [FakeAtariEmulator(s, shape=tuple(cfg["shape"]), meanings=cfg["meanings"], **cfg["emu"])
            for s in range(N_ENV)]


def front_end_kwargs(cfg):
    return dict(frame_skip=cfg["frame_skip"], max_over_num_frames=cfg["max_over"],
                random_initialization_steps=cfg["ris"], max_episode_steps=cfg["max_episode_steps"])


def count_draws():
    """-> (counter list, restore()): counts the calls of random.randint, the front end's only host draw."""
    calls, orig = [0], random.randint

    def randint(a, b):
        calls[0] += 1
        return orig(a, b)
    random.randint = randint

    def restore():
        random.randint = orig
    return calls, restore


def replay_draws(cfg, n_draws):
    """the host generator's state after seeding like the trace and making `n_draws` no-op draws"""
    random.seed(cfg["host_seed"])
    for _ in range(n_draws):
        random.randint(0, cfg["ris"])
    return random.getstate()


def oracle_trace(cfg, actions):
    """-> the arrays of one configuration as make_golden_frontend.py records them, from FrontEndOracle."""
    emus = emulators(cfg)
    oracles = [FrontEndOracle(e, train=cfg["train"], **front_end_kwargs(cfg)) for e in emus]
    calls, restore = count_draws()
    try:
        random.seed(cfg["host_seed"])
        first = [o.reset(True).copy() for o in oracles]
        out = dict(first_frame=np.array(first), first_pos=np.array([(e.episode, e.t) for e in emus], np.int32),
                   frame=[], reward=[], done=[], pos=[], reset_frame=[], reset_pos=[])
        for a in actions:
            row = dict(frame=[], reward=[], done=[], pos=[])
            for e, o in enumerate(oracles):
                f, r, d = o.step(int(a[e]))
                row["frame"].append(f.copy()); row["reward"].append(float(r)); row["done"].append(bool(d))
                row["pos"].append((emus[e].episode, emus[e].t))
                if d:
                    out["reset_frame"].append(o.reset(False).copy())
                    out["reset_pos"].append((emus[e].episode, emus[e].t))
            for k, v in row.items():
                out[k].append(v)
    finally:
        restore()
    shape = tuple(cfg["shape"])
    out["frame"] = np.array(out["frame"], np.uint8)
    out["reward"] = np.array(out["reward"], np.float64)
    out["done"] = np.array(out["done"], bool)
    out["pos"] = np.array(out["pos"], np.int32)
    out["reset_frame"] = np.array(out["reset_frame"], np.uint8).reshape((-1,) + shape)
    out["reset_pos"] = np.array(out["reset_pos"], np.int32).reshape(-1, 2)
    out["n_draws"] = np.array(calls[0], np.int64)
    return out


def compare_traces(got, want, what):
    """every recorded array equal; the first difference is reported with its step, env and emulator position"""
    for k in ("first_frame", "first_pos", "pos", "done", "reward", "frame", "reset_pos", "reset_frame", "n_draws"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            where = tuple(int(x) for x in bad[:2])
            pos = want["pos"][where].tolist() if k in ("pos", "done", "reward", "frame") else None
            raise AssertionError("%s: %s differs first at %s (reference emulator (episode, t) there: %s)"
                                 % (what, k, where, pos))
