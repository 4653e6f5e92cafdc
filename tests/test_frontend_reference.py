"""The Atari front end pinned to the reference's own code.  tests/golden/frontend.npz holds traces of the reference's
GymEnvironment (MaxOverFramesAndFrameskipEnvWrapper, life handling, random no-op starts, FIRE; made by tests/golden/
make_golden_frontend.py over FakeAtariEmulator, with gym's Wrapper / TimeLimit restated: gym and ALE themselves stay
unpinned).  Against it:
  * oracle.frontend.FrontEndOracle (CPU) — every frame, reward, done flag, reset frame, emulator position, host draw;
  * the front end's host half, _Game (CPU) — the same, with the maximum over its kept frames taken in numpy;
  * EmulatorVectorEnvironment (GPU) — the device chain max -> rescale -> luminance -> uint8 on the fixture's frames,
    rewards and done flags; reads only the .npz;
  * where the reference tree is present: the live reference against FrontEndOracle for 300 steps per configuration."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import frontend_ref as FR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_FIX = np.load(os.path.join(GOLDEN, "frontend.npz"))
CONFIGS = json.loads(str(_FIX["configs"]))
KEYS = ("actions", "first_frame", "first_pos", "frame", "reward", "done", "pos", "reset_frame", "reset_pos", "n_draws")


def _trace(c):
    return {k: _FIX["c%d_%s" % (c, k)] for k in KEYS}


_IDS = [cfg["name"] for cfg in CONFIGS]


def test_the_fixture_covers_what_it_must():
    """the configurations between them: both phases, the preset's skip 4 / max 2, skip 3 / max 3, max over 1, 30 and 0
    random no-op steps, an emulator without FIRE, a time limit that is no multiple of the skip, one larger frame."""
    def has(**kw):
        return any(all(cfg[k] == v for k, v in kw.items()) for cfg in CONFIGS)
    assert has(train=True) and has(train=False)
    assert has(frame_skip=4, max_over=2, ris=30) and has(frame_skip=3, max_over=3) and has(max_over=1)
    assert has(ris=0) and any(cfg["meanings"] and cfg["meanings"][1] != "FIRE" for cfg in CONFIGS)
    assert any(cfg["max_episode_steps"] % cfg["frame_skip"] for cfg in CONFIGS)
    assert sorted(tuple(cfg["shape"]) for cfg in CONFIGS)[-1] == (12, 16, 3)
    for c, cfg in enumerate(CONFIGS):
        t = _trace(c)
        assert t["frame"].shape == (cfg["steps"], FR.N_ENV) + tuple(cfg["shape"])
        assert t["done"].sum() == len(t["reset_frame"]) > 0
        assert (t["reset_pos"][:, 0] > 0).any()                       # a real emulator reset


@pytest.mark.parametrize("c", range(len(CONFIGS)), ids=_IDS)
def test_oracle_reproduces_the_reference_trace(c):
    cfg, want = CONFIGS[c], _trace(c)
    got = FR.oracle_trace(cfg, want["actions"])
    after = random.getstate()
    FR.compare_traces(got, want, cfg["name"])
    assert after == FR.replay_draws(cfg, int(want["n_draws"]))       # the same host draws, nothing more


def _host_half_trace(cfg, actions):
    """the front end's _Game objects driven like EmulatorVectorEnvironment drives them, the maximum in numpy"""
    from coach_amd.environments.emulator_frontend import EmulatorEnvironmentParameters, _Game
    emus = FR.emulators(cfg)
    p = EmulatorEnvironmentParameters(emus, 4, raw_shape=tuple(cfg["shape"]), **FR.front_end_kwargs(cfg))
    games = [_Game(e, p) for e in emus]
    kept = np.zeros((2, FR.N_ENV, cfg["max_over"]) + tuple(cfg["shape"]), np.uint8)
    out = dict(frame=[], reward=[], done=[], pos=[], reset_frame=[], reset_pos=[])
    calls, restore = FR.count_draws()
    try:
        random.seed(cfg["host_seed"])
        for e, g in enumerate(games):
            g.reset(kept[0, e], cfg["train"], True)
        out["first_frame"] = kept[0].max(axis=1)
        out["first_pos"] = np.array([(m.episode, m.t) for m in emus], np.int32)
        for a in actions:
            row = dict(reward=[], done=[], pos=[])
            for e, g in enumerate(games):
                g.step(int(a[e]), kept[0, e], cfg["train"])
                row["reward"].append(g.reward); row["done"].append(bool(g.done))
                row["pos"].append((emus[e].episode, emus[e].t))
                frame = kept[0, e].max(axis=0)
                if g.done:
                    g.reset(kept[1, e], cfg["train"], False)
                    out["reset_frame"].append(kept[1, e].max(axis=0))
                    out["reset_pos"].append((emus[e].episode, emus[e].t))
                row.setdefault("frame", []).append(frame)
            for k, v in row.items():
                out[k].append(v)
    finally:
        restore()
    out = {k: np.asarray(v) for k, v in out.items()}
    out["reset_frame"] = out["reset_frame"].reshape((-1,) + tuple(cfg["shape"]))
    out["reset_pos"] = out["reset_pos"].reshape(-1, 2)
    out["n_draws"] = np.array(calls[0])
    return out


@pytest.mark.parametrize("c", range(len(CONFIGS)), ids=_IDS)
def test_front_end_host_half_reproduces_the_reference_trace(c):
    cfg, want = CONFIGS[c], _trace(c)
    got = _host_half_trace(cfg, want["actions"])
    after = random.getstate()
    FR.compare_traces(got, want, cfg["name"])
    assert after == FR.replay_draws(cfg, int(want["n_draws"]))


@pytest.mark.reference
def test_live_reference_against_the_oracle_for_300_steps():
    """a process of its own: the stub-import harness replaces gym, tensorflow, ... for everything imported after it"""
    res = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_frontend.py"), "--live", "300"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    assert res.stdout.count("FrontEndOracle equals the reference") == len(CONFIGS), res.stdout[-4000:]


@pytest.mark.gpu
@pytest.mark.parametrize("c", range(len(CONFIGS)), ids=_IDS)
def test_device_front_end_reproduces_the_reference_trace(dev, c):
    import torch
    from coach_amd.core_types import RunPhase
    from coach_amd.environments.emulator_frontend import EmulatorEnvironmentParameters, EmulatorVectorEnvironment
    from oracle import filters as F
    cfg, want = CONFIGS[c], _trace(c)
    shape = tuple(cfg["shape"])
    out_hw = (6, 5) if shape == (4, 4, 3) else (7, 9)              # up-scale the small frames, down-scale the large
    p = EmulatorEnvironmentParameters(FR.emulators(cfg), 4, raw_shape=shape, observation_shape=out_hw,
                                      **FR.front_end_kwargs(cfg))
    env = EmulatorVectorEnvironment(p, dev)
    env.phase = RunPhase.TRAIN if cfg["train"] else RunPhase.TEST

    def chain(frames):                                             # the reference's Atari input filter, frame by frame
        return np.array([F.to_uint8(F.rgb_to_y(F.resize_bilinear_u8(f, out_hw)), 0, 255) for f in frames])

    want_next = chain(want["frame"].reshape((-1,) + shape)).reshape(want["frame"].shape[:2] + out_hw)
    want_reset = chain(want["reset_frame"])
    random.seed(cfg["host_seed"])
    first = env.reset_internal_state(True).cpu().numpy()
    assert np.array_equal(first, chain(want["first_frame"]))
    d = 0
    for t, a in enumerate(want["actions"]):
        nxt, rst, rew, done = env.step(torch.from_numpy(a.astype(np.int32)).to(dev))
        nxt, rst, rew, done = nxt.cpu().numpy(), rst.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        assert np.array_equal(done.astype(bool), want["done"][t]), (t, want["pos"][t].tolist())
        assert np.array_equal(env.dones_host, want["done"][t])
        assert np.array_equal(rew, want["reward"][t].astype(np.float32)), (t, want["pos"][t].tolist())
        assert np.array_equal(nxt, want_next[t]), (t, want["pos"][t].tolist())
        for e in np.flatnonzero(want["done"][t]):
            assert np.array_equal(rst[e], want_reset[d]), (t, e, want["reset_pos"][d].tolist())
            d += 1
    assert d == len(want_reset)
    assert random.getstate() == FR.replay_draws(cfg, int(want["n_draws"]))
