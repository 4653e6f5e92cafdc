#!/usr/bin/env python
"""Generate tests/golden/dfp.npz by running the REFERENCE's own DFPAgent code under the stub-import harness
(_refstub.py), in the manner of make_golden_c51.py.  Run from the repo root in the build container (the reference tree
must be present):

    python tests/golden/make_golden_dfp.py

Recorded:
  * DFPAgent._update_measurements_targets on episodes of T in {1, 2, 3, 5, 33, 40} transitions, S in {1, 3, 6} steps,
    M in {1, 2} measurements, both HandlingTargetsAfterEpisodeEnd modes, scale factors 1 and (0.5, 3); the measurements
    are doubles that fp32 cannot hold.  dfp_agent.py:236 compares the measurement array with [], which the installed
    numpy refuses for an ndarray: the arrays handed to the reference are a small ndarray subclass whose __eq__ answers
    False to an empty list;
  * DFPAgent.learn_from_batch with stand-in networks: predict returns a fixed fp32 prediction (the merge of two recorded
    stream outputs in the order csrc/dfp_merge.hpp states), train_and_sync_networks records its targets.  The future
    measurements come from the recorded NAN-mode episodes, so NaNs occur; every case has one row that is all NaN and one
    with none (B = 1: a row with none);
  * the action scores of DFPAgent.choose_action, recorded by driving it with a stand-in exploration policy that returns
    what it is given.  One row holds an exact tie of its two best actions.  numpy's dot may sum in another order than
    the device for M > 1: a row whose two best scores are closer than 1e-6 is redrawn (never dropped); the script asserts
    that at most one row in twenty needed it and prints the count;
  * the parameter classes' defaults (JSON text under "defaults").
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))       # tests/: the list of cases lives in dfp_ref.py
import _refstub  # noqa: E402

_refstub.install()

from rl_coach.core_types import Batch, Episode, Transition  # noqa: E402

from dfp_ref import (ACT_CASES, ACT_ROWS, ACT_STEPS, GOALS, LEARN_CASES, LENGTHS, MEAS, SCALES, STEPS,  # noqa: E402
                     WEIGHTS)

MIN_GAP = 1e-6


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Measurements(np.ndarray):
    """an ndarray that answers False when compared with an empty list (dfp_agent.py:236)."""

    def __eq__(self, other):
        if isinstance(other, list) and not other:
            return False
        return np.ndarray.__eq__(self, other)

    __hash__ = None


def _fake_agent(M, S, mode="NAN", scale=None, weights=None, goal=None, A=2):
    from rl_coach.agents.dfp_agent import DFPAgent, HandlingTargetsAfterEpisodeEnd

    class Fake(DFPAgent):
        def __init__(self):
            pass
    f = Fake()
    f.ap = _Obj(algorithm=_Obj(handling_targets_after_episode_end=HandlingTargetsAfterEpisodeEnd[mode],
                               num_predicted_steps_ahead=S, future_measurements_weights=weights),
                network_wrappers={'main': _Obj(input_embedders_parameters={'observation': None, 'measurements': None,
                                                                            'goal': None})})
    f.spaces = _Obj(state={'measurements': _Obj(shape=(M,))}, action=_Obj(actions=list(range(A))))
    f.target_measurements_scale_factors = None if scale is None else np.array(scale[:M])
    f.current_goal = goal
    return f


def _episode(meas):
    ep = Episode()
    T = len(meas)
    for i in range(T):
        ep.insert(Transition(state={'observation': np.zeros(4), 'measurements': meas[i].view(Measurements)}, action=0,
                             reward=0.0, next_state={'observation': np.zeros(4)}, game_over=i == T - 1))
    assert ep.length() == T
    return ep


def gen_targets(out, rng):
    n = 0
    for T in LENGTHS:
        for M in MEAS:
            # accumulated rewards look like this: a running sum of fp32-inexact doubles
            meas = np.cumsum(rng.uniform(-1.0, 2.0, size=(T, M)), axis=0) + rng.uniform(-1e-3, 1e-3, size=(T, M))
            assert not np.array_equal(meas, meas.astype(np.float32).astype(np.float64))
            out["fm_T%d_M%d_meas" % (T, M)] = meas
            for S in STEPS:
                for mode in ("NAN", "LastStep"):
                    for sname, scale in SCALES.items():
                        f = _fake_agent(M, S, mode, scale)
                        ep = _episode(meas)
                        f._update_measurements_targets(ep, S)
                        fm = np.stack([t.info['future_measurements'] for t in ep.transitions])
                        assert fm.shape == (T, S, M) and fm.dtype == np.float64
                        out["fm_T%d_M%d_S%d_%s_%s" % (T, M, S, mode, sname)] = fm
                        n += 1
    print("targets: %d cases" % n)


def merge32(E, X):
    """csrc/dfp_merge.hpp: the stand-in network's output (fp32, sum over the actions from 0.f in index order)."""
    B, A, K = X.shape
    s = np.zeros((B, K), np.float32)
    for a in range(A):
        s = s + X[:, a]
    mean = s / np.float32(A)
    return (E[:, None, :] + (X - mean[:, None, :])).astype(np.float32)


def gen_learn(out, rng):
    for c, (B, A, S, M) in enumerate(LEARN_CASES):
        K = S * M
        # future measurements: rows of the recorded NAN-mode episodes with this (S, M)
        pool = np.concatenate([out["fm_T%d_M%d_S%d_NAN_half3" % (T, M, S)] for T in LENGTHS])
        nans = np.isnan(pool).reshape(len(pool), -1)
        full, empty, some = np.where(~nans.any(1))[0], np.where(nans.all(1))[0], np.arange(len(pool))
        rows = list(rng.choice(some, size=B))
        rows[0] = int(rng.choice(full))                      # one row without a NaN ...
        if B > 1 and len(empty):
            rows[1] = int(rng.choice(empty))                 # ... and one that is all NaN (S = 1 has them only at T - 1)
        fm = pool[rows]                                      # fp64 [B, S, M]
        E = rng.randn(B, K).astype(np.float32)
        X = (rng.randn(B, A, K) * 2.0).astype(np.float32)
        y = merge32(E, X)
        actions = rng.randint(0, A, size=B)
        f = _fake_agent(M, S, A=A, goal=GOALS[M])
        captured = {}

        def train(inputs, targets):
            captured['targets'] = np.array(targets)
            captured['goal'] = np.array(inputs['goal'])
            return 0.0, [0.0], 0.0
        f.networks = {'main': _Obj(online_network=_Obj(predict=lambda inputs: y.copy()), train_and_sync_networks=train)}
        tr = [Transition(state={'observation': rng.randn(4), 'measurements': rng.randn(M)}, action=int(actions[i]),
                         reward=0.0, next_state={'observation': rng.randn(4)}, game_over=False,
                         info={'future_measurements': fm[i]}) for i in range(B)]
        f.learn_from_batch(Batch(tr))
        assert captured['targets'].dtype == np.float32 and captured['targets'].shape == (B, A, K)
        assert captured['goal'].shape == (B, M)
        p = "learn%d_" % c
        out[p + "E"], out[p + "X"], out[p + "y"], out[p + "actions"] = E, X, y, actions
        out[p + "future"], out[p + "targets"] = fm, captured['targets']
        t_nan = np.isnan(captured['targets'][np.arange(B), actions])
        print("learn case %d %s: %d NaN targets of %d, %d all-NaN rows, %d rows without" % (
            c, (B, A, S, M), int(t_nan.sum()), t_nan.size, int(t_nan.all(1).sum()), int((~t_nan.any(1)).sum())))


def _scores(f, y_row):
    """drive DFPAgent.choose_action for one state; the stand-in exploration policy hands back the action values."""
    got = {}

    def get_action(action_values):
        got['v'] = np.array(action_values)
        return 0, None
    f.exploration_policy = _Obj(requires_action_values=lambda: True, get_action=get_action)
    f.prepare_batch_for_inference = lambda state, name: {}
    f.networks = {'main': _Obj(online_network=_Obj(predict=lambda inputs: y_row[None].copy()))}
    f.choose_action({})
    assert got['v'].dtype == np.float64
    return got['v']


def gen_acting(out, rng):
    total = redrawn = 0
    for c, (A, M, W) in enumerate(ACT_CASES):
        S, K = ACT_STEPS, ACT_STEPS * M
        f = _fake_agent(M, S, weights=WEIGHTS[W], goal=GOALS[M], A=A)
        E = rng.randn(ACT_ROWS, K).astype(np.float32)
        X = (rng.randn(ACT_ROWS, A, K) * 2.0).astype(np.float32)
        v = np.zeros((ACT_ROWS, A))
        for r in range(ACT_ROWS):
            while True:
                if c == len(ACT_CASES) - 1 and r == 0:       # the exact tie: the first and the last action are the same
                    X[r, 0] = np.abs(X[r, 0]) + np.float32(8.0)          # stream, and the best by far
                    X[r, A - 1] = X[r, 0]
                v[r] = _scores(f, merge32(E[r:r + 1], X[r:r + 1])[0])
                top = np.sort(v[r])
                if c == len(ACT_CASES) - 1 and r == 0:
                    assert top[-1] == top[-2] == v[r, 0] == v[r, A - 1] and (A == 2 or top[-2] - top[-3] > 1.0)
                    break
                if top[-1] - top[-2] >= MIN_GAP:
                    break
                E[r], X[r] = rng.randn(K).astype(np.float32), (rng.randn(A, K) * 2.0).astype(np.float32)
                redrawn += 1
            total += 1
        p = "act%d_" % c
        out[p + "E"], out[p + "X"], out[p + "scores"] = E, X, v
        out[p + "goal"], out[p + "weights"] = np.array(GOALS[M]), np.array(WEIGHTS[W])
    assert redrawn * 20 <= total, (redrawn, total)
    print("acting: %d rows, %d redrawn" % (total, redrawn))


def gen_defaults(out):
    from rl_coach.agents.dfp_agent import DFPAgentParameters
    ap = DFPAgentParameters()
    net, alg = ap.network_wrappers['main'], ap.algorithm
    emb = net.input_embedders_parameters
    d = {"num_predicted_steps_ahead": alg.num_predicted_steps_ahead, "goal_vector": alg.goal_vector,
         "future_measurements_weights": alg.future_measurements_weights,
         "use_accumulated_reward_as_measurement": alg.use_accumulated_reward_as_measurement,
         "handling_targets_after_episode_end": alg.handling_targets_after_episode_end.name,
         "scale_measurements_targets": alg.scale_measurements_targets,
         "num_consecutive_playing_steps": alg.num_consecutive_playing_steps.num_steps,
         "batch_size": net.batch_size, "adam_optimizer_beta1": net.adam_optimizer_beta1,
         "async_training": net.async_training, "embedders": sorted(emb),
         "embedder_activations": {k: emb[k].activation_function for k in sorted(emb)},
         "embedder_schemes": {k: [type(l).__name__ for l in emb[k].scheme] for k in sorted(emb)},
         "middleware": [type(net.middleware_parameters).__name__, net.middleware_parameters.scheme.name,
                        net.middleware_parameters.activation_function],
         "head": [type(net.heads_parameters[0]).__name__, net.heads_parameters[0].activation_function],
         "memory": [type(ap.memory).__name__, ap.memory.max_size[0].name, ap.memory.max_size[1]],
         "shared_memory": ap.memory.shared_memory,
         "classes": [type(alg).__name__, type(ap.exploration).__name__, type(net).__name__]}
    out["defaults"] = np.array(json.dumps(d, sort_keys=True))


def main():
    rng = np.random.RandomState(2016)
    out = {}
    gen_targets(out, rng)
    gen_learn(out, rng)
    gen_acting(out, rng)
    gen_defaults(out)
    path = os.path.join(HERE, "dfp.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KiB)" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
