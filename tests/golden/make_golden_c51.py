#!/usr/bin/env python
"""Generate tests/golden/c51.npz by running the REFERENCE's own CategoricalDQNAgent code under the stub-import harness
(_refstub.py), in the manner of make_golden_qr_dqn.py.  Run from the repo root in the build container (the reference
tree must be present):

    python tests/golden/make_golden_c51.py

Recorded:
  * learn_from_batch with stand-in networks: parallel_prediction returns fixed fp32 softmaxes, train_and_sync_networks
    records its targets (the projected distribution m in the taken action's row, the online softmax elsewhere) — four
    cases, one of them with the support [0, 200] and all rewards 1; ~30 % game-overs.  The device sums an action's
    expectation in atom order while numpy's dot may not: a row whose two largest target-network Q values are closer
    than 1e-6 is redrawn, so that the target action does not depend on the order;
  * distribution_prediction_to_q_values on a few acting inputs (two of them with exactly tied actions);
  * the parameter classes' defaults (JSON text under "defaults").
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstub  # noqa: E402

_refstub.install()

from rl_coach.core_types import Batch, Transition  # noqa: E402

# (B, A, N, v_min, v_max, all rewards one)
CASES = ((32, 2, 51, -10.0, 10.0, False), (37, 6, 51, -10.0, 10.0, False), (5, 18, 2, 0.0, 1.0, False),
         (32, 2, 51, 0.0, 200.0, True))
MIN_GAP = 1e-6


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _softmax32(rng, shape):
    """fixed fp32 distributions of varying sharpness, as a network's softmax output would be."""
    x = (rng.randn(*shape) * rng.uniform(0.5, 3.0, size=shape[:-1] + (1,))).astype(np.float32)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def _fake_agent(N, v_min, v_max, discount=0.99):
    from rl_coach.agents.categorical_dqn_agent import CategoricalDQNAgent

    class Fake(CategoricalDQNAgent):
        def __init__(self):
            pass
    f = Fake()
    wrapper = _Obj(input_embedders_parameters={'observation': None})
    f.ap = _Obj(network_wrappers={'main': wrapper},
                algorithm=_Obj(discount=discount, atoms=N, v_min=v_min, v_max=v_max))
    f.z_values = np.linspace(v_min, v_max, N)                # categorical_dqn_agent.py:78
    f.q_values = _Obj(add_sample=lambda v: None)
    f.memory = object()                                      # not a PrioritizedExperienceReplay
    return f


def gen_learn(out, rng):
    for s, (B, A, N, v_min, v_max, ones) in enumerate(CASES):
        f = _fake_agent(N, v_min, v_max)
        p_next = _softmax32(rng, (B, A, N))
        redrawn = 0
        while True:                                          # the condition on the inputs (see the module text)
            q = np.sort(f.distribution_prediction_to_q_values(p_next), axis=1)
            close = (q[:, -1] - q[:, -2]) < MIN_GAP
            if not close.any():
                break
            p_next[close] = _softmax32(rng, (int(close.sum()), A, N))
            redrawn += int(close.sum())
        p_online = _softmax32(rng, (B, A, N))
        actions = rng.randint(0, A, size=B)
        rewards = np.ones(B, np.float32) if ones else rng.randn(B).astype(np.float32)   # fp32-exact: the replay's type
        go = rng.rand(B) < 0.3
        captured = {}
        main = _Obj(target_network=object(), online_network=object(),
                    parallel_prediction=lambda pairs: (p_next.copy(), p_online.copy()))

        def train(inputs, targets, importance_weights=None):
            captured['targets'] = np.array(targets)
            captured['importance_weights'] = importance_weights
            return 0.0, [np.zeros((B, A))], 0.0
        main.train_and_sync_networks = train
        f.networks = {'main': main}
        tr = [Transition(state={'observation': rng.randn(4)}, action=int(actions[i]), reward=float(rewards[i]),
                         next_state={'observation': rng.randn(4)}, game_over=bool(go[i])) for i in range(B)]
        f.learn_from_batch(Batch(tr))
        assert captured['targets'].dtype == np.float32 and captured['importance_weights'] is None
        q = np.sort(f.distribution_prediction_to_q_values(p_next), axis=1)
        p = "s%d_" % s
        out[p + "p_next"], out[p + "p_online"], out[p + "z"] = p_next, p_online, f.z_values
        out[p + "actions"], out[p + "rewards"], out[p + "go"] = actions, rewards, go
        out[p + "targets"] = captured['targets']                          # fp32 [B, A, N]
        out[p + "discount"] = np.float64(0.99)
        sums = captured['targets'][np.arange(B), actions].sum(axis=1)
        print("case %d %s: %d rows redrawn, min Q gap %.3g, %d of %d projected rows sum to < 0.999 (min %.3f)" % (
            s, (B, A, N), redrawn, (q[:, -1] - q[:, -2]).min(), int((sums < 0.999).sum()), B, sums.min()))


def gen_acting(out, rng):
    for s, (n, A, N, v_min, v_max) in enumerate(((4, 2, 51, -10.0, 10.0), (3, 6, 51, -10.0, 10.0),
                                                 (2, 18, 2, 0.0, 1.0))):
        f = _fake_agent(N, v_min, v_max)
        x = _softmax32(rng, (n, A, N))
        x[0, 1] = x[0, 0][::-1]           # the mirrored distribution: the opposite expectation on a symmetric support
        x[-1, A - 1] = x[-1, 0]           # identical distributions: an exact tie
        out["act%d_p" % s], out["act%d_z" % s] = x, f.z_values
        out["act%d_q" % s] = f.distribution_prediction_to_q_values(x)


def gen_defaults(out):
    from rl_coach.agents.categorical_dqn_agent import CategoricalDQNAgentParameters
    ap = CategoricalDQNAgentParameters()
    net = ap.network_wrappers['main']
    sch = ap.exploration.epsilon_schedule
    d = {"atoms": ap.algorithm.atoms, "v_min": ap.algorithm.v_min, "v_max": ap.algorithm.v_max,
         "discount": ap.algorithm.discount, "learning_rate": net.learning_rate,
         "optimizer_epsilon": net.optimizer_epsilon, "batch_size": net.batch_size,
         "head": type(net.heads_parameters[0]).__name__,
         "classes": [type(ap.algorithm).__name__, type(ap.exploration).__name__, type(net).__name__],
         "epsilon_schedule": [type(sch).__name__, float(sch.initial_value), float(sch.final_value),
                              int(sch.decay_steps)],
         "evaluation_epsilon": ap.exploration.evaluation_epsilon,
         "num_steps_between_copying_online_weights_to_target":
             ap.algorithm.num_steps_between_copying_online_weights_to_target.num_steps,
         "num_consecutive_playing_steps": ap.algorithm.num_consecutive_playing_steps.num_steps,
         "memory": type(ap.memory).__name__}
    out["defaults"] = np.array(json.dumps(d, sort_keys=True))


def main():
    rng = np.random.RandomState(51)
    out = {}
    gen_learn(out, rng)
    gen_acting(out, rng)
    gen_defaults(out)
    path = os.path.join(HERE, "c51.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KiB)" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
