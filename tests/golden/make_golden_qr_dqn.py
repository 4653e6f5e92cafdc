#!/usr/bin/env python
"""Generate tests/golden/qr_dqn.npz by running the REFERENCE's own QuantileRegressionDQNAgent code under the
stub-import harness (_refstub.py), in the manner of make_golden.py::gen_targets.  Run from the repo root in the build
container (the reference tree must be present):

    python tests/golden/make_golden_qr_dqn.py

Recorded:
  * learn_from_batch with stand-in networks: parallel_prediction returns fixed random quantiles, train_and_sync_networks
    records its inputs (TD targets, action locations, quantile midpoints) — three shapes, no tied atoms in any row;
  * get_q_values on a few acting inputs (two of them with exactly tied actions);
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

SHAPES = ((32, 2, 50), (37, 6, 200), (5, 18, 1))     # (B, A, N)


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _no_ties(rng, shape):
    """random quantiles whose rows of atoms hold distinct values (np.argsort's quicksort is not stable)."""
    x = rng.randn(*shape).astype(np.float32)
    flat = x.reshape(-1, shape[-1])
    for r in flat:
        while len(np.unique(r)) != r.size:
            r[:] = rng.randn(r.size).astype(np.float32)
    return x


def gen_learn(out, rng):
    from rl_coach.agents.qr_dqn_agent import QuantileRegressionDQNAgent
    for s, (B, A, N) in enumerate(SHAPES):
        theta = _no_ties(rng, (B, A, N))
        theta_next = rng.randn(B, A, N).astype(np.float32)
        actions = rng.randint(0, A, size=B)
        rewards = rng.randn(B).astype(np.float32)          # fp32-exact values: the device replay stores fp32
        go = rng.rand(B) < 0.3
        captured = {}

        class Fake(QuantileRegressionDQNAgent):
            def __init__(self):
                pass
        f = Fake()
        wrapper = _Obj(input_embedders_parameters={'observation': None})
        f.ap = _Obj(network_wrappers={'main': wrapper}, algorithm=_Obj(discount=0.99, atoms=N))
        f.quantile_probabilities = np.ones(N) / float(N)
        f.q_values = _Obj(add_sample=lambda v: None)
        main = _Obj(target_network=object(), online_network=object(),
                    parallel_prediction=lambda pairs: (theta_next.copy(), theta.copy()))

        def train(inputs, targets):
            captured['targets'] = np.array(targets)
            captured['locations'] = np.array(inputs['output_0_0'])
            captured['midpoints'] = np.array(inputs['output_0_1'])
            return 0.0, [0.0], 0.0
        main.train_and_sync_networks = train
        f.networks = {'main': main}
        tr = [Transition(state={'observation': rng.randn(4)}, action=int(actions[i]), reward=float(rewards[i]),
                         next_state={'observation': rng.randn(4)}, game_over=bool(go[i])) for i in range(B)]
        f.learn_from_batch(Batch(tr))
        p = "s%d_" % s
        out[p + "theta"], out[p + "theta_next"] = theta, theta_next
        out[p + "actions"], out[p + "rewards"], out[p + "go"] = actions, rewards, go
        out[p + "targets"] = captured['targets']                        # fp64, before the fp32 placeholder
        out[p + "locations"] = captured['locations']
        out[p + "midpoints"] = captured['midpoints']                    # fp64, before the fp32 placeholder
        out[p + "discount"] = np.float64(0.99)


def gen_acting(out, rng):
    from rl_coach.agents.qr_dqn_agent import QuantileRegressionDQNAgent

    class Fake(QuantileRegressionDQNAgent):
        def __init__(self):
            pass
    for s, (n, A, N) in enumerate(((4, 2, 50), (3, 6, 200), (2, 18, 1))):
        f = Fake()
        f.quantile_probabilities = np.ones(N) / float(N)
        x = rng.randn(n, A, N).astype(np.float32)
        x[0, 1] = x[0, 0][::-1]           # same atoms in another order: possibly not the same fp64 mean
        x[-1, A - 1] = x[-1, 0]           # identical atoms: an exact tie
        out["act%d_quantiles" % s] = x
        out["act%d_q" % s] = f.get_q_values(x)


def gen_defaults(out):
    from rl_coach.agents.qr_dqn_agent import QuantileRegressionDQNAgentParameters
    ap = QuantileRegressionDQNAgentParameters()
    net = ap.network_wrappers['main']
    sch = ap.exploration.epsilon_schedule
    d = {"atoms": ap.algorithm.atoms, "huber_loss_interval": ap.algorithm.huber_loss_interval,
         "discount": ap.algorithm.discount, "learning_rate": net.learning_rate,
         "optimizer_epsilon": net.optimizer_epsilon, "batch_size": net.batch_size,
         "head": type(net.heads_parameters[0]).__name__,
         "epsilon_schedule": [type(sch).__name__, float(sch.initial_value), float(sch.final_value),
                              int(sch.decay_steps)],
         "evaluation_epsilon": ap.exploration.evaluation_epsilon,
         "num_steps_between_copying_online_weights_to_target":
             ap.algorithm.num_steps_between_copying_online_weights_to_target.num_steps,
         "memory": type(ap.memory).__name__}
    out["defaults"] = np.array(json.dumps(d, sort_keys=True))


def main():
    rng = np.random.RandomState(41)
    out = {}
    gen_learn(out, rng)
    gen_acting(out, rng)
    gen_defaults(out)
    path = os.path.join(HERE, "qr_dqn.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KiB)" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
