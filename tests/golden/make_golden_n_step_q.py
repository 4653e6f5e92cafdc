#!/usr/bin/env python
"""Generate tests/golden/n_step_q.npz by running the REFERENCE's own NStepQAgent.learn_from_batch under the stub-import
harness (_refstub.py), in the manner of make_golden_a3c.py.  Run from the repo root in the build container (the
reference tree must be present):

    python tests/golden/make_golden_n_step_q.py

Recorded per case c<k>_:
  * the stand-in networks' fixed fp32 outputs: the online network on the window's states [T, A] (`q_online`) and the
    TARGET network on the state behind the window [1, A] ('N-Step') or on the T next states [T, A] ('1-Step')
    (`q_target`);
  * `rewards` (fp32-exact: the device keeps filtered rewards as fp32), `actions`, the last transition's `game_over`;
  * `discount`, `horizon` ('N-Step' / '1-Step');
  * `fed`: the matrix the agent handed to accumulate_gradients, with the dtype it had (`fed_dtype`);
  * `q_values_signal`: the sample of the 'Q Values' signal;
  * `target_rows_asked`: how many rows the target network was asked for (0: it was not run).
Cases: both horizons; bootstrapped and terminal windows; T in {1, 2, 5, 200}; discounts 0.99 and 1.0; rewards of 1.0
through a reward filter scale of 1/200 (as the CartPole_NStepQ preset has) and uneven ones, alternately; A = 3.
Before anything is written, the generator checks that for each horizon some bootstrapped case's fp32 targets differ
between the fp32 and the fp64 form of `discount * <the target network's maximum>`: the fixture then shows which of
the two the reference uses.  `defaults`: the reference parameter classes' defaults (JSON text).  `numpy_version` names
what produced the file: the types of the intermediates follow numpy's promotion rule (tests/n_step_q_ref.py says which
lines).
"""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstub  # noqa: E402

_refstub.install()

from rl_coach.core_types import Batch, Transition  # noqa: E402

N_ACTIONS = 3
LENGTHS = (1, 2, 5, 200)
HORIZONS = ('N-Step', '1-Step')


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Samples(object):
    def __init__(self):
        self.values = []

    def add_sample(self, v):
        self.values.append(np.array(v))


def run_case(c):
    from rl_coach.agents.n_step_q_agent import NStepQAgent

    class Fake(NStepQAgent):
        def __init__(self):
            pass
    f = Fake()
    T = c["rewards"].size
    f.ap = _Obj(network_wrappers={'main': _Obj(input_embedders_parameters={'observation': None})},
                algorithm=_Obj(discount=c["discount"], targets_horizon=c["horizon"]))
    f.q_values, f.value_loss = _Samples(), _Samples()
    fed, asked = {}, []

    def predict_online(inputs):
        assert np.asarray(inputs['observation']).shape[0] == T
        return c["q_online"].copy()

    def predict_target(inputs):
        rows = np.asarray(inputs['observation']).shape[0]
        asked.append(rows)
        assert c["q_target"].shape == (rows, N_ACTIONS) and c["q_target"].dtype == np.float32
        return c["q_target"].copy()

    def accumulate(inputs, targets):
        assert np.asarray(inputs['observation']).shape[0] == T and len(targets) == 1
        fed["targets"] = np.array(targets[0])
        return 0.0, [0.0], 0.0
    f.networks = {'main': _Obj(online_network=_Obj(predict=predict_online, accumulate_gradients=accumulate),
                               target_network=_Obj(predict=predict_target))}
    tr = [Transition(state={'observation': np.zeros(4)}, action=int(c["actions"][i]), reward=float(c["rewards"][i]),
                     next_state={'observation': np.zeros(4)}, game_over=bool(c["game_over"]) and i == T - 1)
          for i in range(T)]
    f.learn_from_batch(Batch(tr))
    assert len(asked) <= 1 and len(f.q_values.values) == 1
    return fed["targets"], f.q_values.values[0], (asked[0] if asked else 0)


def other_form(c):
    """the fp32 targets with the OTHER candidate for `discount * <maximum>`: all-fp64 for 'N-Step' (whose expected form
    is the fp32 product), the fp32 product for '1-Step' (whose expected form is fp64)"""
    r, T = c["rewards"].astype(np.float64), c["rewards"].size
    out = np.empty(T, np.float32)
    if c["horizon"] == 'N-Step':
        R = 0.0 if c["game_over"] else float(c["q_target"].max())
        for i in reversed(range(T)):
            R = r[i] + c["discount"] * R
            out[i] = R
    else:
        for i in range(T):
            go = c["game_over"] and i == T - 1
            out[i] = r[i] + (0.0 if go else np.float64(np.float32(c["discount"]) * c["q_target"][i].max()))
    return out


def gen_defaults(out):
    from rl_coach.agents.n_step_q_agent import NStepQAgentParameters
    from rl_coach.base_parameters import EmbedderScheme, MiddlewareScheme
    ap = NStepQAgentParameters()
    net, alg = ap.network_wrappers['main'], ap.algorithm
    copy = alg.num_steps_between_copying_online_weights_to_target
    scheme = lambda s: s.name if isinstance(s, (EmbedderScheme, MiddlewareScheme)) else s
    d = {"num_steps_between_copying_online_weights_to_target": [type(copy).__name__, copy.num_steps],
         "apply_gradients_every_x_episodes": alg.apply_gradients_every_x_episodes,
         "num_steps_between_gradient_updates": alg.num_steps_between_gradient_updates,
         "targets_horizon": alg.targets_horizon, "discount": alg.discount,
         "rate_for_copying_weights_to_target": alg.rate_for_copying_weights_to_target,
         "learning_rate": net.learning_rate, "optimizer_type": net.optimizer_type,
         "optimizer_epsilon": net.optimizer_epsilon, "adam_optimizer_beta1": net.adam_optimizer_beta1,
         "adam_optimizer_beta2": net.adam_optimizer_beta2, "clip_gradients": net.clip_gradients,
         "async_training": net.async_training, "shared_optimizer": net.shared_optimizer,
         "create_target_network": net.create_target_network,
         "replace_mse_with_huber_loss": net.replace_mse_with_huber_loss, "batch_size": net.batch_size,
         "heads": [[type(h).__name__, h.loss_weight] for h in net.heads_parameters],
         "embedder_scheme": scheme(net.input_embedders_parameters['observation'].scheme),
         "middleware_scheme": scheme(net.middleware_parameters.scheme),
         "activation_function": net.middleware_parameters.activation_function,
         "classes": [type(alg).__name__, type(net).__name__, type(ap).__name__],
         "exploration": type(ap.exploration).__name__, "memory": type(ap.memory).__name__}
    out["defaults"] = np.array(json.dumps(d, sort_keys=True))


def main():
    rng = np.random.RandomState(173)
    scale = np.float32(1 / 200.)
    cases = [dict(horizon=h, T=T, game_over=g, discount=d)
             for h, T, g, d in itertools.product(HORIZONS, LENGTHS, (False, True), (0.99, 1.0))]
    out, shows = {}, {h: 0 for h in HORIZONS}
    for k, c in enumerate(cases):
        T = c["T"]
        # CartPole's filtered rewards (1.0 * 1/200 in fp32) in every other case, uneven scaled rewards in the rest
        raw = np.ones(T, dtype=np.float32) if k % 2 == 0 else rng.uniform(-1.0, 2.0, size=T).astype(np.float32)
        c["rewards"] = raw * scale
        c["actions"] = rng.randint(0, N_ACTIONS, size=T)
        c["q_online"] = (rng.randn(T, N_ACTIONS) * 0.3).astype(np.float32)
        c["q_target"] = (rng.randn(1 if c["horizon"] == 'N-Step' else T, N_ACTIONS) * 0.3).astype(np.float32)
        fed, signal, asked = run_case(c)
        p = "c%d_" % k
        for name in ("rewards", "actions", "q_online", "q_target"):
            out[p + name] = c[name]
        out[p + "game_over"], out[p + "discount"] = np.bool_(c["game_over"]), np.float64(c["discount"])
        out[p + "horizon"] = np.array(c["horizon"])
        assert fed.shape == (T, N_ACTIONS)
        out[p + "fed"], out[p + "fed_dtype"] = fed, np.array(str(fed.dtype))
        out[p + "q_values_signal"] = signal
        out[p + "target_rows_asked"] = np.int64(asked)
        if not c["game_over"]:
            mine = fed[np.arange(T), c["actions"]].astype(np.float32)
            shows[c["horizon"]] += not np.array_equal(mine.view(np.uint32), other_form(c).view(np.uint32))
    assert all(n > 0 for n in shows.values()), "no case tells the fp32 from the fp64 product: %r" % shows
    gen_defaults(out)
    out["n_cases"] = np.int64(len(cases))
    out["reward_scale"] = scale
    out["numpy_version"] = np.array(np.__version__)
    path = os.path.join(HERE, "n_step_q.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d cases, %d arrays, %.1f KiB; numpy %s); cases that tell the two products apart: %r" % (
        path, len(cases), len(out), os.path.getsize(path) / 1024, np.__version__, shows))


if __name__ == "__main__":
    main()
