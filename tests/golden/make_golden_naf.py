#!/usr/bin/env python
"""Generate tests/golden/naf.npz by running the REFERENCE's own NAFAgent.learn_from_batch under the stub-import harness
(_refstub.py), in the manner of make_golden_c51.py.  Run from the repo root in the build container (the reference tree
must be present):

    python tests/golden/make_golden_naf.py

Recorded:
  * learn_from_batch with a stand-in network: the target network's predict returns fixed fp32 V(s') [B, 1],
    train_and_sync_networks records the TD targets it is handed (fp64, [B, 1]) and the actions — three cases, ~30 %
    game-overs, one of them with a scalar action;
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

CASES = ((32, 6), (37, 1), (5, 17))      # (B, A)


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _fake_agent(discount=0.99):
    from rl_coach.agents.naf_agent import NAFAgent

    class Fake(NAFAgent):
        def __init__(self):
            pass
    f = Fake()
    wrapper = _Obj(input_embedders_parameters={'observation': None})
    f.ap = _Obj(network_wrappers={'main': wrapper}, algorithm=_Obj(discount=discount))
    f.TD_targets = _Obj(add_sample=lambda v: None)
    return f


def gen_learn(out, rng):
    for s, (B, A) in enumerate(CASES):
        f = _fake_agent()
        v_next = (rng.randn(B, 1) * 3).astype(np.float32)
        actions = rng.randn(B, A).astype(np.float32)
        rewards = rng.randn(B).astype(np.float32)           # fp32-exact: the replay's type
        go = rng.rand(B) < 0.3
        captured = {}
        target = _Obj(output_heads=[_Obj(V="V")])
        target.predict = lambda inputs, outputs=None, squeeze_output=True: v_next.copy()
        main = _Obj(target_network=target)

        def train(inputs, targets):
            captured['targets'] = np.array(targets)
            captured['actions'] = np.array(inputs['output_0_0'])
            return 0.0, [0.0], 0.0
        main.train_and_sync_networks = train
        f.networks = {'main': main}
        tr = [Transition(state={'observation': rng.randn(4)}, action=actions[i] if A > 1 else float(actions[i, 0]),
                         reward=float(rewards[i]), next_state={'observation': rng.randn(4)}, game_over=bool(go[i]))
              for i in range(B)]
        f.learn_from_batch(Batch(tr))
        assert captured['targets'].shape == (B, 1) and captured['targets'].dtype == np.float64
        assert captured['actions'].shape == (B, A)
        p = "s%d_" % s
        out[p + "v_next"], out[p + "actions"], out[p + "rewards"], out[p + "go"] = v_next, actions, rewards, go
        out[p + "td_targets"] = captured['targets']
        out[p + "fed_actions"] = captured['actions']
        out[p + "discount"] = np.float64(0.99)
        print("case %d (B %d, A %d): %d game-overs" % (s, B, A, int(go.sum())))


def defaults(ap):
    """what tests/test_naf_ref.py reads off the package's own parameter classes"""
    net, alg, head = ap.network_wrappers['main'], ap.algorithm, ap.network_wrappers['main'].heads_parameters[0]
    return {"learning_rate": net.learning_rate, "optimizer_type": net.optimizer_type, "batch_size": net.batch_size,
            "optimizer_epsilon": net.optimizer_epsilon, "adam_optimizer_beta1": net.adam_optimizer_beta1,
            "adam_optimizer_beta2": net.adam_optimizer_beta2, "async_training": net.async_training,
            "create_target_network": net.create_target_network,
            "replace_mse_with_huber_loss": net.replace_mse_with_huber_loss, "clip_gradients": net.clip_gradients,
            "gradients_clipping_method": net.gradients_clipping_method.name,
            "embedder_scheme": str(getattr(net.input_embedders_parameters['observation'].scheme, "name",
                                           net.input_embedders_parameters['observation'].scheme)),
            "middleware_scheme": str(getattr(net.middleware_parameters.scheme, "name",
                                             net.middleware_parameters.scheme)),
            "head": type(head).__name__, "head_activation": head.activation_function,
            "head_loss_weight": head.loss_weight,
            "head_rescale": head.rescale_gradient_from_head_by_factor,
            "classes": [type(alg).__name__, type(ap.exploration).__name__, type(net).__name__,
                        type(ap.memory).__name__],
            "discount": alg.discount, "num_consecutive_training_steps": alg.num_consecutive_training_steps,
            "num_consecutive_playing_steps": [type(alg.num_consecutive_playing_steps).__name__,
                                              alg.num_consecutive_playing_steps.num_steps],
            "num_steps_between_copying_online_weights_to_target":
                [type(alg.num_steps_between_copying_online_weights_to_target).__name__,
                 alg.num_steps_between_copying_online_weights_to_target.num_steps],
            "rate_for_copying_weights_to_target": alg.rate_for_copying_weights_to_target,
            "ou": [ap.exploration.mu, ap.exploration.theta, ap.exploration.sigma, ap.exploration.dt]}


def gen_defaults(out):
    from rl_coach.agents.naf_agent import NAFAgentParameters
    out["defaults"] = np.array(json.dumps(defaults(NAFAgentParameters()), sort_keys=True))


def main():
    rng = np.random.RandomState(1603)
    out = {}
    gen_learn(out, rng)
    gen_defaults(out)
    path = os.path.join(HERE, "naf.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KiB)" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
