#!/usr/bin/env python
"""Generate tests/golden/a3c.npz by running the REFERENCE's own ActorCriticAgent.learn_from_batch under the stub-import
harness (_refstub.py), in the manner of make_golden_pg.py / make_golden_pal_mmc.py.  Run from the repo root in the
build container (the reference tree must be present):

    python tests/golden/make_golden_a3c.py

Recorded per case c<k>_:
  * the stand-in network's fixed fp32 outputs: V on the window's states [T, 1] (`v`) and on the last next state (`boot`);
    its action probabilities are not read by learn_from_batch;
  * `rewards` (fp32-exact: the device keeps filtered rewards as fp32), `actions`, the last transition's `game_over`;
  * `discount`, `gae_lambda`, `estimate_gae`, `rescaler` (PolicyGradientRescaler's value);
  * `targets` and `advantages`: the two arrays the agent handed to accumulate_gradients, as fp64, with the dtypes and
    shapes they had (`targets_dtype`, `advantages_dtype`), and `fed_actions` = the 'output_1_0' input;
  * `values_signal` / `advantages_signal`: the samples of the 'Values' / 'Advantages' signals.
Cases: A_VALUE and GAE; bootstrapped and terminal windows; T in {1, 2, 5, 200}; for GAE gae_lambda in {1, 0.96} and both
settings of estimate_state_value_using_gae; rewards of 1.0 through a reward filter scale of 1/200 (as the CartPole_A3C
preset has) and uneven ones; discounts 0.99 and 1.0.  `defaults`: the reference parameter classes' defaults (JSON text).
`numpy_version` / `scipy_version` name what produced the file: the types of some intermediates follow numpy's promotion
rule (tests/a3c_ref.py says which lines).
"""
import itertools
import json
import os
import sys

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstub  # noqa: E402

_refstub.install()

from rl_coach.agents.policy_optimization_agent import PolicyGradientRescaler  # noqa: E402
from rl_coach.core_types import Batch, Transition  # noqa: E402
from rl_coach.spaces import DiscreteActionSpace  # noqa: E402

N_ACTIONS = 3
LENGTHS = (1, 2, 5, 200)


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Samples(object):
    def __init__(self):
        self.values = []

    def add_sample(self, v):
        self.values.append(np.array(v))


def run_case(c):
    from rl_coach.agents.actor_critic_agent import ActorCriticAgent

    class Fake(ActorCriticAgent):
        def __init__(self):
            pass
    f = Fake()
    T = c["rewards"].size
    f.ap = _Obj(network_wrappers={'main': _Obj(input_embedders_parameters={'observation': None})},
                algorithm=_Obj(discount=c["discount"], gae_lambda=c["gae_lambda"],
                               estimate_state_value_using_gae=c["estimate_gae"]))
    f.policy_gradient_rescaler = PolicyGradientRescaler(c["rescaler"])
    f.spaces = _Obj(action=DiscreteActionSpace(N_ACTIONS))
    f.state_values, f.action_advantages = _Samples(), _Samples()
    f.unclipped_grads, f.value_loss, f.policy_loss = _Samples(), _Samples(), _Samples()
    probs = np.full((1, N_ACTIONS), 1.0 / N_ACTIONS, dtype=np.float32)
    answers = [[c["v"].copy(), np.repeat(probs, T, axis=0)], [c["boot"].copy(), probs]]
    fed = {}

    def predict(inputs):
        rows = np.asarray(inputs['observation']).shape[0]
        out = answers.pop(0)
        assert out[0].shape == (rows, 1) and out[0].dtype == np.float32
        return out

    def accumulate(inputs, targets):
        fed["actions"] = np.array(inputs['output_1_0'])
        fed["targets"], fed["advantages"] = targets
        return 0.0, [0.0, 0.0], 0.0
    f.networks = {'main': _Obj(online_network=_Obj(predict=predict, accumulate_gradients=accumulate))}
    tr = [Transition(state={'observation': np.zeros(4)}, action=int(c["actions"][i]), reward=float(c["rewards"][i]),
                     next_state={'observation': np.zeros(4)}, game_over=bool(c["game_over"]) and i == T - 1)
          for i in range(T)]
    f.learn_from_batch(Batch(tr))
    assert len(answers) <= 1                                 # A_VALUE with a game over does not ask for the bootstrap
    return fed, f.state_values.values, f.action_advantages.values


def gen_defaults(out):
    from rl_coach.agents.actor_critic_agent import ActorCriticAgentParameters
    ap = ActorCriticAgentParameters()
    net, alg = ap.network_wrappers['main'], ap.algorithm
    d = {"policy_gradient_rescaler": alg.policy_gradient_rescaler.name,
         "apply_gradients_every_x_episodes": alg.apply_gradients_every_x_episodes, "beta_entropy": alg.beta_entropy,
         "num_steps_between_gradient_updates": alg.num_steps_between_gradient_updates, "discount": alg.discount,
         "gae_lambda": alg.gae_lambda, "estimate_state_value_using_gae": alg.estimate_state_value_using_gae,
         "learning_rate": net.learning_rate, "optimizer_type": net.optimizer_type,
         "optimizer_epsilon": net.optimizer_epsilon, "adam_optimizer_beta1": net.adam_optimizer_beta1,
         "adam_optimizer_beta2": net.adam_optimizer_beta2, "clip_gradients": net.clip_gradients,
         "async_training": net.async_training, "create_target_network": net.create_target_network,
         "heads": [[type(h).__name__, h.loss_weight] for h in net.heads_parameters],
         "embedder_scheme": net.input_embedders_parameters['observation'].scheme.name,
         "middleware_scheme": net.middleware_parameters.scheme.name,
         "activation_function": net.middleware_parameters.activation_function,
         "classes": [type(alg).__name__, type(net).__name__, type(ap).__name__],
         "discrete_exploration": type(ap.exploration[DiscreteActionSpace]).__name__,
         "memory": type(ap.memory).__name__}
    out["defaults"] = np.array(json.dumps(d, sort_keys=True))


def main():
    rng = np.random.RandomState(91)
    cases = []
    scale = np.float32(1 / 200.)
    for T, game_over, discount in itertools.product(LENGTHS, (False, True), (0.99, 1.0)):
        cases.append(dict(rescaler="A_VALUE", gae_lambda=0.96, estimate_gae=False, T=T, game_over=game_over,
                          discount=discount))
        for lam, est in itertools.product((1, 0.96), (False, True)):
            cases.append(dict(rescaler="GAE", gae_lambda=lam, estimate_gae=est, T=T, game_over=game_over,
                              discount=discount))
    out = {}
    for k, c in enumerate(cases):
        T = c["T"]
        # CartPole's filtered rewards (1.0 * 1/200 in fp32) in every other case, uneven scaled rewards in the rest
        raw = np.ones(T, dtype=np.float32) if k % 2 == 0 else rng.uniform(-1.0, 2.0, size=T).astype(np.float32)
        c["rewards"] = raw * scale
        c["actions"] = rng.randint(0, N_ACTIONS, size=T)
        c["v"] = (rng.randn(T, 1) * 0.3).astype(np.float32)
        c["boot"] = (rng.randn(1, 1) * 0.3).astype(np.float32)
        c["rescaler"] = PolicyGradientRescaler[c["rescaler"]].value
        fed, values, advantages = run_case(c)
        p = "c%d_" % k
        for name in ("rewards", "actions", "v", "boot"):
            out[p + name] = c[name]
        out[p + "game_over"] = np.bool_(c["game_over"])
        out[p + "discount"], out[p + "gae_lambda"] = np.float64(c["discount"]), np.float64(c["gae_lambda"])
        out[p + "estimate_gae"], out[p + "rescaler"] = np.bool_(c["estimate_gae"]), np.int64(c["rescaler"])
        assert fed["targets"].shape == (T, 1) and fed["advantages"].shape == (T,)
        out[p + "targets"] = np.asarray(fed["targets"], dtype=np.float64).reshape(T)
        out[p + "advantages"] = np.asarray(fed["advantages"], dtype=np.float64)
        out[p + "targets_dtype"] = np.array(str(fed["targets"].dtype))
        out[p + "advantages_dtype"] = np.array(str(fed["advantages"].dtype))
        out[p + "fed_actions"] = fed["actions"]
        assert len(values) == 1 and len(advantages) == 1
        out[p + "values_signal"], out[p + "advantages_signal"] = values[0], advantages[0]
    gen_defaults(out)
    out["n_cases"] = np.int64(len(cases))
    out["reward_scale"] = scale
    out["numpy_version"], out["scipy_version"] = np.array(np.__version__), np.array(scipy.__version__)
    path = os.path.join(HERE, "a3c.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d cases, %d arrays, %.1f KiB; numpy %s, scipy %s)" % (
        path, len(cases), len(out), os.path.getsize(path) / 1024, np.__version__, scipy.__version__))


if __name__ == "__main__":
    main()
