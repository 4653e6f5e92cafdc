#!/usr/bin/env python
"""Generate tests/golden/ppo_kl.npz by running the REFERENCE's own PPOAgent (agents/ppo_agent.py) under the stub-import
harness (_refstub.py), in the manner of make_golden_a3c.py.  Run from the repo root in the build container (the
reference tree must be present):

    python tests/golden/make_golden_ppo_kl.py

Per case c<k>_ the agent's fill_advantages, train_value_network(dataset, 1), and then, three times over,
train_policy_network(dataset, 10) + update_kl_coefficient run against stand-in networks that record every feed and answer
with prescribed numbers.  Recorded:
  * the inputs: `lengths` (the episodes of the dataset, in order), `rewards` (fp32-exact), `v` (the critic's fp32 answer
    on every row), `discount`, `gae_lambda`, `num_steps` (num_consecutive_playing_steps), `batch_size`, `target_kl`,
    `action_kind` (0 discrete, 1 Box with vector actions, 2 Box with scalar actions), `action_dim`, `actions`;
  * `adv_raw`: the per-episode GAE advantages as get_general_advantage_estimation_values returned them, concatenated;
    `adv`: the standardised advantages (the 'Advantages' signal; also what every transition's info holds), both fp64,
    with `adv_dtype`;
  * `value_batches` [n, 2]: first and one-past-last dataset row of every critic minibatch, in order; `value_targets`: the
    targets fed, concatenated, with `value_targets_dtype` and `value_targets_shape` (of one minibatch);
  * `policy_batches` [n, 2]: the same for every actor minibatch of the first policy phase (10 epochs);
    `fed_actions` / `fed_advantages`: 'output_0_0' and the [advantages] target of the first epoch, concatenated, with
    their dtypes and the shape of one minibatch's actions; `fed_old`: how many 'output_0_<i>' old-policy inputs were fed;
  * `kl` [3, 10, n_batches], `entropy` alike: the prescribed fetches; `kl_mean` [3] / `entropy_mean` [3]: the last
    epoch's means as the agent kept them (total_kl_divergence_during_training_process, the 'Entropy' signal) with
    `kl_mean_dtype`; `coefficient` [4]: the kl_coefficient variable before the first and after every update, with
    `coefficient_dtype` (of the value handed to set_variable_value).
`defaults`: the reference parameter classes' defaults (JSON text).  `numpy_version` names what produced the file: the
types of the coefficient update follow numpy's promotion rule (tests/ppo_kl_ref.py says which lines).
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstub  # noqa: E402

_refstub.install()

from rl_coach.agents.policy_optimization_agent import PolicyGradientRescaler  # noqa: E402
from rl_coach.core_types import Episode, Transition  # noqa: E402
from rl_coach.spaces import BoxActionSpace, DiscreteActionSpace  # noqa: E402

N_ACTIONS = 3
EPOCHS = 10
INITIAL_COEFFICIENT = np.float32(0.1)


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Samples(object):
    def __init__(self):
        self.values = []

    def add_sample(self, v):
        self.values.append(np.array(v))


def _noop(*a, **k):
    return None


def run_case(c):
    from rl_coach.agents.ppo_agent import PPOAgent

    class Fake(PPOAgent):
        def __init__(self):
            pass
    f = Fake()
    n_rows = int(sum(c["lengths"]))
    wrapper = _Obj(input_embedders_parameters={'observation': None}, batch_size=c["batch_size"],
                   learning_rate_decay_rate=0, learning_rate=1e-3)
    f.ap = _Obj(network_wrappers={'critic': wrapper, 'actor': wrapper}, task_parameters=None, learning_rate=None,
                algorithm=_Obj(discount=c["discount"], gae_lambda=c["gae_lambda"], estimate_state_value_using_gae=False,
                               value_targets_mix_fraction=0.1, target_kl_divergence=c["target_kl"]))
    f.policy_gradient_rescaler = PolicyGradientRescaler.GAE
    discrete = c["action_kind"] == 0
    f.spaces = _Obj(action=DiscreteActionSpace(N_ACTIONS) if discrete else
                    BoxActionSpace(c["action_dim"], -np.ones(c["action_dim"]), np.ones(c["action_dim"])))
    for name in ("action_advantages", "unclipped_grads", "entropy", "kl_divergence", "value_loss", "policy_loss",
                 "curr_learning_rate"):
        setattr(f, name, _Samples())
    f.total_kl_divergence_during_training_process = 0.0

    transitions, row = [], 0
    for L in c["lengths"]:
        ep = Episode(discount=c["discount"])
        for i in range(L):
            a = c["actions"][row]
            action = int(a) if discrete else (float(a[0]) if c["action_kind"] == 2 else np.array(a, dtype=np.float64))
            ep.insert(Transition(state={'observation': np.array([float(row)])}, action=action,
                                 reward=float(c["rewards"][row]), next_state={'observation': np.array([float(row + 1)])},
                                 game_over=i == L - 1))
            row += 1
        ep.update_transitions_rewards_and_bootstrap_data()
        transitions += ep.transitions
    f.memory = _Obj(transitions=transitions)

    rec = dict(adv_raw=[], value_batches=[], value_targets=[], policy_batches=[], fed_actions=[], fed_advantages=[])
    real_gae = PPOAgent.get_general_advantage_estimation_values

    def gae(rewards, values):
        out = real_gae(f, rewards, values)
        rec["adv_raw"].append(np.array(out[0]))
        return out
    f.get_general_advantage_estimation_values = gae

    def rows_of(inputs):
        idx = np.asarray(inputs['observation'])[:, 0].astype(np.int64)
        assert np.array_equal(idx, np.arange(idx[0], idx[0] + idx.size))
        return int(idx[0]), int(idx[0] + idx.size)

    def critic_predict(inputs):
        lo, hi = rows_of(inputs)
        return c["v"][lo:hi].reshape(-1, 1).copy()

    def critic_accumulate(inputs, targets):
        assert not any(k.startswith('output_') for k in inputs)      # the VHead takes no old-policy input (:228-231)
        rec["value_batches"].append(rows_of(inputs))
        rec["value_targets"].append(np.array(targets))
        return [np.float32(0.5)]
    critic = _Obj(online_network=_Obj(predict=critic_predict, accumulate_gradients=critic_accumulate, optimizer_type='Adam',
                                      inputs=[], reset_accumulated_gradients=_noop),
                  target_network=_Obj(predict=lambda inputs: np.zeros((rows_of(inputs)[1] - rows_of(inputs)[0], 1),
                                                                       dtype=np.float32)),
                  apply_gradients_to_online_network=_noop)

    state = dict(coefficient=INITIAL_COEFFICIENT, set_dtypes=[], phase=0, call=0)

    def actor_target_predict(inputs):
        lo, hi = rows_of(inputs)
        if discrete:
            return np.full((hi - lo, N_ACTIONS), 1.0 / N_ACTIONS, dtype=np.float32)
        return [np.zeros((hi - lo, c["action_dim"]), dtype=np.float32), np.ones((hi - lo, c["action_dim"]), dtype=np.float32)]

    def actor_accumulate(inputs, targets, additional_fetches=None):
        assert additional_fetches == ['kl', 'ent'] and len(targets) == 1
        n_b = n_used // c["batch_size"]
        epoch, b = divmod(state["call"], n_b)
        state["call"] += 1
        if state["phase"] == 0:
            rec["policy_batches"].append(rows_of(inputs))
            if epoch == 0:
                rec["fed_actions"].append(np.array(inputs['output_0_0']))
                rec["fed_advantages"].append(np.array(targets[0]))
                rec["fed_old"] = len([k for k in inputs if k.startswith('output_0_')]) - 1
        p = state["phase"]
        return np.float32(0.1), [np.float32(0.1)], np.float32(1.0), [c["kl"][p, epoch, b], c["entropy"][p, epoch, b]]

    def set_variable_value(assign_op, value, placeholder):
        state["set_dtypes"].append(str(np.asarray(value).dtype) if isinstance(value, np.generic) else type(value).__name__)
        state["coefficient"] = np.float32(value)                    # the tf.Variable is float32
    head = _Obj(kl_divergence='kl', entropy='ent', kl_coefficient='klc', assign_kl_coefficient='assign',
                kl_coefficient_ph='ph')
    actor = _Obj(online_network=_Obj(accumulate_gradients=actor_accumulate, output_heads=[head],
                                     reset_accumulated_gradients=_noop,
                                     get_variable_value=lambda v: state["coefficient"],
                                     set_variable_value=set_variable_value),
                 target_network=_Obj(predict=actor_target_predict), apply_gradients_to_online_network=_noop)
    f.networks = {'critic': critic, 'actor': actor}

    n_used = min(c["num_steps"], n_rows)
    with contextlib.redirect_stdout(io.StringIO()):
        dataset = f.memory.transitions                               # train(): :372-380
        f.fill_advantages(dataset)
        dataset = dataset[:c["num_steps"]]
        f.train_value_network(dataset, 1)
        coefficients, kl_means, ent_means, kl_dtypes = [state["coefficient"]], [], [], []
        for phase in range(3):
            state["phase"], state["call"] = phase, 0
            f.train_policy_network(dataset, EPOCHS)
            f.update_kl_coefficient()
            kl_means.append(f.total_kl_divergence_during_training_process)
            kl_dtypes.append(str(np.asarray(f.total_kl_divergence_during_training_process).dtype))
            ent_means.append(f.entropy.values[-1])
            coefficients.append(state["coefficient"])
    assert len(set(kl_dtypes)) == 1 and len(set(state["set_dtypes"])) == 1, (kl_dtypes, state["set_dtypes"])
    info_adv = np.array([t.info['advantage'] for t in transitions])
    assert np.array_equal(info_adv, f.action_advantages.values[0])
    return rec, f.action_advantages.values[0], np.array(coefficients), np.array(kl_means), np.array(ent_means), \
        kl_dtypes[0], state["set_dtypes"][0]


def gen_defaults(out):
    from rl_coach.agents.ppo_agent import PPOAgentParameters
    ap = PPOAgentParameters()
    alg = ap.algorithm
    d = {"algorithm": {k: (v.name if hasattr(v, "name") and not isinstance(v, (int, float, str, bool)) else
                           (type(v).__name__ + ":" + str(getattr(v, "num_steps", ""))
                            if type(v).__name__ in ("EnvironmentSteps", "EnvironmentEpisodes", "TrainingSteps") else v))
                       for k, v in sorted(vars(alg).items())
                       if isinstance(v, (int, float, str, bool, type(None))) or hasattr(v, "name") or hasattr(v, "num_steps")},
         "classes": [type(alg).__name__, type(ap.network_wrappers['actor']).__name__,
                     type(ap.network_wrappers['critic']).__name__, type(ap).__name__],
         "memory": type(ap.memory).__name__,
         "exploration": {k.__name__: type(v).__name__ for k, v in ap.exploration.items()}}
    for name in ("actor", "critic"):
        net = ap.network_wrappers[name]
        d[name] = {"learning_rate": net.learning_rate, "optimizer_type": net.optimizer_type, "batch_size": net.batch_size,
                   "async_training": net.async_training, "l2_regularization": net.l2_regularization,
                   "create_target_network": net.create_target_network, "clip_gradients": net.clip_gradients,
                   "optimizer_epsilon": net.optimizer_epsilon, "adam_optimizer_beta1": net.adam_optimizer_beta1,
                   "adam_optimizer_beta2": net.adam_optimizer_beta2,
                   "heads": [[type(h).__name__, h.loss_weight] for h in net.heads_parameters],
                   "embedder_scheme": net.input_embedders_parameters['observation'].scheme.name,
                   "embedder_activation": net.input_embedders_parameters['observation'].activation_function,
                   "middleware_scheme": net.middleware_parameters.scheme.name,
                   "middleware_activation": net.middleware_parameters.activation_function}
    out["defaults"] = np.array(json.dumps(d, sort_keys=True, default=str))


def main():
    rng = np.random.RandomState(211)
    cases = [dict(lengths=[64], num_steps=64, batch_size=32, action_kind=0, action_dim=1),
             dict(lengths=[20, 37, 15, 28], num_steps=100, batch_size=32, action_kind=0, action_dim=1),
             dict(lengths=[50, 60, 40], num_steps=128, batch_size=32, action_kind=1, action_dim=1),
             dict(lengths=[33, 31], num_steps=64, batch_size=16, action_kind=1, action_dim=3),
             dict(lengths=[1, 70, 9], num_steps=72, batch_size=24, action_kind=2, action_dim=1),
             dict(lengths=[40, 41], num_steps=2048, batch_size=16, action_kind=0, action_dim=1)]
    # the three phases of a case: last-epoch mean KL relative to the target (above 1.3 x, below 0.7 x, in between), in an
    # order that differs from case to case; the earlier epochs carry other values (only the last epoch counts)
    orders = [(2.0, 0.3, 1.0), (0.3, 0.3, 2.0), (2.0, 2.0, 2.0), (1.0, 0.3, 2.0), (1.29, 1.31, 0.69), (0.71, 2.0, 0.3)]
    out = {}
    for k, c in enumerate(cases):
        n = int(sum(c["lengths"]))
        c["discount"], c["gae_lambda"] = (0.99, 0.96) if k % 2 == 0 else (0.95, 1.0)
        c["target_kl"] = 0.01 if k != 3 else 0.02
        c["rewards"] = (rng.uniform(-1.0, 2.0, size=n).astype(np.float32) if k % 2 else
                        np.ones(n, dtype=np.float32) * np.float32(1 / 200.))
        c["v"] = (rng.randn(n) * 0.3).astype(np.float32)
        c["actions"] = rng.randint(0, N_ACTIONS, size=n) if c["action_kind"] == 0 else rng.randn(n, c["action_dim"])
        n_b = min(c["num_steps"], n) // c["batch_size"]
        factor = np.array(orders[k])[:, None, None] * np.ones((3, EPOCHS, n_b))
        factor[:, :-1] = rng.uniform(0.1, 4.0, size=(3, EPOCHS - 1, n_b))
        c["kl"] = (c["target_kl"] * factor * rng.uniform(0.97, 1.03, size=factor.shape)).astype(np.float32)
        if k == 4:                                                   # 1.29 / 1.31 / 0.69 must stay on their side
            c["kl"][:, -1] = (c["target_kl"] * np.array(orders[k])[:, None] * np.ones((3, n_b))).astype(np.float32)
        c["entropy"] = rng.uniform(0.5, 1.5, size=factor.shape).astype(np.float32)
        rec, adv, coefficients, kl_means, ent_means, kl_dtype, coef_dtype = run_case(c)
        p = "c%d_" % k
        for name in ("lengths", "rewards", "v", "actions", "kl", "entropy"):
            out[p + name] = np.asarray(c[name])
        for name in ("num_steps", "batch_size", "action_kind", "action_dim"):
            out[p + name] = np.int64(c[name])
        for name in ("discount", "gae_lambda", "target_kl"):
            out[p + name] = np.float64(c[name])
        raw = np.concatenate(rec["adv_raw"])
        assert raw.dtype == np.float64 and adv.dtype == np.float64 and raw.shape == adv.shape == (n,)
        out[p + "adv_raw"], out[p + "adv"], out[p + "adv_dtype"] = raw, adv, np.array(str(adv.dtype))
        out[p + "value_batches"] = np.array(rec["value_batches"], dtype=np.int64)
        out[p + "value_targets"] = np.concatenate(rec["value_targets"]).astype(np.float64).reshape(-1)
        out[p + "value_targets_dtype"] = np.array(str(rec["value_targets"][0].dtype))
        out[p + "value_targets_shape"] = np.array(rec["value_targets"][0].shape, dtype=np.int64)
        out[p + "policy_batches"] = np.array(rec["policy_batches"], dtype=np.int64)
        out[p + "fed_actions"] = np.concatenate(rec["fed_actions"])
        out[p + "fed_actions_dtype"] = np.array(str(rec["fed_actions"][0].dtype))
        out[p + "fed_actions_shape"] = np.array(rec["fed_actions"][0].shape, dtype=np.int64)
        out[p + "fed_advantages"] = np.concatenate(rec["fed_advantages"])
        out[p + "fed_advantages_dtype"] = np.array(str(rec["fed_advantages"][0].dtype))
        out[p + "fed_old"] = np.int64(rec["fed_old"])
        out[p + "kl_mean"], out[p + "entropy_mean"] = kl_means, ent_means
        out[p + "kl_mean_dtype"] = np.array(kl_dtype)
        out[p + "coefficient"], out[p + "coefficient_dtype"] = coefficients, np.array(coef_dtype)
    gen_defaults(out)
    out["n_cases"] = np.int64(len(cases))
    out["initial_coefficient"] = INITIAL_COEFFICIENT
    out["numpy_version"] = np.array(np.__version__)
    path = os.path.join(HERE, "ppo_kl.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d cases, %d arrays, %.1f KiB; numpy %s)" % (path, len(cases), len(out),
                                                                    os.path.getsize(path) / 1024, np.__version__))


if __name__ == "__main__":
    main()
