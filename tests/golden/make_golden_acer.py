#!/usr/bin/env python
"""Generate tests/golden/acer.npz by running the REFERENCE's own ACERAgent._learn_from_batch and the reference's own
EpisodicExperienceReplay.sample under the stub-import harness (_refstub.py), in the manner of make_golden_n_step_q.py.
Run from the repo root in the build container (the reference tree must be present):

    python tests/golden/make_golden_acer.py

Recorded per case c<k>_:
  * the stand-in networks' fixed fp32 outputs: the online network on the window's states (`q_online`, `policy` [T, A])
    and on the state behind the window (`q_boot`, `policy_boot` [1, A]), the target (average) network's policy on the
    window's states (`avg_policy` [T, A]).  The probabilities are the project's softmax (tests/c51_ref.py) of the
    recorded `logits`, `logits_boot`, `avg_logits`, so that the device launch, which starts from logits, can be fed
    the same case.  `policy` is not stored (it is c51_ref.softmax(logits)); `avg_policy` comes back as `output_1_5`;
  * `mu` [T, A] fp32, the behaviour policy's probabilities of info['all_action_probabilities']: the policy itself in
    every other case (rho = 1 up to eps: rho_bar clips nowhere it matters) and a distribution far from it in the rest
    (rho both above and below 1);
  * `rewards` (fp32-exact: the device keeps filtered rewards as fp32), `actions`, the last transition's `game_over`,
    `discount`;
  * what the agent handed to train_and_sync_networks: `output_1_0` ... `output_1_5`, `target_1`, with the dtypes of all
    eight arrays (`dtypes`, JSON text); `target_0` is the same array as `output_1_3` (the generator asserts equal bits)
    and is stored once; the sample of the 'Values' signal; `boot_rows_asked`: how many rows the bootstrap forward was
    asked for (0: it was not run).
Cases: bootstrapped and terminal windows; T in {1, 2, 5, 200}; discounts 0.99 and 1.0; rewards of 1.0 through a reward
filter scale of 1/200 (as the CartPole_ACER preset has) and uneven ones, alternately; A in {3, 8, 18} (numpy's sum
changes its order at 8); every combination, except that the 200-row windows of A = 8 and 18 keep one bootstrapped and
one terminal case each.  Before anything is written, the generator checks that some bootstrapped case's fp32 targets
differ under the all-fp64 form of the first `discount * Qret`, and that some case's aliased `output_1_3` differs from
the network's own Q values.
`replay_*`: the reference memory's own consecutive-transition draws: episodes of lengths {1, 3, 5, 6, 20} stored in that
order, np.random.seed(REPLAY_SEED), REPLAY_DRAWS times sample(5, True): the chosen episode, start and stop of every draw
and np.random's state afterwards.
`defaults`: the reference parameter classes' defaults (JSON text).  `numpy_version` names what produced the file.
"""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refstub  # noqa: E402

_refstub.install()

import c51_ref  # noqa: E402
from rl_coach.core_types import Batch, Transition  # noqa: E402

LENGTHS = (1, 2, 5, 200)
N_ACTIONS = (3, 8, 18)
REPLAY_LENGTHS, REPLAY_SIZE, REPLAY_SEED, REPLAY_DRAWS = (1, 3, 5, 6, 20), 5, 1611, 64
BITS = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Samples(object):
    def __init__(self):
        self.values = []

    def add_sample(self, v):
        self.values.append(np.array(v))


def run_case(c):
    from rl_coach.agents.acer_agent import ACERAgent

    class Fake(ACERAgent):
        def __init__(self):
            pass
    f = Fake()
    T, A = c["q_online"].shape
    f.ap = _Obj(network_wrappers={'main': _Obj(input_embedders_parameters={'observation': None})},
                algorithm=_Obj(discount=c["discount"], rate_for_copying_weights_to_target=0.01))
    for name in ("q_loss", "policy_loss", "probability_loss", "bias_correction_loss", "unclipped_grads", "V_Values",
                 "kl_divergence"):
        setattr(f, name, _Samples())
    fed, asked, moved = {}, [], []

    def predict_online(inputs):
        rows = np.asarray(inputs['observation']).shape[0]
        if rows == T and not asked and "main" not in fed:
            fed["main"] = True
            return [c["q_online"].copy(), c["policy"].copy()]
        asked.append(rows)
        assert rows == 1
        return [c["q_boot"].copy(), c["policy_boot"].copy()]

    def predict_target(inputs):
        assert np.asarray(inputs['observation']).shape[0] == T
        return [None, c["avg_policy"].copy()]

    def train(inputs, targets, additional_fetches=None):
        assert len(additional_fetches) == 3 and len(targets) == 2
        for i in range(6):
            fed["output_1_%d" % i] = np.array(inputs["output_1_%d" % i])
        fed["target_0"], fed["target_1"] = np.array(targets[0]), np.array(targets[1])
        return 0.0, [0.0, 0.0], 0.0, [0.0, 0.0, 0.0]
    heads = [None, _Obj(probability_loss=None, bias_correction_loss=None, kl_divergence=None)]
    wrapper = _Obj(online_network=_Obj(predict=predict_online, output_heads=heads),
                   target_network=_Obj(predict=predict_target), train_and_sync_networks=train,
                   update_target_network=moved.append)
    f.networks = {'main': wrapper}
    tr = [Transition(state={'observation': np.zeros(4)}, action=int(c["actions"][i]), reward=float(c["rewards"][i]),
                     next_state={'observation': np.zeros(4)}, game_over=bool(c["game_over"]) and i == T - 1,
                     info={'all_action_probabilities': c["mu"][i]})
          for i in range(T)]
    f._learn_from_batch(Batch(tr))
    assert len(asked) <= 1 and len(f.V_Values.values) == 1 and moved == [0.01]
    return fed, f.V_Values.values[0], (asked[0] if asked else 0)


def gen_replay(out):
    from rl_coach.memories.episodic.episodic_experience_replay import EpisodicExperienceReplay
    from rl_coach.memories.memory import MemoryGranularity
    mem = EpisodicExperienceReplay((MemoryGranularity.Transitions, 1000000))
    for e, n in enumerate(REPLAY_LENGTHS):
        for i in range(n):
            mem.store(Transition(state={'observation': np.zeros(1)}, action=0, reward=0.0,
                                 next_state={'observation': np.zeros(1)}, game_over=i == n - 1,
                                 info={'where': (e, i)}))
    assert mem.num_complete_episodes() == len(REPLAY_LENGTHS) and mem.num_transitions() == sum(REPLAY_LENGTHS)
    np.random.seed(REPLAY_SEED)
    draws = []
    for _ in range(REPLAY_DRAWS):
        batch = mem.sample(REPLAY_SIZE, True)
        where = [t.info['where'] for t in batch]
        assert len({w[0] for w in where}) == 1 and [w[1] for w in where] == list(range(where[0][1], where[-1][1] + 1))
        draws.append((where[0][0], where[0][1], where[-1][1] + 1))
    draws = np.array(draws, dtype=np.int64)
    assert set(draws[:, 0]) == set(range(len(REPLAY_LENGTHS))), "every episode is drawn"
    state = np.random.get_state()
    out["replay_lengths"], out["replay_size"] = np.array(REPLAY_LENGTHS, dtype=np.int64), np.int64(REPLAY_SIZE)
    out["replay_seed"], out["replay_draws"] = np.int64(REPLAY_SEED), draws
    out["replay_state_keys"], out["replay_state_pos"] = np.asarray(state[1], dtype=np.uint32), np.int64(state[2])


def gen_defaults(out):
    from rl_coach.agents.acer_agent import ACERAgentParameters
    from rl_coach.base_parameters import EmbedderScheme, MiddlewareScheme
    ap = ACERAgentParameters()
    net, alg = ap.network_wrappers['main'], ap.algorithm
    scheme = lambda s: s.name if isinstance(s, (EmbedderScheme, MiddlewareScheme)) else s
    d = {"apply_gradients_every_x_episodes": alg.apply_gradients_every_x_episodes,
         "num_steps_between_gradient_updates": alg.num_steps_between_gradient_updates,
         "ratio_of_replay": alg.ratio_of_replay,
         "num_transitions_to_start_replay": alg.num_transitions_to_start_replay,
         "rate_for_copying_weights_to_target": alg.rate_for_copying_weights_to_target,
         "importance_weight_truncation": alg.importance_weight_truncation,
         "use_trust_region_optimization": alg.use_trust_region_optimization,
         "max_KL_divergence": alg.max_KL_divergence, "beta_entropy": alg.beta_entropy, "discount": alg.discount,
         "learning_rate": net.learning_rate, "optimizer_type": net.optimizer_type,
         "optimizer_epsilon": net.optimizer_epsilon, "adam_optimizer_beta1": net.adam_optimizer_beta1,
         "adam_optimizer_beta2": net.adam_optimizer_beta2, "clip_gradients": net.clip_gradients,
         "async_training": net.async_training, "shared_optimizer": net.shared_optimizer,
         "create_target_network": net.create_target_network, "batch_size": net.batch_size,
         "heads": [[type(h).__name__, h.loss_weight] for h in net.heads_parameters],
         "embedder_scheme": scheme(net.input_embedders_parameters['observation'].scheme),
         "middleware_scheme": scheme(net.middleware_parameters.scheme),
         "activation_function": net.middleware_parameters.activation_function,
         "classes": [type(alg).__name__, type(net).__name__, type(ap).__name__],
         "exploration": type(ap.exploration[next(iter(ap.exploration))]).__name__
         if isinstance(ap.exploration, dict) else type(ap.exploration).__name__,
         "memory": type(ap.memory).__name__, "memory_max_size": [ap.memory.max_size[0].name, ap.memory.max_size[1]]}
    out["defaults"] = np.array(json.dumps(d, sort_keys=True))


def all_fp64_targets(c):
    """the fp32 retrace values with the OTHER candidate for the first `discount * Qret`: an fp64 product"""
    T = c["rewards"].size
    rows = np.arange(T)
    V = np.sum(c["policy"] * c["q_online"], axis=1)
    rho_bar = np.minimum(1.0, (c["policy"] / (c["mu"] + np.finfo(np.float32).eps))[rows, c["actions"]])
    Qret = 0.0 if c["game_over"] else float(np.sum(c["q_boot"] * c["policy_boot"], axis=1)[0])
    out = np.empty(T, np.float32)
    for i in reversed(range(T)):
        Qret = float(c["rewards"][i]) + c["discount"] * Qret
        out[i] = Qret
        Qret = float(rho_bar[i]) * (Qret - float(c["q_online"][i, c["actions"][i]])) + float(V[i])
    return out


def main():
    rng = np.random.RandomState(1611)
    scale = np.float32(1 / 200.)
    # every combination for the short windows and for A = 3; the 200-row windows of A = 8 and 18 keep one bootstrapped
    # and one terminal case each (with different discounts), which keeps the file small
    cases = [dict(A=A, T=T, game_over=g, discount=d)
             for A, T, g, d in itertools.product(N_ACTIONS, LENGTHS, (False, True), (0.99, 1.0))
             if T < 200 or A == 3 or (g, d) in ({8: (False, 0.99), 18: (False, 1.0)}[A],
                                                {8: (True, 1.0), 18: (True, 0.99)}[A])]
    out, tells_product, tells_alias, clipped = {}, 0, 0, [0, 0]
    for k, c in enumerate(cases):
        T, A = c["T"], c["A"]
        raw = np.ones(T, dtype=np.float32) if k % 2 == 0 else rng.uniform(-1.0, 2.0, size=T).astype(np.float32)
        c["rewards"] = raw * scale
        c["actions"] = rng.randint(0, A, size=T)
        c["q_online"], c["q_boot"] = ((rng.randn(n, A) * 0.3).astype(np.float32) for n in (T, 1))
        c["logits"], c["logits_boot"], c["avg_logits"] = (rng.randn(n, A).astype(np.float32) for n in (T, 1, T))
        c["policy"], c["policy_boot"], c["avg_policy"] = (c51_ref.softmax(c[n]) for n in
                                                          ("logits", "logits_boot", "avg_logits"))
        assert c["policy"].dtype == np.float32
        # mu: the policy itself, or a distribution far from it
        c["mu"] = c["policy"].copy() if (k // 2) % 2 == 0 else c51_ref.softmax(
            (2.0 * rng.randn(T, A)).astype(np.float32))
        fed, values, asked = run_case(c)
        p = "c%d_" % k
        # `policy` is c51_ref.softmax(logits) and is not stored; `avg_policy` comes back as output_1_5
        for name in ("rewards", "actions", "q_online", "q_boot", "logits", "logits_boot", "avg_logits", "policy_boot",
                     "mu"):
            out[p + name] = c[name]
        out[p + "game_over"], out[p + "discount"] = np.bool_(c["game_over"]), np.float64(c["discount"])
        # target_0 IS output_1_3 (the aliasing): stored once, with the fact
        assert np.array_equal(BITS(fed["target_0"]), BITS(fed["output_1_3"]))
        assert np.array_equal(BITS(fed["output_1_5"]), BITS(c["avg_policy"]))
        for name, v in fed.items():
            if name not in ("main", "target_0"):
                out[p + name] = v
        out[p + "dtypes"] = np.array(json.dumps({n: str(v.dtype) for n, v in fed.items() if n != "main"},
                                                sort_keys=True))
        out[p + "values_signal"] = values
        out[p + "boot_rows_asked"] = np.int64(asked)
        assert fed["output_1_4"].dtype == np.float32 and fed["output_1_3"] is not None
        if not c["game_over"]:
            tells_product += not np.array_equal(BITS(fed["output_1_4"]), BITS(all_fp64_targets(c)))
        tells_alias += not np.array_equal(BITS(fed["output_1_3"]), BITS(c["q_online"]))
        rho_i = fed["output_1_2"]
        clipped[0] += int(np.any(rho_i > 1.5))
        clipped[1] += int(np.any(rho_i < 0.5))
    assert tells_product > 0, "no bootstrapped case tells the fp32 from the fp64 first product"
    assert tells_alias > 0, "no case tells the aliased Q values from the network's own"
    assert clipped[0] > 0 and clipped[1] > 0, "rho_bar must both clip and not clip"
    gen_replay(out)
    gen_defaults(out)
    out["n_cases"] = np.int64(len(cases))
    out["reward_scale"] = scale
    out["numpy_version"] = np.array(np.__version__)
    path = os.path.join(HERE, "acer.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d cases, %d arrays, %.1f KiB; numpy %s); cases that tell the two products apart: %d, the aliasing: %d"
          % (path, len(cases), len(out), os.path.getsize(path) / 1024, np.__version__, tells_product, tells_alias))


if __name__ == "__main__":
    main()
