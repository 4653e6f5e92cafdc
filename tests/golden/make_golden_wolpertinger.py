#!/usr/bin/env python
"""Generate tests/golden/wolpertinger.npz by running the REFERENCE's own Wolpertinger code under the stub-import harness
(_refstub.py), in the manner of make_golden_naf.py.  Run from the repo root in the build container (the reference tree
must be present):

    python tests/golden/make_golden_wolpertinger.py

`annoy` is not installed, so this recipe supplies a stand-in module of its own before the reference is imported: its
AnnoyIndex keeps the items as fp32 (as Annoy does), takes the query as fp32 and answers by brute force — per item
acc = 0; for w in order: t = q[w] - item[w]; acc = acc + t * t, every operation rounded to fp32 — ordered by (acc, item
id), distances reported as sqrt(acc).  On top of it the reference's own AnnoyDictionary.add / query,
WolpertingerAgent.get_initialized_knn, BoxDiscretization.get_unfiltered_action_space / filter, AdditiveNoise.get_action,
WolpertingerAgent.choose_action (stand-in networks that return recorded values) and the conversion of
WolpertingerAgent.learn_from_batch run for real.  The critic's stand-in answers predict with the list of its head outputs,
[Q of shape (k, 1)], which is what the `[0]` of choose_action (wolpertinger_agent.py:106) takes the Q values from: the
action is indices[argmax over the k candidates].

The real Annoy's order among equal distances is unspecified, so a step whose query has two equal fp32 distances among
its k + 1 nearest keys is drawn again; fewer than 1 % are (asserted).

Recorded, per case c<i> = (bounds, n, k):
  keys (knn_tree.embeddings, fp64), target_actions (the filter's list, in np.linspace's dtype for the fp32 bounds gym
  gives a box: fp32 under numpy 2's promotion rules), and per step the actor's output (fp32),
  the query as Annoy received it (fp32), the neighbour indices, the critic's values (fp32, some with ties, NaN and -inf),
  the chosen action, the phase (1: TEST); a batch of discrete actions and what learn_from_batch handed to DDPG's update;
and the parameter classes' defaults (JSON text under "defaults").
"""
import json
import os
import sys
import types
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstub  # noqa: E402

QUERIES = []         # every query a built index answered, as it saw it


class AnnoyIndex(object):
    def __init__(self, f, metric='euclidean'):
        assert metric == 'euclidean'
        self.f, self.items, self.built = f, {}, False

    def set_seed(self, seed):
        pass

    def add_item(self, i, vector):
        v = np.asarray(vector, dtype=np.float32)
        assert v.shape == (self.f,)
        self.items[int(i)] = v

    def build(self, n_trees):
        self.ids = np.array(sorted(self.items), dtype=np.int64)
        self.table = np.stack([self.items[i] for i in self.ids]) if len(self.ids) else np.zeros((0, self.f), np.float32)
        self.built = True

    def unbuild(self):
        self.built = False

    def get_nns_by_vector(self, vector, n, search_k=-1, include_distances=False):
        if not self.built or len(self.ids) == 0:
            return ([], []) if include_distances else []
        q = np.asarray(vector, dtype=np.float32).reshape(self.f)
        QUERIES.append(q.copy())
        acc = np.zeros(len(self.ids), dtype=np.float32)
        for w in range(self.f):
            t = q[w] - self.table[:, w]
            acc = acc + t * t
        order = np.lexsort((self.ids, acc))[:n]
        ids = [int(self.ids[j]) for j in order]
        return (ids, [float(np.sqrt(acc[j])) for j in order]) if include_distances else ids


_annoy = types.ModuleType("annoy")
_annoy.AnnoyIndex = AnnoyIndex
sys.modules["annoy"] = _annoy

_refstub.install()

from rl_coach.core_types import Batch, RunPhase, Transition  # noqa: E402

BOUNDS = ((-1.0, 1.0), (-2.0, 3.0))
SIZES = (2, 5, 64)
KS = (1, 3, 5)
STEPS, TEST_STEPS, BATCH = 64, 8, 32


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _fake_agent(low, high, n, k):
    from rl_coach.agents.wolpertinger_agent import WolpertingerAgent
    from rl_coach.exploration_policies.additive_noise import AdditiveNoise
    from rl_coach.filters.action.box_discretization import BoxDiscretization
    from rl_coach.schedules import LinearSchedule
    from rl_coach.spaces import BoxActionSpace

    class Fake(WolpertingerAgent):
        def __init__(self):
            pass
    f = Fake()
    box = BoxActionSpace(1, low=np.array([low], dtype=np.float32), high=np.array([high], dtype=np.float32))
    disc = BoxDiscretization(num_bins_per_dimension=n)
    space = disc.get_unfiltered_action_space(box)
    assert len(space.actions) == n
    f.spaces = _Obj(action=space)
    f.ap = _Obj(algorithm=_Obj(k=k, action_embedding_width=1),
                network_wrappers={'actor': _Obj(input_embedders_parameters={'observation': None})})
    f.exploration_policy = AdditiveNoise(space, LinearSchedule(0.1, 0.1, 50000), 0.05,
                                         noise_as_percentage_from_action_space=False)
    f.action_signal = _Obj(add_sample=lambda v: None)
    f.output_filter = _Obj(action_filters=OrderedDict([('discretization', disc)]))
    f.knn_tree = f.get_initialized_knn()
    return f, disc, box


def _q_values(rng, k, step):
    q = rng.randn(k, 1).astype(np.float32)
    if k > 1 and step % 7 == 3:
        q[rng.randint(k)] = q.max()                  # a tie: np.argmax takes the first
    if k > 1 and step % 11 == 5:
        q[rng.randint(k)] = np.nan
    if step % 13 == 6:
        q[:] = -np.inf
    return q


def gen_case(out, p, low, high, n, k, rng, counts):
    f, disc, box = _fake_agent(low, high, n, k)
    out[p + "low_high"] = np.array([low, high], dtype=np.float32)
    out[p + "n_k"] = np.array([n, k], dtype=np.int64)
    out[p + "max_abs_range"] = np.asarray(box.max_abs_range)
    out[p + "keys"] = f.knn_tree.embeddings.copy()
    out[p + "target_actions"] = np.array(disc.target_actions)         # (in the dtype numpy gives np.linspace of fp32 bounds)
    keys32 = f.knn_tree.embeddings.astype(np.float32)
    rows = {name: [] for name in ("proto", "query", "indices", "q", "action", "test")}
    step = 0
    while step < STEPS + TEST_STEPS:
        test = step >= STEPS
        f.exploration_policy.change_phase(RunPhase.TEST if test else RunPhase.TRAIN)
        proto = (rng.uniform(-1.2, 1.2, (1, 1)) * float(box.max_abs_range[0])).astype(np.float32)
        q = _q_values(rng, k, step)
        seen = {}
        f.networks = {'actor': _Obj(online_network=_Obj(predict=lambda inputs: proto.copy())),
                      'critic': _Obj(online_network=_Obj(predict=lambda inputs: (seen.update(inputs), [q.copy()])[1]))}
        del QUERIES[:]
        info = f.choose_action({'observation': rng.randn(4)})
        assert len(QUERIES) == 1
        query = QUERIES[0]
        counts[0] += 1
        d = np.sort(((query[0] - keys32[:, 0]) * (query[0] - keys32[:, 0])).astype(np.float32))[:k + 1]
        if len(np.unique(d)) != len(d):              # the real Annoy's order would be unspecified: draw again
            counts[1] += 1
            continue
        if test:
            assert query[0] == proto[0, 0]           # no noise in TEST
        assert seen['observation'].shape == (k, 4) and np.asarray(seen['action']).shape == (k, 1)
        idx = [j for j in range(n) if np.any(np.all(np.asarray(seen['action']) == f.knn_tree.embeddings[j], axis=1))]
        assert len(idx) == k
        order = np.lexsort((np.arange(n), ((query[0] - keys32[:, 0]) ** 2).astype(np.float32)))[:k]
        assert np.array_equal(np.asarray(seen['action']), f.knn_tree.embeddings[order])
        rows["proto"].append(proto[0]); rows["query"].append(query); rows["indices"].append(order)
        rows["q"].append(q[:, 0]); rows["action"].append(info.action); rows["test"].append(int(test))
        step += 1
    out[p + "proto"] = np.array(rows["proto"], dtype=np.float32)
    out[p + "query"] = np.array(rows["query"], dtype=np.float32)
    out[p + "indices"] = np.array(rows["indices"], dtype=np.int32)
    out[p + "q"] = np.array(rows["q"], dtype=np.float32)
    out[p + "action"] = np.array(rows["action"], dtype=np.int32)
    out[p + "test"] = np.array(rows["test"], dtype=np.int32)

    # learn_from_batch: what DDPG's update is handed after the conversion
    import rl_coach.agents.ddpg_agent as ddpg
    captured = {}
    original = ddpg.DDPGAgent.learn_from_batch
    ddpg.DDPGAgent.learn_from_batch = lambda self, batch: captured.update(actions=np.array(batch.actions()))
    try:
        actions = rng.randint(0, n, size=BATCH)
        tr = [Transition(state={'observation': rng.randn(4)}, action=int(a), reward=0.0,
                         next_state={'observation': rng.randn(4)}, game_over=False) for a in actions]
        f.learn_from_batch(Batch(tr))
    finally:
        ddpg.DDPGAgent.learn_from_batch = original
    assert captured["actions"].shape == (BATCH,) and captured["actions"].dtype == out[p + "target_actions"].dtype
    out[p + "batch_actions"] = actions.astype(np.int32)
    out[p + "batch_converted"] = captured["actions"]


def defaults(ap):
    """what tests/test_wolpertinger_ref.py reads off the package's own parameter classes"""
    alg, ex = ap.algorithm, ap.exploration
    actor, critic = ap.network_wrappers['actor'], ap.network_wrappers['critic']
    head = actor.heads_parameters[0]
    s = ex.noise_schedule
    return {"k": alg.k, "action_embedding_width": alg.action_embedding_width,
            "use_target_network_for_evaluation": alg.use_target_network_for_evaluation,
            "rate_for_copying_weights_to_target": alg.rate_for_copying_weights_to_target,
            "num_steps_between_copying_online_weights_to_target":
                [type(alg.num_steps_between_copying_online_weights_to_target).__name__,
                 alg.num_steps_between_copying_online_weights_to_target.num_steps],
            "num_consecutive_playing_steps": [type(alg.num_consecutive_playing_steps).__name__,
                                              alg.num_consecutive_playing_steps.num_steps],
            "discount": alg.discount,
            "classes": [type(alg).__name__, type(ex).__name__, type(ap.memory).__name__, type(actor).__name__,
                        type(critic).__name__, type(head).__name__],
            "noise_as_percentage_from_action_space": ex.noise_as_percentage_from_action_space,
            "evaluation_noise": ex.evaluation_noise,
            "noise_schedule": [type(s).__name__, s.initial_value, s.final_value, s.decay_steps],
            "head_activation": head.activation_function, "head_batchnorm": head.batchnorm,
            "actor": [actor.learning_rate, actor.batch_size, actor.optimizer_type, actor.create_target_network],
            "critic": [critic.learning_rate, critic.batch_size, critic.optimizer_type, critic.create_target_network]}


def gen_defaults(out):
    from rl_coach.agents.wolpertinger_agent import WolpertingerAgentParameters
    out["defaults"] = np.array(json.dumps({"plain": defaults(WolpertingerAgentParameters()),
                                           "batchnorm": defaults(WolpertingerAgentParameters(use_batchnorm=True))},
                                          sort_keys=True))


def main():
    rng = np.random.RandomState(1512)
    np.random.seed(7679)                 # AdditiveNoise draws from the global stream
    out, counts, case = {}, [0, 0], 0
    for low, high in BOUNDS:
        for n in SIZES:
            for k in KS:
                if k >= n:               # AnnoyDictionary.has_enough_entries: the reference answers only for k < n
                    continue
                gen_case(out, "c%d_" % case, low, high, n, k, rng, counts)
                case += 1
    out["cases"] = np.int64(case)
    assert counts[1] < 0.01 * counts[0], counts
    print("%d cases, %d steps drawn, %d drawn again" % (case, counts[0], counts[1]))
    gen_defaults(out)
    path = os.path.join(HERE, "wolpertinger.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KiB)" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
