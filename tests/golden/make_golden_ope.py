#!/usr/bin/env python
"""Generate tests/golden/ope.npz by running the REFERENCE's own off-policy evaluators under the stub-import harness
(_refstub.py), in the manner of make_golden_bcq.py.  Run from the repo root where the reference tree is present:

    python tests/golden/make_golden_ope.py

Recorded, per case of CASES (episode lengths, A, batch size, softmax temperature): the inputs — q and reward-model
outputs of stand-in networks (fixed fp32 linear maps of a 4-float observation, evaluated row by row so that a row's value
does not depend on the batch it is in; the q network's `.softmax` output is ope_ref.softmax32), actions, rewards
(fp32-representable), the stored behaviour probabilities mu (fp32, alternating uniform rows and rows bounded below by
0.2 / A), the episode offsets and every transition's n_step_discounted_rewards after Episode.update_discounted_rewards()
— and what OpeManager.gather_static_shared_stats + OpeManager.evaluate (DoublyRobust, SequentialDoublyRobust,
WeightedImportanceSampling inside it) return: the five estimates, with the policy probabilities and the v values the
manager wrote into the transitions' info.

Input condition: in every case the largest episode weight w_e is > 1e-3, so that sum w_e is not made of products that
underflowed in the reference's fp32 (it multiplies fp32 ratios; the restatement multiplies in fp64).  The range of w_e is
printed per case.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]
import _refstub  # noqa: E402

_refstub.install()

import ope_ref  # noqa: E402
from rl_coach.core_types import Episode, Transition  # noqa: E402
from rl_coach.off_policy_evaluators.ope_manager import OpeManager  # noqa: E402

F32 = np.float32
WIDTH = 4
DISCOUNT = 0.99
# (episode lengths, A, batch size, temperature)
CASES = (([1], 2, 32, 0.2), ([1, 1, 1, 1, 1], 2, 32, 1.0),
         ([7, 64, 65, 1, 200, 13], 3, 32, 0.2), ([7, 64, 65, 1, 200, 13], 3, 32, 1.0),
         ([129, 1, 63, 300], 18, 32, 0.2), ([129, 1, 63, 300], 18, 32, 1.0),
         ([7, 64, 65, 1, 200, 13], 3, 512, 0.2))                      # batch size larger than the evaluation set


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def linear(obs, W, b):
    """fp32, one product and one addition per input, in input order: a row's value does not depend on its batch"""
    out = np.tile(b.astype(F32), (obs.shape[0], 1))
    for f in range(obs.shape[1]):
        out = out + obs[:, f, None] * W[None, f, :]
    assert out.dtype == F32
    return out


def make_case(rng, lengths, A, T):
    n = int(sum(lengths))
    c = {"lengths": np.array(lengths), "n_actions": np.int64(A), "temperature": np.float64(T),
         "discount": np.float64(DISCOUNT)}
    c["obs"] = rng.randn(n, WIDTH).astype(F32)
    c["Wq"], c["bq"] = (rng.randn(WIDTH, A) * 0.15).astype(F32), (rng.randn(A) * 0.1 + 1.0).astype(F32)
    c["Wr"], c["br"] = (rng.randn(WIDTH, A) * 0.3).astype(F32), (rng.randn(A) * 0.2).astype(F32)
    c["actions"] = rng.randint(0, A, size=n)
    c["rewards"] = rng.randn(n).astype(F32)
    mu = (0.2 / A + 0.8 * rng.dirichlet(np.ones(A), size=n)).astype(F32)
    mu[::2] = F32(1) / F32(A)
    c["mu"] = mu
    c["episode_offsets"] = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return c


def run_reference(c, batch_size):
    A, T = int(c["n_actions"]), float(c["temperature"])
    episodes, transitions, j = [], [], 0
    for L in c["lengths"]:
        ep = Episode(discount=DISCOUNT)
        for t in range(int(L)):
            tr = Transition(state={'observation': c["obs"][j]}, action=int(c["actions"][j]), reward=float(c["rewards"][j]),
                            next_state={'observation': c["obs"][j]}, game_over=t == L - 1,
                            info={'all_action_probabilities': c["mu"][j]})
            ep.insert(tr)
            transitions.append(tr)
            j += 1
        ep.update_discounted_rewards()
        episodes.append(ep)
    head = _Obj(q_values="q_values", softmax="softmax")
    calls = {"q": [], "rm": []}

    def predict_q(states, outputs=None):
        assert outputs == [head.q_values, head.softmax]
        q = linear(np.asarray(states['observation'], dtype=F32), c["Wq"], c["bq"])
        calls["q"].append(q)
        return q, ope_ref.softmax32(q, T)

    def predict_rm(states):
        rm = linear(np.asarray(states['observation'], dtype=F32), c["Wr"], c["br"])
        calls["rm"].append(rm)
        return rm
    m = OpeManager()
    m.gather_static_shared_stats(evaluation_dataset_as_transitions=transitions, batch_size=batch_size,
                                 reward_model=_Obj(predict=predict_rm), network_keys=['observation'])
    est = m.evaluate(evaluation_dataset_as_episodes=episodes, evaluation_dataset_as_transitions=transitions,
                     batch_size=batch_size, discount_factor=DISCOUNT,
                     q_network=_Obj(predict=predict_q, output_heads=[head]), network_keys=['observation'])
    out = {"q": np.concatenate(calls["q"]), "reward_model": np.concatenate(calls["rm"]),
           "returns": np.array([t.n_step_discounted_rewards for t in transitions], dtype=np.float64),
           "ref_estimates": np.array([float(x) for x in est], dtype=np.float64),
           "ref_pi": np.stack([t.info['softmax_policy_prob'] for t in transitions]),
           "ref_v": np.array([t.info['v_value_q_model_based'] for t in transitions])}
    assert tuple(type(est)._fields) == ope_ref.NAMES
    assert np.array_equal(out["q"], linear(c["obs"], c["Wq"], c["bq"]))
    assert np.array_equal(out["reward_model"], linear(c["obs"], c["Wr"], c["br"]))
    return out


def main():
    rng = np.random.RandomState(2107)
    out = {"cases": np.int64(len(CASES))}
    for i, (lengths, A, batch_size, T) in enumerate(CASES):
        c = make_case(rng, lengths, A, T)
        c["batch_size"] = np.int64(batch_size)
        c.update(run_reference(c, batch_size))
        _, _, extras = ope_ref.evaluate(c["q"], c["reward_model"], batch_size, c["actions"], c["rewards"], c["mu"], T,
                                        c["episode_offsets"], c["returns"], DISCOUNT)
        w = extras["ep_w"]
        assert w.max() > 1e-3, "case %d: the largest episode weight is %r" % (i, w.max())
        for k, v in c.items():
            if k not in ("obs", "Wq", "bq", "Wr", "br"):
                out["c%d_%s" % (i, k)] = np.array(v)
        print("case %d (lengths=%s A=%d batch=%d T=%g): n=%d, w_e in [%.3e, %.3e], estimates %s"
              % (i, lengths, A, batch_size, T, sum(lengths), w.min(), w.max(),
                 " ".join("%s=%.6g" % kv for kv in zip(ope_ref.NAMES, c["ref_estimates"]))))
    path = os.path.join(HERE, "ope.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KiB)" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
