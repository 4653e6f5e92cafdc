#!/usr/bin/env python
"""Generate tests/golden/cil.npz from the REFERENCE's own BalancedExperienceReplay and CILAgent.learn_from_batch under the
stub-import harness (_refstub.py); run from the repo root where the reference tree is present.  Recorded:
  * mem_classes: the class of each of 16 stored transitions (3 classes, max size 10; the reward is the sequence number);
    mem_dup / mem_nodup: the rewards of three batches of 6 after np.random.seed(7), with and without duplicates;
    mem_order, mem_class<c>: transitions_order and each class list's rewards at the end.
    The reference's class does not run as shipped: its store() counts in `_num_transitions`, which nothing defines, and
    first calls ExperienceReplay.store, which appends the transition to `self.transitions` -- here the list of class
    lists.  The recorder supplies the counter (and num_transitions() on it, what the class's own checks mean) and
    makes the base store a no-op; the class's store, sample and _enforce_max_length run as written.
  * cil_predict [K, B, A], cil_commands, cil_actions -> cil_targets: what learn_from_batch hands the training call."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]
import _refstub  # noqa: E402

_refstub.install()
from rl_coach.agents.cil_agent import CILAgent  # noqa: E402
from rl_coach.core_types import Batch, Transition  # noqa: E402
from rl_coach.memories.memory import MemoryGranularity  # noqa: E402
from rl_coach.memories.non_episodic.balanced_experience_replay import BalancedExperienceReplay  # noqa: E402


from rl_coach.memories.non_episodic.experience_replay import ExperienceReplay  # noqa: E402

ExperienceReplay.store = lambda self, transition, lock=True: None


class _Recorded(BalancedExperienceReplay):
    _num_transitions = 0

    def num_transitions(self):
        return self._num_transitions


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def main():
    rng, out = np.random.RandomState(5), {}
    classes = np.concatenate([rng.randint(0, 3, 10), np.tile(np.arange(3), 2)])
    out["mem_classes"] = classes
    for dup in (True, False):
        mem = _Recorded((MemoryGranularity.Transitions, 10), dup, 3, 'class')
        for i, c in enumerate(classes):
            mem.store(Transition(state={'class': int(c)}, action=0, reward=float(i), next_state={'class': 0}))
        np.random.seed(7)
        out["mem_dup" if dup else "mem_nodup"] = np.array([[t.reward for t in mem.sample(6)] for _ in range(3)])
    out["mem_order"] = np.array(mem.transitions_order)
    for c in range(3):
        out["mem_class%d" % c] = np.array([t.reward for t in mem.transitions[c]])
    K, B, A = 4, 6, 2
    predict, commands = rng.randn(K, B, A).astype(np.float32), rng.randint(0, K, B)
    actions, got = rng.randn(B, A).astype(np.float32), {}
    agent = object.__new__(CILAgent)
    agent.ap = _Obj(network_wrappers={'main': _Obj(input_embedders_parameters={'observation': None})},
                    algorithm=_Obj(state_key_with_the_class_index='high_level_command'))
    agent.networks = {'main': _Obj(online_network=_Obj(predict=lambda inputs: [p.copy() for p in predict]),
                                   train_and_sync_networks=lambda inputs, targets: (got.update(t=targets), (0., [0.], [0.]))[1])}
    agent.learn_from_batch(Batch([Transition(state={'observation': np.zeros(3), 'high_level_command': int(c)}, action=a,
                                             next_state={'observation': np.zeros(3), 'high_level_command': 0})
                                  for c, a in zip(commands, actions)]))
    out.update(cil_predict=predict, cil_commands=commands, cil_actions=actions, cil_targets=np.array(got["t"]))
    np.savez(os.path.join(HERE, "cil.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
