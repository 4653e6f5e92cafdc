"""Writes tests/golden/default_param_lists.json: for the networks the epsilon-greedy DQN-family agents build, every
parameter's name, offset in the flat buffer, shape, towers and tower stride, in buffer order, and the buffer's size.
Run from the root of a checkout of the commit whose networks are to be recorded (the file in git was written from the
commit before the noisy layers existed); needs the built library but no GPU: the Adam slots, the only part of a
network's construction that launches a kernel, are left out.

    python tests/golden/make_default_param_lists.py OUT.json"""
import json
import sys

import torch

CASES = {
    "dqn_vector": ("DQNNet", ((6,), 3), {}),
    "dqn_image": ("DQNNet", ((84, 84, 4), 3), {}),
    "dqn_dueling_vector": ("DQNNet", ((6,), 3), {"dueling": True}),
    "dqn_dueling_image": ("DQNNet", ((84, 84, 4), 3), {"dueling": True}),
    "qr_dqn_vector": ("QRDQNNet", ((6,), 3, 11), {}),
    "c51_vector": ("C51Net", ((6,), 3, 11), {}),
    "c51_image": ("C51Net", ((84, 84, 4), 6, 51), {}),
}


def describe(device, adam_stub=False):
    from coach_amd.nn import graph as G
    from coach_amd.nn import networks as N
    if adam_stub:
        class _NoAdam(object):
            one_launch = True

            def __init__(self, *a, **k):
                pass
        G.AdamState = _NoAdam
    out = {}
    for case, (cls, args, kw) in CASES.items():
        net = getattr(N, cls)(device, *args, **kw)
        entries = sorted(net.params.entries.items(), key=lambda e: e[1][0])
        out[case] = {"size": int(net.params.size),
                     "entries": [[name, int(off), list(shape), int(towers), int(stride)]
                                 for name, (off, shape, towers, stride) in entries]}
    return out


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.getcwd())
    with open(sys.argv[1], "w") as f:
        json.dump(describe(torch.device("cpu"), adam_stub=True), f, indent=1, sort_keys=True)
