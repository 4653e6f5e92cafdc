"""Kernel times of one dense layer's forward and backward pass, fp32 (the launches G.Dense makes by default) against
precision="bf16" (csrc/gemm_bf16.hip), per launch, from the library's in-process kernel timer (the dispatch's own begin /
end timestamps).  The two precisions alternate inside one process; every shape is warmed first; medians over --reps.

    python tools/bench_dense_bf16.py [--reps 200]          (needs the GPU; prints one table)
"""
import argparse
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(64, 3136, 512), (256, 376, 256), (32, 4, 512)]      # (M, K, N): the image DQN's FC layer, TD3's, CartPole's


def main():
    import torch
    from coach_amd import _rlx
    from coach_amd.nn import graph as G
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    reps = ap.parse_args().reps
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a CPU run cannot time anything")
    dev = torch.device("cuda:0")
    ctx, rng = G.Context(dev), np.random.RandomState(0)
    print("| M, K, N | pass | fp32: launches (us) | fp32 total us | bf16: launches (us) | bf16 total us |")
    print("|---|---|---|---|---|---|")
    for M, K, N in SHAPES:
        x = G.Tensor(torch.from_numpy(rng.randn(1, M, K).astype(np.float32)).to(dev), M, K, 1)
        layers, times = {}, {}
        for prec in G.PRECISIONS:
            params = G.FlatParams()
            layers[prec] = G.Dense(params, "layer_" + prec, K, N, "relu", precision=prec)
            params.finalize(dev)
            layers[prec].initialize(rng)
            times[prec] = {"forward": collections.defaultdict(list), "backward": collections.defaultdict(list)}

        def one(prec, record):
            l, passes = layers[prec], {}
            with _rlx.KernelTimer(64) as t:
                y = l.forward(ctx, x, tag=prec)
            passes["forward"] = t.records
            y.ensure_grad().fill_(1e-3)
            y.grad_is_dz = False
            with _rlx.KernelTimer(64) as t:
                l.backward(ctx, x, y)
            passes["backward"] = t.records
            if record:
                for p, recs in passes.items():
                    for i, (name, us) in enumerate(recs):
                        times[prec][p]["%d %s" % (i, name.split("<")[0].split("::")[-1])].append(us)
        for rep in range(-10, reps):                 # ten warm-up rounds, then alternate the two precisions
            for prec in G.PRECISIONS:
                one(prec, rep >= 0)
        for p in ("forward", "backward"):
            cells = []
            for prec in G.PRECISIONS:
                med = {k: float(np.median(v)) for k, v in times[prec][p].items()}
                cells += [", ".join("%s %.1f" % (k.split(" ", 1)[1], v) for k, v in sorted(med.items())),
                          "%.1f" % sum(med.values())]
            print("| %d, %d, %d | %s | %s |" % (M, K, N, p, " | ".join(cells)))


if __name__ == "__main__":
    main()
