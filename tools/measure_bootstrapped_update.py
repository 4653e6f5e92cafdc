#!/usr/bin/env python
"""Time one Atari-shaped Bootstrapped DQN update (84 x 84 x 4 frames, A = 6, B = 32, K = 10 heads) against the
Double-DQN update of the same torso, on the GPU.

    python tools/measure_bootstrapped_update.py [--rounds 5] [--replays 300] [--out FILE]
    python tools/measure_bootstrapped_update.py --eager-updates 5        # for a kernel trace: a few eager updates only

Both updates are captured into a graph after a warm-up, as the agents run them, and timed with device events over
`replays` replays per round, the two versions alternating round by round; the spread over the rounds is printed with
the medians.  Launch counts are the library's entry-point calls of one eager update, and the kernels of one eager
update are listed with their own dispatch times (KernelTimer).  Prints one JSON line; fails without a GPU."""
import argparse
import json
import statistics
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def build(kind, dev, A, K, B):
    from coach_amd.nn.networks import BootstrappedDQNNet, DQNNet
    rng = np.random.RandomState(0)
    both = torch.from_numpy(rng.randint(0, 256, size=(2, B, 84, 84, 4)).astype(np.uint8)).to(dev)
    actions = torch.from_numpy(rng.randint(0, A, size=B).astype(np.int32)).to(dev)
    rewards = torch.from_numpy(rng.choice([0.0, 1.0], size=B).astype(np.float32)).to(dev)
    go = torch.from_numpy((rng.rand(B) < 0.1).astype(np.uint8)).to(dev)
    if kind == "bootstrapped":
        net = BootstrappedDQNNet(dev, (84, 84, 4), A, K, seed=1, head_gradient_rescale=1.0 / K)
        masks = torch.full((B,), (1 << K) - 1, dtype=torch.int32, device=dev)
        run = lambda: net.learn_from_batch(both[0], both[1], B, actions, rewards, go, masks, 0.99, states_pair=both)
    else:
        net = DQNNet(dev, (84, 84, 4), A, seed=1)
        run = lambda: net.learn_from_batch(both[0], both[1], B, actions, rewards, go, 0.99, double_dqn=True,
                                           states_pair=both)
    return net, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=300)
    ap.add_argument("--eager-updates", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    from coach_amd import _rlx
    from coach_amd.agents.vector_agent import capture
    dev = torch.device("cuda", 0)
    A, K, B = 6, 10, 32
    runs = {k: build(k, dev, A, K, B) for k in ("bootstrapped", "double_dqn")}
    if args.eager_updates:
        for _, run in runs.values():
            for _ in range(args.eager_updates):
                run()
        torch.cuda.synchronize()
        return
    res = {"shape": dict(obs=[84, 84, 4], actions=A, heads=K, batch=B), "replays_per_round": args.replays}
    graphs = {}
    for name, (net, run) in runs.items():
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        c0 = _rlx.CALL_COUNT
        run()
        launches = _rlx.CALL_COUNT - c0
        with _rlx.KernelTimer() as t:
            run()
        torch.cuda.synchronize()
        graphs[name] = capture(run)
        for _ in range(20):
            graphs[name].replay()
        res[name] = {"library_calls_per_update": launches, "kernels_per_update": len(t.records),
                     "kernel_us_sum": round(sum(us for _, us in t.records), 2),
                     "kernels": [[n.split("(")[0][-48:], round(us, 2)] for n, us in t.records], "us_per_update": []}
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name in ("bootstrapped", "double_dqn"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.replays):
                graphs[name].replay()
            b.record()
            torch.cuda.synchronize()
            res[name]["us_per_update"].append(round(1e3 * a.elapsed_time(b) / args.replays, 2))
    for name in ("bootstrapped", "double_dqn"):
        v = res[name]["us_per_update"]
        res[name]["median_us"], res[name]["min_us"], res[name]["max_us"] = statistics.median(v), min(v), max(v)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
