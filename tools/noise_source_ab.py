"""A/B of the TD3 / SAC noise source (VectorOffPolicyAgent.NOISE_SOURCE): `bench.py --workload c5` and `--workload c4`,
once with the host's np.random normals ("host", the default) and once with the device generator ("device",
rlx_normal_fill).  Every run is a child process of its own under its own time limit; the first failure stops the tool.
bench.py itself is not changed: the child sets the class attribute, then runs bench.py as __main__.

    python tools/noise_source_ab.py [--steps 10 --warmup 3 --full] [--out profiles/noise_source_ab.jsonl]

Prints, and writes to --out, one JSON line per workload holding both modes' bench lines side by side."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = """
import os, runpy, sys
root, mode = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
from coach_amd.agents.vector_agent import VectorOffPolicyAgent
VectorOffPolicyAgent.NOISE_SOURCE = mode
sys.argv = [os.path.join(root, "bench.py")] + sys.argv[3:]
runpy.run_path(sys.argv[0], run_name="__main__")
"""


def run_bench(workload, mode, args):
    cmd = [sys.executable, "-c", _CHILD, ROOT, mode, "--gpus", "1", "--workload", workload,
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    if args.full:
        cmd += ["--full", "--no-cpu-baseline"]
    res = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=args.timeout)
    if res.returncode != 0:
        sys.stderr.write(res.stderr[-4000:])
        raise SystemExit("bench.py --workload %s with NOISE_SOURCE=%r failed (exit %d)" % (workload, mode, res.returncode))
    for line in reversed(res.stdout.strip().splitlines()):
        try:
            return json.loads(line)
        except ValueError:
            continue
    raise SystemExit("bench.py --workload %s (%s) printed no JSON line" % (workload, mode))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c5,c4")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="bench.py --full (roofline: host_draws_us_per_update), no CPU baseline")
    ap.add_argument("--timeout", type=float, default=900.0, help="seconds per bench run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for w in args.workloads.split(","):
        res = {m: run_bench(w, m, args) for m in ("host", "device")}
        h, d = res["host"]["value"], res["device"]["value"]
        line = {"workload": w, "host": res["host"], "device": res["device"], "device_over_host": round(d / h, 4)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
