"""`python bench.py --gpus N` from a bare shell must launch its own N ranks: the entry
point re-executes itself under torch.distributed.run on 127.0.0.1.  CPU flavour: --dry-run (gloo, no
kernels) exercises the launcher, the rendezvous, the barrier-bracketed timing, max-over-ranks /
sum-over-ranks and the single JSON line from rank 0."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "3", "--warmup", "1"] + extra,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


def test_bare_shell_two_ranks():
    out = _run(["--gpus", "2"])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1
    assert out["allreduce_check"] == 1.0            # sum over 2 ranks / 2
    assert out["value"] > 0 and out["scaling"] == "weak"


def test_single_rank_needs_no_launcher():
    out = _run([])
    assert out["n_gpus"] == 1


def test_dump_outputs_writes_float_npy_files_within_the_size_limit(tmp_path, monkeypatch):
    """--dump-outputs: every network's online weights and the step's results as DIR/<name>.npy in float32 / float64;
    past the size limit an array becomes a fixed, seeded sample (identical from call to call)."""
    import types

    import numpy as np
    import torch
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench

    w = torch.arange(50000, dtype=torch.float32)
    agent = types.SimpleNamespace(networks={"main": types.SimpleNamespace(params=types.SimpleNamespace(weights=w))})
    losses = torch.ones(10, 8, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "a"), agent, {"epoch_losses": losses, "count": torch.tensor([3], dtype=torch.int32)})
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "weights_main.npy"), w.numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "epoch_losses.npy"), losses.numpy())
    assert np.load(tmp_path / "a" / "count.npy").dtype == np.float32
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), agent, {"epoch_losses": losses})
    total = sum(os.path.getsize(p) - 128 for p in (tmp_path / "b").iterdir())      # less the .npy headers
    assert total <= 64 << 10
    b, c = np.load(tmp_path / "b" / "weights_main.npy"), np.load(tmp_path / "c" / "weights_main.npy")
    assert 0 < b.size < w.numel() and np.array_equal(b, c) and np.all(np.diff(b) > 0)
