"""bench.py's multi-rank path end to end on CPU: ``--gpus 2`` with no
torchrun environment makes bench.py start ``torch.distributed.run`` itself as a
child process; the two ranks (gloo) run the ChunkPipeline baton ring on a toy
model and rank 0 prints the one JSON line, with n_gpus = 2 and outputs equal to
the one-rank run (the driver's N = 1, 2, 4, 8 scaling command takes this path;
run_model.py:472 is the reference's DDP launch)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "selftest", "--steps", "2",
                        "--warmup", "1", "--seq-frames", "44", "--frames", "6", "--overlap", "2", *argv],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


def test_bench_launches_ranks_itself():
    one = _bench("--gpus", "1")
    two = _bench("--gpus", "2")
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert two["value"] > 0 and two["steps"] == 2
    for k, v in one["checksum"].items():
        assert abs(two["checksum"][k] - v) <= 1e-6 * max(1.0, abs(v)), (k, v, two["checksum"][k])


def test_dump_outputs_writes_last_step_arrays(tmp_path):
    """--dump-outputs DIR leaves the last timed step's arrays as DIR/<name>.npy
    (float32): one file per output the line's checksum names, summing to it;
    --full is accepted beside it."""
    import numpy as np
    a = str(tmp_path / "a")
    one = _bench("--gpus", "1", "--full", "--dump-outputs", a)
    assert sorted(os.listdir(a)) == sorted(k + ".npy" for k in one["checksum"])
    for k, v in one["checksum"].items():
        x = np.load(os.path.join(a, k + ".npy"))
        assert x.dtype == np.float32 and x.size > 0
        assert abs(float(x.astype(np.float64).sum()) - v) <= 1e-5 * max(1.0, abs(v)), (k, v)


def test_dump_outputs_samples_large_arrays(tmp_path, monkeypatch):
    """Past the byte budget every array larger than its share is cut to a fixed
    seeded sample: same indices on every call, values taken from the array."""
    import numpy as np
    import torch
    import bench  # the repository root is on sys.path (conftest.py)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 100)
    big = torch.arange(1000, dtype=torch.float64).reshape(10, 100)
    outs = {"big": big, "pair": [torch.ones(3), torch.zeros(2, 2)], "skipped": None}
    assert bench.dump_outputs(str(tmp_path), outs) == ["big", "pair_0", "pair_1"]
    got = np.load(tmp_path / "big.npy")
    assert got.dtype == np.float32 and got.shape == (33,)
    assert np.all(np.diff(got) >= 0) and set(got.tolist()) <= set(range(1000))
    assert np.load(tmp_path / "pair_1.npy").shape == (2, 2)
    bench.dump_outputs(str(tmp_path / "again"), outs)
    assert np.array_equal(got, np.load(tmp_path / "again" / "big.npy"))
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith(".npy"))
    assert total <= 4 * 100 + 3 * 128  # the data within the budget, plus one .npy header each
