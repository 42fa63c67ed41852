"""bench.py --dump-outputs on CPU: what the writer keeps of the timed leg's last control step (the GPU run itself: tests/test_gpu_bench_contract.py)."""
import os

import numpy as np

import bench


def _arrays(n):
    return {"obs": np.arange(n * 49, dtype=np.float32).reshape(n, 49), "done": (np.arange(n) % 3 == 0).astype(np.float32),
            "gc": np.linspace(-1, 1, n * 19, dtype=np.float32).reshape(n, 19)}


def test_dump_outputs_writes_every_array_whole_under_the_budget(tmp_path):
    a = _arrays(64)
    shapes = bench.dump_outputs(str(tmp_path / "out"), a)
    assert shapes == {"obs": [64, 49], "done": [64], "gc": [64, 19]}
    assert sorted(os.listdir(tmp_path / "out")) == ["done.npy", "gc.npy", "obs.npy"]
    for k, v in a.items():
        got = np.load(tmp_path / "out" / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, v), k


def test_dump_outputs_keeps_one_seeded_sample_of_envs_above_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 16384)
    a = _arrays(1000)
    first = bench.dump_outputs(str(tmp_path / "a"), a)
    again = bench.dump_outputs(str(tmp_path / "b"), a)
    assert first == again
    idx = np.load(tmp_path / "a" / "env_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(tmp_path / "b" / "env_index.npy"))
    rows = idx.astype(np.int64)
    assert len(rows) > 0 and np.all(np.diff(rows) > 0) and rows[-1] < 1000          # distinct envs, in order
    total = 0
    for k, v in a.items():
        got = np.load(tmp_path / "a" / f"{k}.npy")
        assert np.array_equal(got, v[rows]), k           # the same envs from every array
        total += got.nbytes
    assert total + idx.nbytes <= 16384
