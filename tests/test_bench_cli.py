"""bench.py's command line and its --dump-outputs writer, without a GPU (the end-to-end runs are in test_gpu_bench.py)."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _State:
    """Stands in for SagaSolver: get(name) -> the (K, p) / (K, n) / (K,) state arrays."""

    def __init__(self, K, p, n, broadcast=False):
        shapes = {"w": (K, p), "g_sum": (K, p), "g_memory": (K, n), "intercept": (K,), "g_sum_intercept": (K,)}
        if broadcast:                                  # the shapes of the big workloads without their memory
            self.arrays = {k: np.broadcast_to(np.float64(i + 0.5), s) for i, (k, s) in enumerate(shapes.items())}
        else:
            rng = np.random.default_rng(3)
            self.arrays = {k: np.asfortranarray(rng.normal(size=s)) for k, s in shapes.items()}

    def get(self, name):
        return self.arrays[name]


def test_steps_must_be_a_positive_count():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr and "must be >= 1" in r.stderr


def test_dump_writes_every_state_array_in_float64(tmp_path):
    S = _State(3, 50, 400)
    total = bench.dump_outputs(S, str(tmp_path / "out"))
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "out"))
    assert names == sorted(bench.DUMP_STATE)
    for name in names:
        got = np.load(tmp_path / "out" / f"{name}.npy")
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, S.get(name))
    assert total == sum(a.nbytes for a in S.arrays.values())


def test_dump_samples_large_arrays_by_fixed_columns(tmp_path):
    S = _State(3, 50, 5000)
    for d in ("a", "b"):
        bench.dump_outputs(S, str(tmp_path / d), max_entries=4096)
    idx = np.load(tmp_path / "a" / "g_memory_index.npy")
    assert idx.dtype == np.float64 and idx.shape == (4096 // 3,)
    cols = idx.astype(np.int64)
    assert np.all(np.diff(cols) > 0) and cols[0] >= 0 and cols[-1] < 5000 and np.array_equal(cols, idx)
    gm = np.load(tmp_path / "a" / "g_memory.npy")
    np.testing.assert_array_equal(gm, S.get("g_memory")[:, cols])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "w.npy"), S.get("w"))   # small arrays stay whole
    assert not os.path.exists(tmp_path / "a" / "w_index.npy")
    for f in os.listdir(tmp_path / "a"):                                           # the same sample on every run
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_dump_of_every_workload_stays_under_64_mb(tmp_path):
    for name, (n, p, _density, _family, K, _seed) in bench.WORKLOADS.items():
        total = bench.dump_outputs(_State(K, p, n, broadcast=True), str(tmp_path / name))
        on_disk = sum(np.load(tmp_path / name / f).nbytes for f in os.listdir(tmp_path / name))
        assert total == on_disk <= 64 * 2 ** 20, name
