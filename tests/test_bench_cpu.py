"""bench.py --dump-outputs: what it writes, without a GPU."""
import os

import numpy as np

import bench


def test_dump_outputs_writes_every_array_as_float64(tmp_path):
    x = np.arange(12.0).reshape(4, 3)
    success = np.array([True, False, True, True])
    iters = np.array([3, 4, 5, 6], dtype=np.int32)
    bench.dump_outputs(str(tmp_path / "out"), dict(x=x, success=success, sqp_iters=iters))
    assert sorted(os.listdir(tmp_path / "out")) == ["sqp_iters.npy", "success.npy", "x.npy"]
    for name, want in (("x", x), ("success", success), ("sqp_iters", iters)):
        got = np.load(tmp_path / "out" / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64))


def test_dump_outputs_above_the_cap_keeps_the_same_seeded_rows_of_every_array(tmp_path):
    n = 1000
    x = np.arange(n * 8, dtype=np.float64).reshape(n, 8)
    records = np.arange(n + 500, dtype=np.float64)          # gathered over all ranks: rank 0's problems come first
    cap = 100 * (8 + 8 * 8 + 8)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), dict(x=x, records=records), cap=cap)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert len(idx) == 100 and np.all(np.diff(idx) > 0) and idx.max() < n
    assert total <= cap + 3 * 128                            # + the .npy headers
    assert np.array_equal(np.load(tmp_path / "a" / "x.npy"), x[idx.astype(int)])
    assert np.array_equal(np.load(tmp_path / "a" / "records.npy"), records[idx.astype(int)])
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))

