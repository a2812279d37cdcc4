"""bench.py --dump-outputs, host side: what the last timed step returned goes to <name>.npy as float64, within the size
limit (a larger gradient: a fixed seeded sample of its rows, with their indices)."""
import os

import numpy as np

import bench


def _llgrad_like(n, dx, ncov):
    rng = np.random.RandomState(5)
    return [float(rng.randn()), rng.randn(n, dx), rng.randn(1, ncov) if ncov else np.zeros((0, 0))]


def test_dump_writes_every_array_as_float64(tmp_path):
    out = _llgrad_like(300, 2, 4)
    shapes = bench.dump_outputs(str(tmp_path / "d"), out)
    assert shapes == {"ll": [1], "grad_X": [300, 2], "grad_cov": [1, 4]}
    assert sorted(os.listdir(str(tmp_path / "d"))) == ["grad_X.npy", "grad_cov.npy", "ll.npy"]
    for name, ref in (("ll", np.array([out[0]])), ("grad_X", out[1]), ("grad_cov", out[2])):
        a = np.load(str(tmp_path / "d" / (name + ".npy")))
        assert a.dtype == np.float64 and np.array_equal(a, ref)


def test_dump_without_grad_cov_writes_no_empty_file(tmp_path):
    assert bench.dump_outputs(str(tmp_path), _llgrad_like(10, 3, 0)) == {"ll": [1], "grad_X": [10, 3]}
    assert not os.path.exists(str(tmp_path / "grad_cov.npy"))


def test_dump_over_the_limit_is_a_fixed_row_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    out = _llgrad_like(1000, 2, 0)
    files = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out)
        files.append({f: np.load(str(tmp_path / d / f)) for f in os.listdir(str(tmp_path / d))})
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) - 128 for f in files[0]) <= 4096      # (128: the .npy header)
    rows = files[0]["grad_X_rows.npy"].astype(np.int64)
    assert len(rows) > 100 and np.all(np.diff(rows) > 0)
    assert np.array_equal(files[0]["grad_X.npy"], out[1][rows])
    assert all(np.array_equal(files[0][f], files[1][f]) for f in files[0])          # seeded: the same sample every time
