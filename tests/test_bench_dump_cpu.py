"""bench.py --dump-outputs without a GPU: dump_outputs() writes every array in its own precision, keeps the whole set under the
size bound by a fixed row sample of the two-dimensional arrays, and writes the same files every time."""
import os

import numpy as np
import pytest

import bench


def _arrays():
    rng = np.random.default_rng(7)
    return dict(W_T=rng.random((300, 16)).astype(np.float32), H=rng.random((2000, 16)).astype(np.float32),
                d=rng.random(16).astype(np.float32), loss=np.array([1.25], np.float64))


def _read(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_small_outputs_are_written_whole(tmp_path):
    a = _arrays()
    bench.dump_outputs(str(tmp_path), a)
    got = _read(str(tmp_path))
    assert sorted(got) == sorted(a)
    for name, v in a.items():
        assert got[name].dtype == v.dtype and np.array_equal(got[name], v)


def test_large_outputs_keep_a_fixed_row_sample_within_the_bound(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 60000)
    a = _arrays()
    for run in ("one", "two"):
        bench.dump_outputs(str(tmp_path / run), a)
    one, two = _read(str(tmp_path / "one")), _read(str(tmp_path / "two"))
    assert sorted(one) == sorted(two) == ["H", "H_rows", "W_T", "W_T_rows", "d", "loss"]
    assert sum(os.path.getsize(str(tmp_path / "one" / f)) for f in os.listdir(str(tmp_path / "one"))) <= 60000
    for name in one:
        assert np.array_equal(one[name], two[name])
    for name in ("W_T", "H"):
        rows = one[name + "_rows"]
        assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and 0 < len(rows) < a[name].shape[0]
        assert np.array_equal(one[name], a[name][rows.astype(np.int64)])
    assert np.array_equal(one["d"], a["d"]) and np.array_equal(one["loss"], a["loss"])


def test_only_floating_outputs(tmp_path):
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path), dict(iterations=np.arange(3)))
