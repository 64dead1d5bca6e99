"""bench.dump_outputs (``bench.py --dump-outputs DIR``): every output as float32 / float64 ``.npy``, a large
array as the same seeded sample of its rows in every run, at most 64 MB in all."""

import numpy as np
import pytest
import torch

import bench


def test_small_outputs_are_written_whole(tmp_path):
    g = torch.arange(12, dtype=torch.float32).reshape(3, 4).requires_grad_(True)
    named = {"grad_n": g, "loss": torch.tensor(2.5, dtype=torch.float64), "count": torch.arange(5),
             "geometry_depth_mean": np.arange(4, dtype=np.float64), "absent": None}
    bench.dump_outputs(tmp_path / "out", named)
    got = {p.stem: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert sorted(got) == ["count", "geometry_depth_mean", "grad_n", "loss"]
    assert got["grad_n"].dtype == np.float32 and np.array_equal(got["grad_n"], g.detach().numpy())
    assert got["loss"].dtype == np.float64 and got["loss"].shape == () and got["loss"] == 2.5
    assert got["count"].dtype == np.float32 and np.array_equal(got["count"], np.arange(5))
    assert got["geometry_depth_mean"].dtype == np.float64


def test_a_large_output_is_the_same_row_sample_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ARRAY_BYTES", 64 * 10 * 4)  # 64 rows of 10 float32
    x = torch.arange(1000 * 10, dtype=torch.float32).reshape(1000, 10)
    bench.dump_outputs(tmp_path / "a", {"runoff": x}, ".rank1")
    bench.dump_outputs(tmp_path / "b", {"runoff": x.clone()}, ".rank1")
    a, b = np.load(tmp_path / "a" / "runoff.rank1.npy"), np.load(tmp_path / "b" / "runoff.rank1.npy")
    assert a.shape == (64, 10) and np.array_equal(a, b)
    rows = (a[:, 0] / 10).astype(np.int64)
    assert np.all(np.diff(rows) > 0) and rows.max() > 64  # distinct rows of the whole array, in ascending order
    assert np.array_equal(a, x.numpy()[rows])


def test_the_total_is_bounded(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_TOTAL_BYTES", 100)
    with pytest.raises(RuntimeError, match="more than 100 bytes"):
        bench.dump_outputs(tmp_path, {"a": torch.zeros(20), "b": torch.zeros(20)})
