"""bench.py's --dump-outputs writer (bench.dump_outputs) on CPU tensors: dtypes, names, the size cap and its seeded sample."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_writes_float32_and_keeps_float64(tmp_path):
    import bench
    logits = torch.randn(32, 40).half()
    bench.dump_outputs(str(tmp_path), {"loss": torch.tensor(2.5), "logits": logits, "param.w": torch.randn(7, dtype=torch.float64)})
    assert sorted(os.listdir(tmp_path)) == ["logits.npy", "loss.npy", "param.w.npy"]
    got = np.load(tmp_path / "logits.npy")
    assert got.dtype == np.float32 and got.shape == (32, 40) and np.array_equal(got, logits.float().numpy())
    assert np.load(tmp_path / "loss.npy").dtype == np.float32 and float(np.load(tmp_path / "loss.npy")) == 2.5
    assert np.load(tmp_path / "param.w.npy").dtype == np.float64


def test_dump_outputs_samples_the_same_positions_over_the_cap(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    big = torch.arange(10000, dtype=torch.float32).view(100, 100)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"loss": torch.tensor(1.0), "logits": big})
        assert sorted(os.listdir(tmp_path / d)) == ["logits_sample.npy", "loss.npy"]
    a, b = np.load(tmp_path / "a" / "logits_sample.npy"), np.load(tmp_path / "b" / "logits_sample.npy")
    assert np.array_equal(a, b) and a.nbytes <= 4096 // 2 and a.size > 0
    assert np.all(np.diff(a) > 0)                     # sorted distinct flat positions (the values here are the positions)
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a")) <= 4096
