"""bench.py's command line and --dump-outputs writer (CPU only; the timed path itself needs a GPU)."""
import sys

import numpy as np
import pytest
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_lean_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full is True and a.dump_outputs == "out"


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_small_is_written_whole(tmp_path):
    t = torch.arange(2 * 4 * 8, dtype=torch.bfloat16).reshape(2, 4, 8)
    bench.dump_outputs(str(tmp_path / "d"), {"embeddings": t})
    got = np.load(tmp_path / "d" / "embeddings.npy")
    assert got.dtype == np.float32 and got.shape == (2, 4, 8)
    assert np.array_equal(got, t.float().numpy())


def test_dump_outputs_large_is_a_fixed_row_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    a = torch.arange(100 * 16, dtype=torch.float32).reshape(100, 16)      # 6400 B
    b = torch.arange(50 * 32, dtype=torch.float32).reshape(50, 32) + 0.5  # 6400 B
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b})
    ga, gb = np.load(tmp_path / "one" / "a.npy"), np.load(tmp_path / "one" / "b.npy")
    assert ga.nbytes + gb.nbytes <= 4096 and ga.shape[0] > 1 and gb.shape[0] > 1
    assert np.array_equal(ga, np.load(tmp_path / "two" / "a.npy"))
    assert np.array_equal(gb, np.load(tmp_path / "two" / "b.npy"))
    rows = (ga[:, 0] / 16).astype(int)                                    # whole rows of a, in order
    assert np.all(np.diff(rows) > 0) and np.array_equal(ga, a.numpy()[rows])
