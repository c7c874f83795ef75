"""bench.py's options on the host: a plain run measures the headline figure only (everything else behind --full), and
--dump-outputs writes float32 / float64 .npy files within its size budget, sampling large arrays at fixed positions."""
import sys

import numpy as np
import pytest
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_leaves_every_extra_measurement_to_full(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.steps == 7 and a.warmup == 2 and a.workload == "cifar20" and a.dump_outputs is None
    assert not a.secondary
    assert a.no_kernel_timing and a.no_train_rate and a.no_cpu_baseline and a.no_one_stream_pass
    f = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2", "--full")
    assert f.secondary
    assert not (f.no_kernel_timing or f.no_train_rate or f.no_cpu_baseline or f.no_one_stream_pass)
    assert not _parse(monkeypatch, "--full", "--workload", "sd256").secondary
    assert _parse(monkeypatch, "--full", "--no-cpu-baseline").no_cpu_baseline


def test_dump_outputs_dtypes_sample_and_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "torch", torch)
    big = torch.randn(bench.DUMP_MAX_ELEMS + 1000, generator=torch.Generator().manual_seed(1))
    arrays = {"loss": torch.tensor([0.25], dtype=torch.float64), "half": torch.ones(2, 3, dtype=torch.bfloat16), "big": big}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert got["loss"].dtype == np.float64 and got["loss"].tolist() == [0.25]
    assert got["half"].dtype == np.float32 and got["half"].shape == (2, 3)
    assert got["big"].dtype == np.float32 and got["big"].shape == (bench.DUMP_MAX_ELEMS,)
    assert np.isin(got["big"], big.numpy()).all()                              # a sample of the array, not new values
    np.testing.assert_array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))      # at the same positions every run
    with pytest.raises(ValueError, match="budget"):
        bench.dump_outputs(str(tmp_path / "c"), {f"x{i}": big for i in range(5)})
    assert not (tmp_path / "c").exists()
