"""bench.py's own options, host only: --steps / --warmup are checked, --full is off by default, and --dump-outputs writes the last
step's loss, gradients and parameters as float32 / float64 .npy files within 64 MB, the same from run to run (oracle blocks on CPU:
the device path is what bench.py itself runs)."""
import os
import sys

import numpy as np
import pytest
import torch

import bench
from oracle import spectral_oracle as so
from uno_amd.harness import DarcyTrainer, UNO_9, synthetic_darcy_batch


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default_and_steps_are_checked(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert _parse(monkeypatch, "--full", "--dump-outputs", "d").full
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def _dump(path):
    torch.manual_seed(0)
    tr = DarcyTrainer(UNO_9(3, 4, pad=5, block_cls=so.OracleOperatorBlock2d), lr=1e-3, weight_decay=1e-3)
    a, u = synthetic_darcy_batch(2, 72, 1234, "cpu")
    for _ in range(2):
        loss = tr.step(a, u)
    bench.dump_outputs(str(path), loss, tr)
    n = sum(p.numel() * (2 if p.is_complex() else 1) for p in tr.model.parameters())
    return float(loss), n


def test_dump_outputs_sampled_and_repeatable(tmp_path, monkeypatch):
    assert 2 * bench.DUMP_SAMPLE * 4 + 8 <= 64 << 20
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)           # the model below is larger: the sampled branch
    loss, n = _dump(tmp_path / "a")
    _dump(tmp_path / "b")
    assert n > 1000
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grad_sample.npy", "loss.npy", "param_sample.npy"]
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all()
        assert np.array_equal(x, y), f
    assert np.load(tmp_path / "a" / "loss.npy")[0] == loss
    assert np.load(tmp_path / "a" / "param_sample.npy").shape == (1000,)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1 << 22)        # smaller than the sample: written whole
    _dump(tmp_path / "c")
    assert np.load(tmp_path / "c" / "param_sample.npy").shape == (n,)
