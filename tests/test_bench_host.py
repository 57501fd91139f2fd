"""bench.py without a GPU: the options of a plain run and --full, and what --dump-outputs writes."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def _outputs():
    return (torch.arange(600, dtype=torch.float32).reshape(2, 3, 10, 10), torch.full((2, 2, 10, 10), -1.0),
            (torch.tensor([1.5]), torch.tensor([2.5], dtype=torch.float64)),
            (torch.ones(2, 4, 4, 8, dtype=torch.float16), torch.ones(2, 4, 4, 8)))


NAMES = ("rgb", "op", "rgb_diff", "op_diff", "rgb_q", "op_q")


def test_plain_run_is_lean_by_default(monkeypatch):
    b = _bench()
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = b.parse()
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None and a.mode == "infer"
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float32_arrays_whole(tmp_path):
    b = _bench()
    b.dump_outputs(str(tmp_path), _outputs())
    got = {n: np.load(tmp_path / f"{n}.npy") for n in NAMES}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["rgb"].shape == (2, 3, 10, 10) and np.array_equal(got["rgb"].reshape(-1), np.arange(600, dtype=np.float32))
    assert got["op_diff"].tolist() == [2.5] and got["rgb_q"].shape == (2, 4, 4, 8)


def test_dump_outputs_samples_within_its_budget(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 1000)           # 1514 entries = 6056 bytes: every 7th entry fits
    b.dump_outputs(str(tmp_path), _outputs())
    got = {n: np.load(tmp_path / f"{n}.npy") for n in NAMES}
    assert sum(a.nbytes for a in got.values()) <= 1000
    assert np.array_equal(got["rgb"], np.arange(600, dtype=np.float32)[::7])
    assert got["op"].size == 58 and got["rgb_diff"].tolist() == [1.5]


def test_dump_outputs_is_refused_outside_the_infer_mode(monkeypatch):
    b = _bench()
    monkeypatch.setattr("sys.argv", ["bench.py", "--mode", "train", "--dump-outputs", "d"])
    with pytest.raises(SystemExit, match="infer"):
        b.main()
