"""bench.py --dump-outputs DIR writes what the timed path computed as DIR/<name>.npy (float32), 64 MB at most in all: a tensor
past the budget is replaced by a fixed, seeded sample of its elements.  The writer is host code and is checked here without a GPU."""
import importlib.util
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("umfa_bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_headline_output_fits_the_budget_whole():
    b = _bench()
    assert b.B * b.H * b.S * b.D * 4 <= b.DUMP_LIMIT_BYTES == 64 << 20  # the fp32 O of the FLUX problem is written in full


def test_dump_writes_float32_npy_whole_under_the_budget(tmp_path):
    b = _bench()
    o = torch.randn(2, 3, 5, 7, dtype=torch.bfloat16)
    b.dump_outputs(str(tmp_path / "out"), {"o": o})
    got = np.load(tmp_path / "out" / "o.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 5, 7)
    assert np.array_equal(got, o.float().numpy())


def test_dump_samples_past_the_budget_the_same_way_every_run(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 1200)
    big = torch.arange(4096, dtype=torch.float32).reshape(64, 64)
    for run in ("a", "b"):
        b.dump_outputs(str(tmp_path / run), {"big": big})
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["big_sample.npy", "big_sample_index.npy"]
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= 1200 + 2 * 128  # (+ two .npy headers)
    vals, idx = np.load(tmp_path / "a" / "big_sample.npy"), np.load(tmp_path / "a" / "big_sample_index.npy")
    assert vals.dtype == np.float32 and np.array_equal(vals, big.numpy().reshape(-1)[idx])
    assert np.array_equal(idx, np.load(tmp_path / "b" / "big_sample_index.npy"))
