"""bench.py's --dump-outputs writer and its options, on host tensors: float32 files, the 64 MB cap kept by a fixed row sample that
is the same in every run, small outputs written whole."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_outputs_are_written_whole_in_float32(tmp_path):
    t = torch.randn(3, 5, 7, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    written = bench.dump_outputs(str(tmp_path), {"x": t})
    a = np.load(tmp_path / "x.npy")
    assert written == {"x": [3, 5, 7]} and a.dtype == np.float32
    np.testing.assert_array_equal(a, t.float().numpy())


def test_large_outputs_are_a_fixed_row_sample_within_the_budget(tmp_path):
    budget = 1 << 20
    big = torch.arange(4096 * 128, dtype=torch.float32).view(4096, 128)        # 2 MB in float32: over its half of the budget
    small = torch.ones(16, 8, dtype=torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "a"), {"big": big, "small": small}, budget=budget)
    bench.dump_outputs(str(tmp_path / "b"), {"big": big, "small": small}, budget=budget)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    np.testing.assert_array_equal(a, b)
    assert a.shape == (budget // 2 // (4 * 128), 128) and a.dtype == np.float32
    rows = a[:, 0] / 128
    assert (np.diff(rows) > 0).all() and np.array_equal(a, big.numpy()[rows.astype(np.int64)])   # sorted, distinct, whole rows
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= budget + 2 * 128     # (npy headers)


def test_full_is_off_by_default_and_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2", "--dump-outputs", "out"])
    args = bench.parse_args()
    assert args.full is False and args.steps == 4 and args.warmup == 2 and args.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse_args().full is True
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()
