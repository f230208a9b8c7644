"""CPU: bench.py's --full / --dump-outputs plumbing.  A plain run asks for
neither; --steps must be a real step count; dump_outputs writes float32 .npy
files, whole while they fit the byte budget and as a fixed seeded sample
beyond it (the same elements on every run, so two builds compare)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (3, 1)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--steps", "-2"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse(argv)


def test_dump_outputs_whole(tmp_path):
    import torch
    img = np.arange(4 * 5 * 3, dtype=np.float64).reshape(4, 5, 3) / 7
    g = torch.tensor([0.25, -1.5, 3.0])
    bench.dump_outputs(str(tmp_path / "o"), {"image": img, "gradient": g, "absent": None})
    assert sorted(os.listdir(tmp_path / "o")) == ["gradient.npy", "image.npy"]
    a = np.load(tmp_path / "o" / "image.npy")
    assert a.dtype == np.float32 and a.shape == (4, 5, 3)
    np.testing.assert_array_equal(a, img.astype(np.float32))
    np.testing.assert_array_equal(np.load(tmp_path / "o" / "gradient.npy"), g.numpy())


def test_dump_outputs_samples_over_the_budget(tmp_path):
    big = np.random.default_rng(5).random((64, 64, 3)).astype(np.float32)  # 48 KiB
    small = np.array([1.0, 2.0, 3.0], np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"image": big, "gradient": small}, max_bytes=4096)
    a, b = np.load(tmp_path / "a" / "image.npy"), np.load(tmp_path / "b" / "image.npy")
    np.testing.assert_array_equal(a, b)  # the same elements on every run
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "gradient.npy"), small)  # fits: whole
    assert a.ndim == 1 and a.nbytes + small.nbytes <= 4096 and a.size == (4096 - 12) // 4
    idx = np.sort(np.random.default_rng(0).choice(big.size, size=a.size, replace=False))
    np.testing.assert_array_equal(a, big.reshape(-1)[idx])
