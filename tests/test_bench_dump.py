"""bench.py --dump-outputs, the writer itself (CPU tensors: no GPU needed): a small output is written whole, a large one as a fixed, seeded sample of
windows whose offsets are written next to it; float32 only, within the size bound."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_output_is_written_whole(tmp_path):
    import torch
    y = torch.arange(2 * 1000, dtype=torch.float32).reshape(2, 1000) / 7
    bench.dump_outputs(torch, y, str(tmp_path))
    assert os.listdir(tmp_path) == ["output.npy"]
    got = np.load(tmp_path / "output.npy")
    assert got.dtype == np.float32 and np.array_equal(got, y.numpy())


def test_large_output_is_a_fixed_sample_with_its_offsets(tmp_path):
    import torch
    n = bench.DUMP_SAMPLES * 4 + 123
    y = torch.arange(n, dtype=torch.float64).reshape(1, n).to(torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(torch, y, str(tmp_path / d))
    s, off = np.load(tmp_path / "a" / "output_sample.npy"), np.load(tmp_path / "a" / "output_sample_offsets.npy")
    assert s.dtype == np.float32 and off.dtype == np.float64
    assert s.shape == (bench.DUMP_SAMPLES // bench.DUMP_WINDOW, bench.DUMP_WINDOW) and s.nbytes + off.nbytes <= 64 << 20
    assert np.all(np.diff(off) >= bench.DUMP_WINDOW) and off[-1] + bench.DUMP_WINDOW <= n and np.all(off % bench.DUMP_WINDOW == 0)
    flat = y.reshape(-1).numpy()
    for i in (0, len(off) // 2, len(off) - 1):
        assert np.array_equal(s[i], flat[int(off[i]):int(off[i]) + bench.DUMP_WINDOW])
    assert np.array_equal(s, np.load(tmp_path / "b" / "output_sample.npy")) and np.array_equal(off, np.load(tmp_path / "b" / "output_sample_offsets.npy"))
