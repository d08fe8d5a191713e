"""bench.py's ONE line as the driver sees it (round 6; verdict r05 "missing" 2: the line was > 20 KB, the driver keeps the last 8 KB of stdout, and the product figures of three
BASELINE configurations never reached its record).  The --full run must print exactly one JSON line of at most 7 000 bytes that carries the contract's fields, the roofline and
cpu_baseline objects, and a short measured entry for every BASELINE configuration (ids: profiles/bench_workloads.md)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_default_bench_line_fits_the_drivers_window_and_names_every_baseline_config():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--repeats", "2", "--full"], capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:3]                                   # ONE line on stdout, nothing else
    line = lines[0]
    assert len(line.encode()) <= 7000, len(line)
    j = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["steps"] == 6 and j["warmup"] == 2 and j["n_gpus"] == 1 and j["unit"] == "frames/s" and j["higher_is_better"] is True and j["vs_baseline"] is None
    assert j["config"]["workload"].startswith("C2") and (j["config"]["fft"], j["config"]["hop"], j["config"]["channels"], j["config"]["hops_per_step"]) == (1024, 256, 1, 1 << 20)
    rf = j["roofline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and 0.05 < rf["frac"] < 0.5
    assert rf["algorithmic_bytes_per_launch"] == (1 << 20) * 2 * 256 * 4
    assert abs(rf["achieved"] - rf["algorithmic_bytes_per_launch"] / (rf["kernel_ms"] * 1e-3) / 1e9) < 1e-6 * rf["achieved"]
    assert 2000.0 < rf["copy_gbs_measured"] < 8000.0                      # the device-copy ceiling measured in the same run, beside the 8 TB/s peak
    assert abs(j["value"] - (1 << 20) * 6 / (j["ms_per_step"] * 6e-3)) < 1e-6 * j["value"]
    cb = j["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 1e3 and cb["unit"] == "frames/s"
    ids = [c["id"] for c in j["configs"]]
    for need in ("C3", "C4-share", "C5-sweep", "C5-f1.5", "8ch-1024", "native", "C2-f0.8", "C2-sweep", "N16384"):
        assert need in ids, need
    assert ids.index("C3") < ids.index("C2-fwd64")                        # BASELINE's product configurations first
    for c in j["configs"]:
        assert "err" not in c, c
        assert c["par"] is None or c["par"] < 2e-7, c
    assert j["parity_rms_vs_oracle"] < 2e-7 and 0.0 <= j["fallback_rate"] < 0.1
    assert {h["id"] for h in j["host"]} >= {"C4-share-host", "8ch-1024-host"} and all(h.get("bit_equal", True) for h in j["host"])
    assert set(j["latency_us"]) == {"C5-launch", "C5-resident", "C2-launch", "C2-resident"}
    assert os.path.exists(os.path.join(ROOT, j["legend"]))


def _plain(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:3]
    return json.loads(lines[0])


def test_the_plain_bench_line_times_exactly_steps_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain run (no --full) measures the headline only: ONE timed region of exactly --steps launches, none of the --full figures, and --dump-outputs
    writes a fixed sample of the last step's output that is identical from run to run (seeded input, state reset before warm-up)."""
    import numpy as np
    a, b = _plain(tmp_path / "a"), _plain(tmp_path / "b")
    for j in (a, b):
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "roofline"):
            assert k in j, k
        assert j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "frames/s" and j["higher_is_better"] is True
        assert j["roofline"]["regions"] == 1 and j["roofline"]["copy_gbs_measured"] is None and j["parity_rms_vs_oracle"] is None
        assert not {"configs", "host", "latency_us", "cpu_baseline"} & set(j)
        assert abs(j["value"] - (1 << 20) * 3 / (j["ms_per_step"] * 3e-3)) < 1e-6 * j["value"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["output_sample.npy", "output_sample_offsets.npy"] and sorted(os.listdir(tmp_path / "b")) == names
    ya, yb = np.load(tmp_path / "a" / "output_sample.npy"), np.load(tmp_path / "b" / "output_sample.npy")
    assert ya.dtype == np.float32 and ya.shape == (2048, 4096) and np.all(np.isfinite(ya)) and float(np.sqrt(np.mean(ya.astype(np.float64) ** 2))) > 1e-3
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32))
    assert np.array_equal(np.load(tmp_path / "a" / "output_sample_offsets.npy"), np.load(tmp_path / "b" / "output_sample_offsets.npy"))
