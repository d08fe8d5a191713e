"""GPU checks of the phase-locked time stretch (TimeStretch / pv_stretch_*): parity with the CPU model (tests/stretch_model.py), stretch 1 against the
pitch shifter at pitchFactor 1, the bit-exact invariances the integer phase state promises, robustness to non-finite input, and the C99 example."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import signals as S
from stretch_model import StretchModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# hs / ha = 0.5, 0.8, 1.25, 2 at a quarter-frame scale
RATIOS = {0.5: (4, 8), 0.8: (32 / 5, 8), 1.25: (4, 16 / 5), 2.0: (8, 4)}


def _hops(N, r):
    a, s = RATIOS[r]
    return int(round(N / a)), int(round(N / s))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def _signal(nch, n):
    return np.stack([S.make_signal("tonal" if c % 2 == 0 else "noise", c, n) for c in range(nch)])


@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096, 8192])
@pytest.mark.parametrize("ratio", [0.5, 0.8, 1.25, 2.0])
@pytest.mark.parametrize("nch", [1, 8])
def test_model_parity(N, ratio, nch, record_property):
    import phaze_amd
    ha, hs = _hops(N, ratio)
    assert abs(hs / ha - ratio) < 1e-9
    T = 40 if N >= 4096 else 64
    x = _signal(nch, T * ha)
    ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=nch, max_frames=T)
    y = ts.process(x)
    ts.close()
    ref = StretchModel(N, ha, hs, nch).process(x)
    assert y.shape == ref.shape == (nch, T * hs)
    worst = max(_rel(y[c], ref[c]) for c in range(nch))
    record_property("rel", worst)
    assert worst <= 5e-7, worst                                       # measured <= 1.3e-7 on one MI355X


@pytest.mark.parametrize("N,hop", [(1024, 256), (2048, 128)])
def test_stretch_one_matches_pitch_factor_one(N, hop):
    import phaze_amd
    T = 400
    x = _signal(2, T * hop)
    ts = phaze_amd.TimeStretch(N, hop, hop, max_channels=2, max_frames=T)
    y = ts.process(x)
    ts.close()
    pv = phaze_amd.PhaseVocoder(fft_size=N, hop_size=hop, max_channels=2, max_hops=T)
    ref = pv.process_batch(x, np.ones(T, np.float32))
    pv.close()
    assert _rel(y, ref) <= 1e-6


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_bit_exact_invariances():
    import phaze_amd
    import torch
    N, ha, hs = 1024, 256, 320
    T = 1 << 16
    x = S.make_signal("tonal", 0, T * ha)[None, :]
    ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=8, max_frames=T)
    one = ts.process(x)
    # repeated run from reset
    ts.reset()
    assert np.array_equal(_bits(ts.process(x)), _bits(one))
    # 7 irregular calls
    ts.reset()
    cuts = [0, 1, 5, 300, 4097, 20000, 20001, T]
    parts = [ts.process(x[:, a * ha:b * ha]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(one))
    # frame by frame (first 300 frames)
    ts.reset()
    fb = [ts.process(x[:, m * ha:(m + 1) * ha]) for m in range(300)]
    assert np.array_equal(_bits(np.concatenate(fb, axis=1)), _bits(one[:, :300 * hs]))
    # device pointers
    ts.reset()
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.empty((1, T * hs), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ts.process_device(d_in.data_ptr(), d_out.data_ptr(), 1, T, T * ha, T * hs)
    ts.synchronize()
    assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(one))
    # export after call k, import into a fresh handle on another channel slot, continue
    ts.reset()
    k = 777
    a = ts.process(x[:, :k * ha])
    st = ts.export_state(0)
    ts2 = phaze_amd.TimeStretch(N, ha, hs, max_channels=4, max_frames=T)
    ts2.import_state(3, *st)
    xb = np.zeros((4, (T - k) * ha), np.float32)
    xb[3] = x[0, k * ha:]
    b = ts2.process(xb)[3:4]
    assert np.array_equal(_bits(np.concatenate([a, b], axis=1)), _bits(one))
    ts2.close()
    # 8 channels in one call against each channel alone
    T8 = 3000
    x8 = _signal(8, T8 * ha)
    ts.reset()
    y8 = ts.process(x8)
    for c in range(8):
        ts.reset()
        assert np.array_equal(_bits(ts.process(x8[c:c + 1])), _bits(y8[c:c + 1])), c
    ts.close()


def test_non_finite_input_recovers():
    import phaze_amd
    N, ha, hs = 1024, 256, 320
    T = 200
    x = S.make_signal("tonal", 0, T * ha)[None, :].copy()
    s_nan, s_inf = 10000, 20000
    x[0, s_nan] = np.nan
    x[0, s_inf] = np.inf
    ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=1, max_frames=T)
    y = ts.process(x)
    hist, acc, phi, psi = ts.export_state(0)
    ts.close()
    halo = (N - 1) // hs
    clean_from = ((s_inf + N - ha) // ha + halo + 1) * hs
    assert not np.all(np.isfinite(y))                                   # the bad samples did reach the output
    assert np.all(np.isfinite(y[0, clean_from:]))
    assert np.all(np.isfinite(acc)) and np.all(np.isfinite(hist))
    # ... and the integer phase state carries on: the tail matches the model run on the same input
    ref = StretchModel(N, ha, hs).process(x)
    assert _rel(y[0, clean_from:], ref[0, clean_from:]) <= 1e-5


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_c_example_runs(tmp_path):
    import phaze_amd
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_stretch")
    cmd = ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "pv_stretch.c"),
           "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "1024", "256", "320", "400"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["output_samples"] == 400 * 320 and 0.1 < j["output_rms"] < 1.0
