"""CPU checks of the time-stretch model (tests/stretch_model.py) that the GPU kernels are held to: at ha = hs it is the pitch shifter at pitchFactor 1
(the path pinned to the reference), a stretched sine keeps its frequency, and the fixed-point phase advance is the integer arithmetic of DESIGN.md."""
import numpy as np
import pytest

import oracle_lib
import signals as S
from stretch_model import StretchModel, phase_advance, phase_q, regions, find_peaks


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


@pytest.mark.parametrize("N", [1024, 2048])
@pytest.mark.parametrize("hop", [128, 256, 512])
@pytest.mark.parametrize("kind", ["tonal", "noise"])
def test_stretch_one_is_pitch_factor_one(N, hop, kind):
    T = 64
    x = S.make_signal(kind, 0, T * hop)[None, :]
    y = StretchModel(N, hop, hop).process(x)
    ref = oracle_lib.Oracle(N, hop, 1).process_planar(x, np.ones(T, np.float32))
    assert y.shape == ref.shape
    assert _rel(y, ref) <= 1e-8


def test_sine_keeps_its_frequency():
    N, ha, hs, k = 1024, 256, 384, 64
    T = 96
    n = np.arange(T * ha)
    x = (0.5 * np.sin(2 * np.pi * k * n / N)).astype(np.float32)[None, :]
    y = StretchModel(N, ha, hs).process(x)
    assert y.shape == (1, T * hs)
    tail = y[0, N:N + 16 * N].astype(np.float64)                     # past the latency of N - hs samples
    spec = np.abs(np.fft.rfft(tail * np.hanning(tail.size)))
    f = np.argmax(spec) / tail.size                                  # cycles per sample
    assert abs(f - k / N) < 0.5 / tail.size
    assert 0.1 < float(np.sqrt(np.mean(tail ** 2))) < 1.0


def test_fixed_point_advance_by_hand():
    N, ha, hs = 1024, 256, 384                                       # 2^32 / N = 2^22
    k = np.array([0, 3, 5], np.int64)
    phi = np.array([0, 0, 100], np.uint32)
    # bin 3: e = 256*3*2^22 mod 2^32 = 3*2^30 mod 2^32 = 3221225472; q = e - 1000 -> d = -1000
    # adv = 384*3*2^22 + floor((2*(-1000)*384 + 256) / 512) = 1152*2^22 + floor(-767744/512 = -1499.5) = 4831838208 - 1500 -> mod 2^32
    # bin 5: e = 1280*2^22 mod 2^32 = 1073741824; q = e + 100 + 7 -> d = 7: floor((5376 + 256) / 512) = 11
    # bin 0: q = 0, d = 0: adv = floor(256 / 512) = 0
    q = np.array([0, (3221225472 - 1000) % 2 ** 32, (1073741824 + 107) % 2 ** 32], np.uint32)
    adv = phase_advance(q, phi, k, N, ha, hs)
    assert adv.tolist() == [0, (4831838208 - 1500) % 2 ** 32, (1920 * 2 ** 22 + 11) % 2 ** 32]


def test_phase_q_rules():
    X = np.array([0 + 0j, -1 + 0j, 0 + 1j, np.nan + 0j, 1 + 1e-300j, complex(np.inf, np.inf), complex(1.0, -np.inf)], np.complex128)
    assert phase_q(X).tolist() == [0, 2 ** 31, 2 ** 30, 0, 0, 0, 0]


def test_regions_follow_shift_peaks_at_one():
    assert regions([], 9).tolist() == [-1] * 9
    assert regions([4], 9).tolist() == [4] * 9
    # peaks 3 and 8 (gap 5): 3 keeps 3..5 (ceil(5/2) = 3 bins), 8 starts at 8 - floor(5/2) = 6; peaks 8 and 12 (gap 4): 12 starts at 10
    assert regions([3, 8, 12], 16).tolist() == [3] * 6 + [8] * 4 + [12] * 6
    mag = np.array([0, 1, 5, 1, 0, 2, 3, 9, 2], np.float32)
    assert find_peaks(mag) == [2]                                    # i in [2, H - 2): bin 7 is outside
