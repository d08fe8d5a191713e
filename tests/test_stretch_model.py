"""CPU checks of the time-stretch model (tests/stretch_model.py) that the GPU kernels are held to: at ha = hs it is the pitch shifter at pitchFactor 1
(the path pinned to the reference), a stretched sine keeps its frequency, and the fixed-point phase advance is the integer arithmetic of DESIGN.md."""
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib
import signals as S
import tones as TN
from stretch_model import StretchModel, phase_advance, phase_q, regions, find_peaks
from tones import edge_d, phi_for_d


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


# ---- a closed-form oracle: stationary tones (tests/tones.py) -------------------------------------------------------------------------------------------
# What the model gives (max |amplitude ratio - 1| / residual): single tones <= 2e-8 / <= 7e-7, two partials 3e-7 / 2.4e-5, three partials 5e-9 / 3.5e-6.
# The gates are about 4x that; the multi-partial residual is the algorithm's (the other partial's window sidelobes locked to the wrong peak), not rounding.
CPU_TOL = {"2p-1024-256-320": 1e-4, "3p-1024-256-384": 1.5e-5}


@pytest.mark.parametrize("cid", list(TN.CASES))
def test_tones_closed_form(cid):
    N, ha, hs, freqs, amps = TN.CASES[cid]
    TN.check_partials(N, freqs)
    T, x = TN.case_input(N, ha, hs, freqs, amps)
    y = StretchModel(N, ha, hs).process(x[None, :])[0]
    ratio, res = TN.tone_fit(y, N, ha, hs, freqs, amps)
    tol = CPU_TOL.get(cid, 3e-6)
    assert np.all(np.abs(ratio - 1.0) <= tol), (ratio, tol)
    assert res <= tol, (res, tol)


def test_envelope_ripple():
    """g(n) is what a correct vocoder's gain is: 0.25 .. 0.5 at R_s = 2, +-0.8 % at R_s = 3.2, +-4.3 % at R_s = 8/3, flat at R_s = 4 and 8."""
    lo, hi = TN.ripple(1024, 512)
    assert abs(lo - 0.25) < 1e-9 and abs(hi - 0.5) < 1e-9
    for hs, rip in ((320, 0.008), (384, 0.043)):
        lo, hi = TN.ripple(1024, hs)
        assert abs((hi - lo) / (hi + lo) - rip) < 0.001, (hs, lo, hi)
    for hs in (256, 128):
        lo, hi = TN.ripple(1024, hs)
        assert hi - lo < 1e-6 and abs(hi - 0.375) < 1e-6


def test_half_bin_tie_is_silent():
    """A tone on an exact half bin has two equal bins in exact arithmetic.  Where they tie, there is no strict maximum: findPeaks finds no peak and the frame
    is silent (the reference's rule).  Whether they tie rests on the rounding of the input, so the tone tests keep 0.05 bin away from a half bin."""
    mag = np.array([0, 1, 3, 9, 9, 3, 1, 0, 0], np.float32)
    assert find_peaks(mag) == []
    assert regions(find_peaks(mag), mag.size).tolist() == [-1] * mag.size
    m = StretchModel(256, 64, 80)
    assert np.all(m.process(np.zeros((1, 8 * 64), np.float32)) == 0.0) and m.last["peaks"][0] == -1


def _adv_exact(q, phi, k, N, ha, hs):
    """The advance from its definition with Python integers: hs k 2^32/N + round-half-up(d hs / ha), d the principal value of q - phi - ha k 2^32/N."""
    out = []
    for qq, pp, kk in zip(q.tolist(), phi.tolist(), k.tolist()):
        d = (qq - pp - ha * kk * (2 ** 32 // N)) % 2 ** 32
        d = d - 2 ** 32 if d >= 2 ** 31 else d
        r = (2 * d * hs + ha) // (2 * ha)                        # floor(d hs / ha + 1/2)
        assert Fraction(r) <= Fraction(d * hs, ha) + Fraction(1, 2) < r + 1
        out.append((hs * kk * (2 ** 32 // N) + r) % 2 ** 32)
    return out


@pytest.mark.parametrize("N,ha,hs", [(1024, 256, 384), (8192, 1, 4096), (256, 256, 1), (512, 100, 97), (256, 255, 64), (1024, 7, 8)])
def test_fixed_point_advance_edges(N, ha, hs):
    """phase_advance at the edges of d: -2^31, 2^31 - 1, 0, +-1, the d where 2 d hs + ha sits on (or just below) a multiple of 2 ha, random d."""
    rng = np.random.default_rng(N + ha + hs)
    H = N // 2 + 1
    k = np.arange(H, dtype=np.int64)
    q = rng.integers(0, 2 ** 32, H, dtype=np.uint64).astype(np.uint32)
    d = edge_d(ha, hs, H, rng)
    phi = phi_for_d(q, d, k, N, ha)
    got = phase_advance(q, phi, k, N, ha, hs).tolist()
    assert got == _adv_exact(q, phi, k, N, ha, hs)
    # and at those bins the rounding really is on an edge (ha > 1): floor(... + 1/2) with and without the half differ somewhere
    assert ha == 1 or any(((2 * int(dd) * hs + ha) // (2 * ha)) != ((2 * int(dd) * hs) // (2 * ha)) for dd in d)
