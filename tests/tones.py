"""Stationary tones and their closed-form time stretch (test infrastructure for tests/test_stretch_model.py and tests/test_gpu_stretch_edges.py).

A phase-locked vocoder maps a sum of partials A_i cos(2 pi f_i n / N + phi_i) (f_i in bins) to  sum_i A_i g(n) cos(2 pi f_i n / N + c_i)  after the onset:
every partial keeps its frequency and its amplitude and gets one constant phase c_i.  g(n) = (hs / N) sum_m w^2(n - m hs) is the overlap-add envelope of
the periodic Hann window w (hann_f32), frame m's synthesis window starting at output sample m hs.  `tone_fit` fits an output to that basis by least
squares and returns each partial's fitted amplitude over A_i and the relative RMS of what the fit leaves.
"""
import numpy as np

from stretch_model import hann_f32


def partials(N, freqs, amps, phases, n):
    """float32[n]: sum_i amps[i] cos(2 pi freqs[i] k / N + phases[i]), k = 0 .. n-1 (fp64, rounded once)."""
    k = np.arange(n, dtype=np.float64)
    x = np.zeros(n, np.float64)
    for f, a, p in zip(freqs, amps, phases):
        x += a * np.cos(2.0 * np.pi * f * k / N + p)
    return x.astype(np.float32)


def envelope(N, hs, n):
    """g[0 .. n): (hs / N) sum_{m >= 0} w^2(k - m hs), w the periodic f32 Hann of N points taken exactly."""
    w2 = hann_f32(N).astype(np.float64) ** 2
    g = np.zeros(n + N, np.float64)
    for m in range(0, (n + hs - 1) // hs):
        g[m * hs:m * hs + N] += w2
    return g[:n] * (hs / N)


def steady_range(N, ha, hs, n):
    """[lo, hi) of the output where the closed form holds: past the onset of (ceil(N / ha) + 2) hs + N samples and before the last N."""
    lo = (-(-N // ha) + 2) * hs + N
    return lo, n - N


def tone_fit(y, N, ha, hs, freqs, amps):
    """(fitted amplitude / A_i for every partial, relative RMS of the residual) over the steady range of y (one channel)."""
    y = np.asarray(y, np.float64)
    lo, hi = steady_range(N, ha, hs, y.size)
    assert hi - lo >= 4 * N, ("too short for the closed form", lo, hi, y.size)
    g = envelope(N, hs, y.size)[lo:hi]
    k = np.arange(lo, hi, dtype=np.float64)
    cols = []
    for f in freqs:
        w = 2.0 * np.pi * f / N
        cols += [g * np.cos(w * k), g * np.sin(w * k)]
    B = np.stack(cols, axis=1)
    yy = y[lo:hi]
    coef, *_ = np.linalg.lstsq(B, yy, rcond=None)
    res = yy - B @ coef
    ratio = np.hypot(coef[0::2], coef[1::2]) / np.asarray(amps, np.float64)
    return ratio, float(np.sqrt(np.mean(res ** 2)) / np.sqrt(np.mean(yy ** 2)))


def check_partials(N, freqs):
    """The oracle's scope: >= N/32 bins from DC and Nyquist, >= 12 bins apart, >= 0.05 bin from a half bin."""
    f = np.sort(np.asarray(freqs, np.float64))
    assert np.all(f >= N / 32) and np.all(f <= N / 2 - N / 32), f
    assert np.all(np.diff(f) >= 12), f
    assert np.all(np.abs((f % 1.0) - 0.5) >= 0.05), f


def ripple(N, hs):
    """(min, max) of g in the steady state (g has period hs there): the gain ripple when Hann^2 does not overlap-add to a constant."""
    g = envelope(N, hs, 2 * N + hs)[2 * N:]
    return float(g.min()), float(g.max())


# (N, ha, hs, partials in bins, amplitudes): every N from 256 to 8192, hs / ha from 1/8 to 8, R_s = N / hs in {2, 8/3, 3.2, 4, 8, N} and beyond
CASES = {
    "1024-256-256": (1024, 256, 256, [64.37], [0.5]),
    "1024-256-320": (1024, 256, 320, [64.37], [0.5]),
    "1024-256-384": (1024, 256, 384, [64.37], [0.5]),
    "1024-256-512": (1024, 256, 512, [64.37], [0.5]),
    "1024-512-256": (1024, 512, 256, [64.37], [0.5]),
    "1024-1024-256": (1024, 1024, 256, [64.37], [0.5]),
    "1024-7-8": (1024, 7, 8, [64.37], [0.5]),
    "256-64-80": (256, 64, 80, [40.3], [0.5]),
    "256-64-128": (256, 64, 128, [40.3], [0.5]),
    "256-8-1": (256, 8, 1, [40.3], [0.5]),
    "256-1-8": (256, 1, 8, [40.3], [0.5]),
    "512-100-97": (512, 100, 97, [77.7], [0.5]),
    "512-32-256": (512, 32, 256, [77.7], [0.5]),
    "2048-256-256": (2048, 256, 256, [300.6], [0.5]),
    "2048-2048-256": (2048, 2048, 256, [300.6], [0.5]),
    "4096-512-1024": (4096, 512, 1024, [700.2], [0.5]),
    "8192-2048-2560": (8192, 2048, 2560, [1000.37], [0.5]),
    "2p-1024-256-320": (1024, 256, 320, [64.37, 80.9], [0.5, 0.3]),
    "3p-1024-256-384": (1024, 256, 384, [40.3, 100.7, 180.2], [0.4, 0.3, 0.2]),
}


def case_input(N, ha, hs, freqs, amps, seed=0):
    """(T, float32[T ha]): enough frames for 8 N of steady output."""
    lo, _ = steady_range(N, ha, hs, 0)
    T = -(-(lo + 9 * N) // hs)
    rng = np.random.default_rng(seed)
    return T, partials(N, freqs, amps, rng.uniform(0, 2 * np.pi, len(freqs)), T * ha)


def edge_d(ha, hs, H, rng):
    """int64[H] values of d = (int32)(q - phi - ha k 2^32/N) that sit on the advance's edges, cycled over the bins: -2^31, 2^31 - 1, 0, +-1, the d in
    [0, 2 ha) where (2 d hs + ha) mod 2 ha is smallest and largest (an exact multiple of 2 ha when one exists, else the nearest on either side), their
    negatives, and random values."""
    t = np.arange(2 * ha, dtype=np.int64)
    r = (2 * t * hs + ha) % (2 * ha)
    lo, hi = int(t[np.argmin(r)]), int(t[np.argmax(r)])
    fixed = [-2 ** 31, 2 ** 31 - 1, 0, 1, -1, lo, hi, -lo, -hi, lo + 2 * ha * 1000, -hi - 2 * ha * 777]
    d = rng.integers(-2 ** 31, 2 ** 31, H, dtype=np.int64)
    for i in range(H):
        if i % 2 == 0:
            d[i] = fixed[(i // 2) % len(fixed)]
    return d


def phi_for_d(q, d, k, N, ha):
    """uint32 phi with (int32)(q - phi - ha k 2^32/N) = d."""
    e = (np.int64(ha) * np.asarray(k, np.int64) * (2 ** 32 // N)) & 0xFFFFFFFF
    return ((np.asarray(q, np.int64) - e - np.asarray(d, np.int64)) & 0xFFFFFFFF).astype(np.uint32)
