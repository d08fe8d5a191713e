"""The resampler's numpy model (tests/resample_model.py) against closed forms: what the filter itself leaves, before any kernel is involved.

Every gate is twice the figure measured on this model (DESIGN.md "Resampling and pitch" lists them); the figures are printed before each assertion.
"""
import numpy as np
import pytest

import resample_model as RM
import tones
from stretch_model import StretchModel

RATIOS = [(4, 5), (5, 4), (1, 8), (8, 1), (97, 100), (3, 2)]
# max |y - cos| over the steady output for a unit tone at `frac` of the narrower Nyquist, measured on this model: (up, down) -> {frac: figure}
PASSBAND = {
    (4, 5): {0.01: 3.63e-6, 0.1: 1.25e-5, 0.5: 1.48e-6, 0.8: 3.23e-5},
    (5, 4): {0.01: 4.45e-6, 0.1: 1.32e-5, 0.5: 1.43e-6, 0.8: 3.63e-5},
    (1, 8): {0.01: 2.97e-6, 0.1: 1.12e-5, 0.5: 1.30e-6, 0.8: 3.05e-5},
    (8, 1): {0.01: 4.41e-6, 0.1: 1.37e-5, 0.5: 1.52e-6, 0.8: 3.63e-5},
    (97, 100): {0.01: 4.39e-6, 0.1: 1.37e-5, 0.5: 1.56e-6, 0.8: 3.64e-5},
    (3, 2): {0.01: 4.18e-6, 0.1: 1.32e-5, 0.5: 1.43e-6, 0.8: 3.63e-5},
}
# RMS of the output over the RMS of the input for a tone at 1.09 x the output Nyquist (it would alias), measured: (up, down) -> figure.  Ratios with
# M / L >= 1.09 only: below that the tone lies above the INPUT Nyquist and is no tone of that frequency at all
STOPBAND = {(4, 5): 1.75e-5, (1, 8): 1.74e-5, (2, 3): 1.71e-5}


def tone_error(up, down, frac, taps=None, process=None):
    """max |y[j] - cos(2 pi f j M / L + p)| over every output the filter has fully entered, f = frac x the narrower Nyquist (cycles per input sample)."""
    m = RM.ResampleModel(up, down, 1, taps)
    f = 0.5 * frac * min(1.0, m.L / m.M)
    nin = 6 * m.T + 4000 * max(1, m.M // m.L)
    n = np.arange(nin, dtype=np.float64)
    x = np.cos(2.0 * np.pi * f * n + 0.3).astype(np.float32)
    y = np.asarray((process or m.process)(x[None, :]), np.float64)[0]
    j = np.arange(y.size, dtype=np.float64)
    want = np.cos(2.0 * np.pi * f * j * m.M / m.L + 0.3)
    lo = -(-m.T * m.L // m.M)                                   # outputs whose window reaches before the stream
    return float(np.max(np.abs(y[lo:] - want[lo:])))


def alias_ratio(up, down, taps=None, process=None):
    m = RM.ResampleModel(up, down, 1, taps)
    assert m.M > m.L
    f = 0.5 * 1.09 * m.L / m.M
    nin = 6 * m.T + 4000 * (m.M // m.L)
    x = np.cos(2.0 * np.pi * f * np.arange(nin, dtype=np.float64) + 0.3).astype(np.float32)
    y = np.asarray((process or m.process)(x[None, :]), np.float64)[0]
    lo = -(-m.T * m.L // m.M)
    return float(np.sqrt(np.mean(y[lo:] ** 2)) / np.sqrt(np.mean(x.astype(np.float64) ** 2)))


@pytest.mark.parametrize("up,down", RATIOS)
def test_passband_tones_follow_the_cosine(up, down):
    for frac, measured in PASSBAND[(up, down)].items():
        err = tone_error(up, down, frac)
        print(f"passband {up}/{down} at {frac}: {err:.3e} (gate {2 * measured:.1e})")
        assert err <= 2 * measured, (up, down, frac, err)


@pytest.mark.parametrize("up,down", sorted(STOPBAND))
def test_a_tone_above_the_output_nyquist_is_removed(up, down):
    r = alias_ratio(up, down)
    print(f"stopband {up}/{down}: {r:.3e} (gate {2 * STOPBAND[(up, down)]:.1e})")
    assert r <= 2 * STOPBAND[(up, down)], (up, down, r)


@pytest.mark.parametrize("up,down", RATIOS + [(147, 160), (8191, 8192), (8192, 8191), (1, 1), (6, 8)])
def test_every_phase_has_unit_dc_gain_and_the_documented_shape(up, down):
    h, L, M, W = RM.design(up, down)
    assert h.dtype == np.float32 and h.shape == (L, 2 * W) and W == int(np.ceil(32 * max(1.0, M / L)))
    assert L * 2 * W <= 8192 * 512
    assert np.max(np.abs(h.astype(np.float64).sum(axis=1) - 1.0)) <= 2.0 ** -22
    raw, *_ = RM.design(up, down, normalise=False)
    print(f"{up}/{down}: un-normalised row sums within {np.max(np.abs(raw.sum(axis=1) - 1.0)):.2e} of 1")
    if (up, down) == (4, 5):
        assert np.max(np.abs(raw.sum(axis=1) - 1.0)) > 2.0 ** -22                                # the division is not a no-op


@pytest.mark.parametrize("up,down", [(4, 5), (5, 4), (100, 97), (1, 8), (8, 1), (8191, 8192)])
def test_count_equals_the_brute_force_definition(up, down):
    L, M = RM.reduce_ratio(up, down)
    W = RM.half_width(L, M)
    for total in list(range(0, 3 * W + 40)) + [10 * W + 7, 100003]:
        j, brute = 0, 0
        while (j * M) // L + W <= total - 1:                          # the newest sample output j reads is n_j + W
            brute += 1
            j += 1
        assert RM.count(up, down, total) == brute, (up, down, total)


def test_ratios_outside_the_range_are_refused():
    for up, down in [(0, 1), (1, 0), (-4, 5), (9, 1), (1, 9), (8193, 8192), (8191, 8193), (65537, 8192)]:
        with pytest.raises(ValueError):
            RM.reduce_ratio(up, down)
    assert RM.reduce_ratio(16384, 32768) == (1, 2) and RM.reduce_ratio(8, 1) == (8, 1) and RM.reduce_ratio(1, 8) == (1, 8)


@pytest.mark.parametrize("up,down", [(4, 5), (5, 4), (1, 8), (8, 1), (100, 97)])
def test_any_split_of_a_stream_gives_the_same_model_output(up, down):
    rng = np.random.default_rng(up * 131 + down)
    nin = 700 if down <= 2 * up else 2600
    x = rng.standard_normal((2, nin)).astype(np.float32)
    whole = RM.ResampleModel(up, down, 2)
    want = whole.process(x)
    assert want.shape[1] == RM.count(up, down, nin) > 0
    for cuts in ("ones", "random", "short"):
        m = RM.ResampleModel(up, down, 2)
        at, parts = 0, []
        while at < nin:
            n = 1 if cuts == "ones" else int(rng.integers(1, m.W)) if cuts == "short" else int(rng.integers(1, 400))
            assert m.out_count(min(n, nin - at)) == RM.count(up, down, min(nin, at + n)) - RM.count(up, down, at)
            parts.append(m.process(x[:, at:at + n]))
            at += n
        got = np.concatenate(parts, axis=1)
        assert got.shape == want.shape and np.array_equal(got, want), cuts
        assert np.array_equal(m.hist, whole.hist) and (m.I, m.J) == (whole.I, whole.J)


@pytest.mark.parametrize("up,down", [(4, 5), (100, 97), (16, 125), (8191, 8192)])
def test_a_model_set_to_a_position_continues_like_one_that_got_there(up, down):
    """tests/test_gpu_resample.py starts the model at 2^40 + 12345 by assigning hist, I and J.  That is sound if (a) a model set to a small position it could
    have reached continues exactly like the one that did reach it, and (b) the index arithmetic holds far out: shifted by k M inputs / k L outputs the phases
    repeat, so the outputs must be the same doubles -- at k M just above 2^40 and as far out as the model's own int64 product j M allows (j M ~ 2^62)."""
    rng = np.random.default_rng(up + 3 * down)
    one = RM.ResampleModel(up, down, 2)
    I0 = 3 * one.T + 12345 % one.T
    nin = I0 + 6 * one.T + 50 * max(1, down // up)
    x = rng.standard_normal((2, nin)).astype(np.float32)
    one.process(x[:, :I0])
    hist = one.hist.copy()
    want = one.process(x[:, I0:])
    assert want.shape[1] > 0
    for k in (0, 2 ** 40 // one.M + 1, 2 ** 62 // (one.L * one.M)):
        m = RM.ResampleModel(up, down, 2)
        m.hist[:], m.I, m.J = hist, I0 + k * m.M, RM.count(up, down, I0) + k * m.L
        assert m.J == RM.count(up, down, m.I)
        got = m.process(x[:, I0:])
        assert got.shape == want.shape and np.array_equal(got, want), k
        assert np.array_equal(m.hist, one.hist) and (m.I, m.J) == (one.I + k * m.M, one.J + k * m.L)


# ---- the composition: StretchModel followed by the resampler at ha / hs, against the closed form --------------------------------------------

def envelope_at(N, hs, t):
    """tones.envelope as a continuous function of the output position t: (hs / N) sum_m w^2(t - m hs), w(u) = (1 - cos(2 pi u / N)) / 2 on [0, N]."""
    t = np.asarray(t, np.float64)
    g = np.zeros_like(t)
    m0 = np.floor(t / hs).astype(np.int64)
    for d in range(0, N // hs + 2):
        u = t - (m0 - d) * hs
        ok = (u >= 0) & (u <= N) & (m0 - d >= 0)
        g += np.where(ok, (0.5 * (1.0 - np.cos(2.0 * np.pi * u / N))) ** 2, 0.0)
    return g * (hs / N)


def pitch_basis(ysize, n_mid, N, ha, hs, L, M, freqs):
    """The tones.py basis on the resampled grid: output j of the resampler sits at position t = j M / L of the stretch's output (the taps are symmetric
    about it; the lag W is only when it becomes available), so the columns are g(t) cos(w t), g(t) sin(w t) per partial.  Rows: the outputs inside the
    stretch's steady range of its n_mid samples.  Returns (their indices j, the basis)."""
    lo, hi = tones.steady_range(N, ha, hs, n_mid)
    j = np.arange(-(-lo * L // M), min(ysize, (hi * L) // M), dtype=np.int64)
    assert j.size * M // L >= 4 * N, ("too short for the closed form", j.size)
    t = j.astype(np.float64) * M / L
    g = envelope_at(N, hs, t)
    cols = []
    for f in freqs:
        w = 2.0 * np.pi * f / N
        cols += [g * np.cos(w * t), g * np.sin(w * t)]
    return j, np.stack(cols, axis=1)


def pitch_fit(y, n_mid, N, ha, hs, L, M, freqs, amps):
    """(fitted amplitude / A_i per partial, relative RMS of the residual) of one channel over pitch_basis."""
    y = np.asarray(y, np.float64)
    j, B = pitch_basis(y.size, n_mid, N, ha, hs, L, M, freqs)
    yy = y[j]
    coef, *_ = np.linalg.lstsq(B, yy, rcond=None)
    res = yy - B @ coef
    return np.hypot(coef[0::2], coef[1::2]) / np.asarray(amps, np.float64), float(np.sqrt(np.mean(res ** 2)) / np.sqrt(np.mean(yy ** 2)))


def pitch_phase_fit(y, n_mid, N, ha, hs, L, M, freqs):
    """Per channel and partial, the fitted phase (rad) over pitch_basis: float64[nch, len(freqs)] (link_model.phase_fit on the resampled grid)."""
    y = np.asarray(y, np.float64)
    j, B = pitch_basis(y.shape[1], n_mid, N, ha, hs, L, M, freqs)
    out = np.zeros((y.shape[0], len(freqs)))
    for c in range(y.shape[0]):
        coef, *_ = np.linalg.lstsq(B, y[c, j], rcond=None)
        out[c] = np.arctan2(-coef[1::2], coef[0::2])
    return out


PITCH_CASES = ["1024-256-320", "1024-256-384", "1024-512-256", "512-100-97", "256-64-80", "1024-256-512", "4096-512-1024", "2p-1024-256-320"]
# measured on the models: case -> (largest |fitted amplitude / A - 1|, relative residual)
PITCH_MEASURED = {
    "1024-256-320": (1.25e-5, 2.38e-6), "1024-256-384": (9.6e-8, 3.31e-7), "1024-512-256": (5.4e-8, 3.29e-7), "512-100-97": (8.5e-7, 3.01e-6),
    "256-64-80": (1.06e-5, 3.05e-6), "1024-256-512": (1.18e-7, 5.82e-7), "4096-512-1024": (5.4e-7, 1.40e-7), "2p-1024-256-320": (1.28e-5, 2.37e-5),
}


def pitch_case_model(name):
    N, ha, hs, freqs, amps = tones.CASES[name]
    tones.check_partials(N, freqs)
    T, x = tones.case_input(N, ha, hs, freqs, amps)
    mid = StretchModel(N, ha, hs).process(x[None, :])
    rs = RM.ResampleModel(ha, hs)
    y = rs.process(mid)[0]
    return N, ha, hs, freqs, amps, x, y, rs


@pytest.mark.parametrize("name", PITCH_CASES)
def test_stretch_then_resample_fits_the_closed_form(name):
    N, ha, hs, freqs, amps, x, y, rs = pitch_case_model(name)
    assert y.size == RM.count(ha, hs, (x.size // ha) * hs)
    ratio, res = pitch_fit(y, (x.size // ha) * hs, N, ha, hs, rs.L, rs.M, freqs, amps)
    amp_gate, res_gate = (2 * v for v in PITCH_MEASURED[name])
    print(f"pitch {name}: amplitude ratio {ratio}, residual {res:.3e} (gates {amp_gate:.1e}, {res_gate:.1e})")
    assert np.max(np.abs(ratio - 1.0)) <= amp_gate and res <= res_gate, (name, ratio, res)
