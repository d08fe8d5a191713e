"""How far the reference's rotation cos/sin(fl(2 pi delta / N) * t) drifts from the exact root of unity the kernels apply, tw[(delta * t) mod N], as the
time cursor t grows.  CPU only, numpy only.

The reference (phase-vocoder.js:155-157, oracle/pv_oracle.c shift_peaks) forms omega = 2 * pi * delta / N in doubles (N is a power of two: one rounding of
pi itself, one of the product with delta) and then the angle omega * t (one more rounding).  The three relative errors add up to at most
(0.36 + 1 + 1) 2^-53 < 2.4 * 2^-53 of an angle of at most pi * t (|delta| <= N / 2):

    |angle error| <= 2.4 * 2^-53 * pi * t        (+ 1e-15 for libm's cos / sin and the atan2 below)

The kernels reduce delta * t mod N in integers and look the rotation up: they have no such term.  So past some t it is the REFERENCE that is wrong, and a
comparison of kernel against reference measures the reference.  This file measures where: the angle between the two unit vectors, from their cross and
dot products (never by subtracting large angles), for every delta in [-N/2, N/2] and every residue of t = m * hop mod N.

Measured maxima (N = 1024 / N = 8192; the bound in brackets):
    t ~ 2^20   5.5e-10 / 5.8e-10 rad   (8.8e-10)
    t ~ 2^24   9.3e-9  / 9.0e-9        (1.4e-8)
    t ~ 2^26   3.6e-8  / 3.7e-8        (5.6e-8)
    t ~ 2^28   1.4e-7  / 1.5e-7        (2.2e-7)
    t ~ 2^31   1.1e-6  / 1.2e-6        (1.8e-6)
    t ~ 2^32   2.3e-6  / 2.3e-6        (3.6e-6)
The reference stays within 1e-7 rad of the exact rotation up to t = 1.67e8 samples (2^27.3: 58 minutes at 48 kHz), see
test_where_the_reference_leaves_1e_7.
"""
import numpy as np
import pytest

BOUND = 2.4 * 2.0 ** -53 * np.pi             # rad per sample of t
SLACK = 1e-15


def worst_angle(N, hop, t0):
    """max over delta in [-N/2, N/2] and the R cursors t0, t0 + hop, .. of the angle between the reference's rotation and the exact one."""
    delta = np.arange(-N // 2, N // 2 + 1, dtype=np.int64)[:, None]
    t = (int(t0) + hop * np.arange(N // hop, dtype=np.int64))[None, :]
    omega = 2 * np.pi * delta.astype(np.float64) / N                       # the reference's order of operations (pv:155)
    a = omega * t.astype(np.float64)                                       # t < 2^53: exact as a double
    k = (delta * t) % N                                                    # |delta * t| < 2^13 * 2^33: exact in int64; numpy's % is non-negative
    e = 2 * np.pi * k.astype(np.float64) / N                               # an angle in [0, 2 pi): cos / sin of it are good to an ulp
    rc, rs, ec, es = np.cos(a), np.sin(a), np.cos(e), np.sin(e)
    return float(np.max(np.abs(np.arctan2(rs * ec - rc * es, rc * ec + rs * es))))


@pytest.mark.parametrize("N", [1024, 8192])
@pytest.mark.parametrize("log2t", [20, 24, 26, 28, 31, 32])
def test_the_reference_rotation_stays_within_its_rounding_bound(N, log2t):
    hop = N // 4
    t0 = 2 ** log2t + 3 * hop
    w = worst_angle(N, hop, t0)
    bound = BOUND * (t0 + N) + SLACK
    print(f"N {N} t ~ 2^{log2t}: max angle error {w:.3e} rad (bound {bound:.3e})")
    assert w <= bound
    assert w >= 0.25 * bound, "the bound is not tight within a factor of four: the model of the reference's roundings is wrong"
    if log2t == 26:
        assert w < 1e-7                      # what tests/test_gpu_long_streams.py relies on for its oracle comparison at 2^26


def test_where_the_reference_leaves_1e_7():
    """The largest t on a grid of 2^(1/16) steps up to which the reference is within 1e-7 rad: DESIGN.md quotes it."""
    N, hop = 1024, 256
    last = None
    for s in range(26 * 16, 28 * 16 + 1):
        t0 = int(round(2.0 ** (s / 16.0) / hop)) * hop
        if worst_angle(N, hop, t0) >= 1e-7:
            break
        last = t0
    print(f"the reference stays within 1e-7 rad up to t = {last} (2^{np.log2(last):.2f}, {last / 48000 / 60:.0f} min at 48 kHz); "
          f"at 2^31: {worst_angle(N, hop, 2 ** 31):.3e} rad")
    assert 2 ** 26 < last < 2 ** 28          # between the two powers the bound puts it
