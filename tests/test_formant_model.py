"""CPU checks of warped grains on the overlap-add path as tests/formant_model.py defines them (DESIGN.md "Formant shifting"): a table without warped grains
is tests/tsm_model.py's in every respect; the planner with warps=None is tsm_plan bit for bit, and with a row differs from it in L and in bits 17 .. 26 of w
only; every tile of a warped plan fits the span at its corners; the envelope moves with the step while the pitch follows the grain spacing; and a warped
grain above step 1 does not alias.  The C planner and tile walk are compared with the model in tests/test_formant_abi.py, the kernel in
tests/test_gpu_formant.py."""
import numpy as np
import pytest

import f0_model as FM
import formant_model as FoM
import psola_model as PM
import test_epoch_model as TEM
import test_gpu_tsm as TGT
import test_mirror_model as TMM
import test_psola_model as TPM
import tsm_model as TM

SR = FM.SAMPLE_RATE
STEP = FoM.STEP


# ---- tables without warped grains ------------------------------------------------------------------------------------------------------------------

def test_a_table_without_warped_grains_is_tsm_models():
    """process (values, bound and poisoned outputs) and tiles, with ==, on the tables of tests/test_gpu_tsm.py, written with z = 0 and with z = 256; the
    verdicts of check_grains with the new reason."""
    for name in ("small", "mid", "tiny", "huge", "sweep", "gap", "empty", "slow"):
        mp, R, nin, g = TGT._grains(name)
        x = TGT._signals(nin, 3)[:2]
        x[1, nin // 2] = np.nan
        same = np.array(g, np.int64)
        same[:, 1] += 256 * STEP                                            # z = 256: treated exactly as z = 0
        assert FoM.check_grains(g, mp) is None and FoM.check_grains(same, mp) is None and not FoM.warped(same).any()
        for first, count in ((0, TGT.NOUT), (1001, 1500)):
            want = TM.process(x, g, first, count, bound=True)
            for table in (g, same):
                got = FoM.process(x, table, first, count, bound=True)
                for a, b in zip(got, want):
                    assert np.array_equal(a, b, equal_nan=True), name
                assert np.array_equal(FoM.process(x, table, first, count), want[0])
                assert np.array_equal(FoM.tiles(table, mp, first, count), TM.tiles(g, mp, first, count))
    for bad, why in (([[5, 1 << 27, 0, 9]], "step"), ([[5, -1, 0, 9]], "step"), ([[5, 127 * STEP, 0, 9]], "step"), ([[5, STEP, 0, 9]], "step"),
                     ([[5, 513 * STEP + 7, 0, 9]], "step"), ([[5, 65536, 0, 9]], "step"), ([[5, 65536 + 300 * STEP, 0, 9]], "step"), ([[-1, 0, 0, 9]], "centre"),
                     ([[1 << 30, 300 * STEP, 0, 9]], "centre"), ([[5, 300 * STEP, 1 << 30, 9]], "shift"), ([[5, 300 * STEP, -(1 << 30), 9]], "shift"),
                     ([[5, 128 * STEP + 7, 0, 65]], "half length"), ([[5, 512 * STEP + 7, 0, 9], [5, 200 * STEP + 6, 0, 9]], "out of order")):
        assert FoM.check_grains(np.array(bad), 64)[1] == why, bad
    assert FoM.check_grains(np.array([[5, 128 * STEP + 65535, (1 << 30) - 1, 64], [5, 512 * STEP + 65535, 1 - (1 << 30), 2], [5, 256 * STEP + 65535, 0, 2]]), 64) is None


def test_a_warped_grain_reads_the_position_the_contract_states():
    """On a ramp x[p] = p an interpolated sample is its position: (t + tf / 256 - D - phi / 256) + (s / 256) (n - t - tf / 256), at every step and fraction."""
    ramp = np.arange(6000, dtype=np.float32)
    for s in (128, 129, 200, 255, 257, 300, 511, 512):
        for tf, phi in ((0, 0), (200, 77), (255, 255), (0, 1)):
            t, D, L = 500, -2000, 100
            y = FoM.process(ramp, np.array([[t, tf + 256 * phi + STEP * s, D, L]]), 0, 700)[0]
            k = np.arange(t - L + 1, t + L)
            want = (t + tf / 256.0 - D - phi / 256.0) + (s / 256.0) * (k - t - tf / 256.0)
            assert np.all(np.abs(y[k] - want) < 4e-3), (s, tf, phi, float(np.max(np.abs(y[k] - want))))       # the interpolator's error on a ramp
            assert np.all(y[:t - L] == 0.0) and np.all(y[t + L + 1:] == 0.0)


# ---- the planner ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(24))
def test_the_plan_without_warps_is_tsm_plan_and_with_them_differs_in_length_and_step_only(seed):
    args, kw, mp, R = TMM.track(seed)
    nrec = np.asarray(args[0]).reshape(-1, 4).shape[0]
    base, base_len = TM.tsm_plan(*args, **kw)
    got, n = FoM.formant_plan(*args, warps=None, **kw)
    assert got.dtype == np.int32 and np.array_equal(got, base) and n == base_len
    got, n = FoM.formant_plan(*args, warps=np.ones(nrec), **kw)
    assert np.array_equal(got, base) and n == base_len                      # the step 256 is written as z = 0
    warps = np.random.default_rng(700 + seed).uniform(0.5, 2.0, nrec)
    warps[::7] = 1.0
    got, n = FoM.formant_plan(*args, warps=warps, **kw)
    assert n == base_len and got.shape == base.shape and FoM.check_grains(got, mp) is None
    assert np.array_equal(got[:, [0, 2]], base[:, [0, 2]]) and np.array_equal(got[:, 1] & 0xFFFF, base[:, 1])
    z = got[:, 1] >> 17
    assert np.all((z == 0) | ((z >= 128) & (z <= 512) & (z != 256))) and (z != 0).sum() > got.shape[0] // 2
    s = FoM.steps(got)
    assert np.all(got[s > 256, 3] <= base[s > 256, 3]) and np.all(got[s < 256, 3] >= base[s < 256, 3]) and np.any(got[:, 3] != base[:, 3])
    assert np.array_equal(got[s == 256, 3], base[s == 256, 3])
    assert FoM.check_span(got, mp, R, 0, n) is None and FoM.check_span(got, mp, R, 777, max(n - 777, 0)) is None
    for bad in (np.full(nrec, 0.49), np.full(nrec, 2.01), np.full(nrec, np.nan), np.ones(nrec + 1)):
        with pytest.raises(ValueError):
            FoM.formant_plan(*args, warps=bad, **kw)


PAIRS = [(mp, R) for R in (1, 2, 3, 4) for mp in (64, 256, 1024, 2048, max(m for m in range(1024, 4097) if FoM.fits(m, R))) if FoM.fits(mp, R)]


def test_the_pairs_that_fit_are_fewer_than_tsm():
    assert {R: max(m for m in range(2, 4097) if FoM.fits(m, R)) for R in (1, 2, 3, 4)} == {1: 3753, 2: 2900, 3: 2331, 4: 1925}
    assert all(TM.lds_bytes(mp, R) <= TM.LDS_BYTES for mp, R in PAIRS) and not FoM.fits(4096, 1) and not FoM.fits(2048, 4) and FoM.fits(2048, 3)
    assert (1024, 4) in PAIRS and (3753, 1) in PAIRS and (1925, 4) in PAIRS and len(PAIRS) == 19


@pytest.mark.parametrize("mp,R", PAIRS)
def test_the_span_at_the_highest_rate_the_longest_period_and_the_extreme_steps(mp, R):
    """tests/test_tsm_model.py's corner (the rate R throughout, periods at max_period and at its half, ratios 1/2, 1 and 2, voiced and unvoiced, marks snapped
    onto arbitrary epoch records) at the steps 1/2 and 2, for pairs up to the largest the handle accepts at each rate."""
    rng = np.random.default_rng(mp + R)
    worst = 0
    for period in (float(mp), mp / 2.0, -float(mp)):
        for ratio in (0.5, 1.0, 2.0):
            nrec = (4 * 1024 * R + 8 * mp) // 64
            recs = PM.records_of([period] * nrec)
            ep = TEM.random_epochs(rng, nrec, 2 * min(mp, 2048))
            for warp in (0.5, 2.0):
                for epochs in (None, ep):
                    g, nout = FoM.formant_plan(recs, 64, 32, nrec * 64, float(mp), min(20, mp), mp, ratios=np.full(nrec, ratio), rates=np.full(nrec, float(R)),
                                               warps=np.full(nrec, warp), epochs=epochs, lock=1.0)
                    for first in (0, 511):
                        worst = max(worst, int(FoM.tiles(g, mp, first, nout - first)[:, 3].max()))
    print(f"max_period {mp} rate {R}: worst tile extent {worst} = {worst / FoM.span(mp, R):.3f} of span {FoM.span(mp, R)}")
    assert worst <= FoM.span(mp, R)


# ---- the envelope ---------------------------------------------------------------------------------------------------------------------------------

# (ratio, warp) -> the largest deviation in dB of a harmonic between 300 and 5000 Hz from the warped envelope |H(f / warp)|, the worst of eight mark offsets
# across one period, measured with this file on the model; the gates are twice these, the convention of tests/test_psola_model.py and tests/test_vari_model.py.
# The case (ratio 1, warp 0.75) of the issue's list is NOT here: at the mark offset -27.2 samples (the fourth of the eight; the issue's prototype tried
# three) the harmonic at 1988 Hz under the second formant (2600 * 0.75 = 1950 Hz) comes out at 0.184 and the one at 884 Hz under the first
# (1200 * 0.75 = 900 Hz) at 0.167, so the strongest harmonic lies 4.9 f0 from 900 Hz; at the other seven offsets it is 884 Hz.  The gate stays at one f0.
# Where warp == ratio every grain is a plain resampling of one period and the harmonics sit on the moved envelope to the interpolator's error.
MEASURED = {(1.0, 1.25): 25.31, (1.0, 1.5): 11.58, (1.25, 0.75): 18.92, (1.25, 1.25): 0.0002, (1.25, 1.5): 16.81, (0.8, 0.8): 0.147, (0.8, 1.25): 32.64}


@pytest.fixture(scope="module")
def voice():
    p = FM.period(PM.records_of([TPM.PERIOD])[0])
    x = PM.voice(p, TPM.N_ENV)
    x.setflags(write=False)
    f, a, res = PM.harmonic_amplitudes(x, p, *TPM.FIT)
    env = PM._resonator_response(f * SR, SR)
    return p, x, float(np.median(a / env))


@pytest.mark.parametrize("ratio,warp", sorted(MEASURED))
def test_the_envelope_moves_with_the_step_and_the_pitch_with_the_spacing(voice, ratio, warp):
    """The voice of tests/test_psola_model.py (period 217.3, resonators at 1200 and 2600 Hz).  At every one of eight mark offsets across one period the
    output is periodic at p / ratio (residual of the harmonic fit under 1 %), its strongest harmonic lies within one f0 of 1200 * warp and is not the
    harmonic nearest 1200 Hz; the deviation from the warped envelope is gated at twice MEASURED."""
    p, x, scale = voice
    nrec = TPM.N_ENV // TPM.HOP
    recs = PM.records_of([TPM.PERIOD] * nrec)
    worst, far = 0.0, 0.0
    for j in range(8):
        offset = (j / 8.0 - 0.5) * p
        g, n = FoM.formant_plan(recs, TPM.HOP, TPM.HOP // 2, TPM.N_ENV, 256.0, 32, 1024, ratios=np.full(nrec, ratio), warps=np.full(nrec, warp), offset=offset)
        assert n == TPM.N_ENV and (np.all(FoM.steps(g) == round(256 * warp)))
        y = FoM.process(x, g, 0, TPM.N_ENV)[0]
        f, a, res = PM.harmonic_amplitudes(y, p / ratio, *TPM.FIT)
        hz = f * SR
        sel = (hz >= 300.0) & (hz <= 5000.0)
        dev = float(np.max(np.abs(20.0 * np.log10(a[sel] / (scale * PM._resonator_response(hz[sel] / warp, SR))))))
        peak = float(hz[np.argmax(a)])
        f0 = SR * ratio / p
        print(f"ratio {ratio} warp {warp} offset {offset:+7.1f}: strongest {peak:6.0f} Hz ({abs(peak - 1200.0 * warp) / f0:.2f} f0 from {1200.0 * warp:.0f}), "
              f"deviation {dev:6.3f} dB, residual {res:.1e}")
        assert res < 0.01, (j, res)
        assert abs(peak - 1200.0 * warp) < f0, (j, peak)
        assert peak != float(hz[np.argmin(np.abs(hz - 1200.0))]), (j, peak)
        worst, far = max(worst, dev), max(far, abs(peak - 1200.0 * warp) / f0)
    print(f"ratio {ratio} warp {warp}: worst deviation {worst:.4f} dB (measured {MEASURED[(ratio, warp)]}), strongest harmonic at most {far:.3f} f0 from 1200 * warp")
    assert worst <= 2.0 * MEASURED[(ratio, warp)], worst


# ---- no alias ---------------------------------------------------------------------------------------------------------------------------------------

# A compressed grain (s > 256) is the input low-passed at 256 / s of its band and then decimated; the low-pass is the prototype of tests/vari_model.py
# widened by s / 256: a Kaiser window of beta 9 (side lobes near -90 dB) on 64 widened samples, cutoff 0.91, so its stop band begins at 1/2 * 256 / s cycles
# per sample.  The level asked of the stop band is the largest error tests/test_vari_model.py allows this table anywhere in its pass band, twice 4.21e-5
# (PASSBAND, "320x400" at 0.8): a stop band at the table's own error level.
STOPBAND = 2 * 4.21e-5


@pytest.mark.parametrize("warp", [1.5, 2.0])
def test_a_tone_above_the_lowered_cutoff_does_not_come_out(warp):
    """Unit tones at 1, 1.1 and 1.3 times 0.5 / warp cycles per sample through a plan at that warp (period 200, ratio 1): played compressed they would land at
    or above the output's Nyquist frequency and fold back; every output sample away from the ends stays at or below STOPBAND, so neither the tone nor an alias
    of it comes out.  A tone at a tenth of that frequency passes, moved up by the warp."""
    n, hop = 8192, 256
    nrec = n // hop
    recs = PM.records_of([200.0] * nrec)
    g, nout = FoM.formant_plan(recs, hop, hop // 2, n, 256.0, 32, 1024, warps=np.full(nrec, warp))
    assert FoM.warped(g).all() and nout == n
    t = np.arange(n, dtype=np.float64)
    for k in (1.0, 1.1, 1.3):
        f = k * 0.5 / warp
        y = FoM.process(np.cos(2.0 * np.pi * f * t + 0.3).astype(np.float32), g, 0, n)[0]
        level = float(np.max(np.abs(y[1024:n - 1024])))
        print(f"warp {warp}: tone at {f:.4f} cycles per sample comes out at {level:.3e} (gate {STOPBAND:.2e})")
        assert level <= STOPBAND, (warp, f, level)
    y = FoM.process(np.cos(2.0 * np.pi * 0.05 / warp * t + 0.3).astype(np.float32), g, 0, n)[0]
    assert float(np.sqrt(np.mean(y[1024:n - 1024] ** 2))) > 0.3
