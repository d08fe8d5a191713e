"""CPU checks of the pitch-synchronous overlap-add path as tests/psola_model.py defines it (DESIGN.md "Pitch-synchronous correction"): an unshifted
plan is transparent, a shifted tone has the period p / ratio, the spectral envelope stays where it was (and moves with the pitch through the stretch
and the resampler, which is the point of the path), and the planner keeps its promises over random period and ratio tracks.  The C planner is
compared with the model bit for bit in tests/test_psola_abi.py, the kernel against it in tests/test_gpu_psola.py."""
import numpy as np
import pytest

import f0_model as FM
import psola_model as PM
import stretch_model as SM
import vari_model as VM

SR = FM.SAMPLE_RATE
HOP = 256


def _plan(period, n, ratio=None, offset=0.0, max_period=1024):
    recs = PM.records_of([period] * (n // HOP))
    ratios = None if ratio is None else np.full(recs.shape[0], ratio)
    return FM.period(recs[0]), PM.psola_plan(recs, HOP, HOP // 2, n, 256.0, 16, max_period, ratios=ratios, offset=offset)


def test_ratio_one_returns_the_input_within_four_ulp():
    """Every grain of an unshifted plan has dq = 0 and reads the samples themselves: y = (sum h x) / (sum h) = x.  Away from the ends, where every
    output is covered, the fp64 model is within 4 ulp of the f32 input (measured: 0)."""
    n, mp = 8192, 1024
    x = FM.tone("harm", 100.37, n)
    _, grains = _plan(100.37, n)
    assert np.all(grains[:, 2] == 0)
    y = PM.process(x, grains)[0]
    mid = slice(mp, n - mp)
    err = np.abs(y[mid] - x[mid].astype(np.float64))
    print("ratio 1: worst error in ulp", float(np.max(err / np.spacing(np.abs(x[mid]) + np.float32(1e-30)))))
    assert np.all(err <= 4.0 * np.spacing(np.abs(x[mid]).astype(np.float32)))


@pytest.mark.parametrize("period", [40.0, 100.37, 217.3, 480.5])
def test_a_shifted_tone_has_the_period_over_the_ratio(period):
    """Harmonics 1 .. 8 at 1 / k shifted by 0.8, 1.25 and 1.5: three frames of the tracker (window 1024, lags 16 .. 1024) in the middle of the output read
    p / ratio within the tracker's documented bound, 1.5e-3 relative for periods from 40 samples and 3e-3 for the shorter ones (tests/test_f0_model.py)."""
    n = 8192
    x = FM.tone("harm", period, n)
    for ratio in (0.8, 1.25, 1.5):
        p, grains = _plan(period, n, ratio)
        y = PM.process(x, grains)[0].astype(np.float32)
        recs = FM.track(y[2048:2048 + 2048 + 2 * HOP], 1024, HOP, 16, 1024)
        assert recs.shape[0] == 3 and np.all(recs[:, 0] > 0), (ratio, recs)
        want = p / ratio
        err = max(abs(FM.period(r) - want) / want for r in recs)
        print(f"period {period} ratio {ratio}: relative error {err:.2e}")
        assert err <= (1.5e-3 if want >= 40.0 else 3e-3), (ratio, err)


# ---- the envelope -----------------------------------------------------------------------------------------------------------------------------

PERIOD = 217.3
N_ENV = 16384
FIT = (3000, 13000)
# measured with this file (dB): the largest deviation of a harmonic between 300 and 5000 Hz from the input's envelope, with the analysis marks on the
# pulses and the worst of eight mark offsets across one period; the gates are twice these, the convention of tests/test_vari_model.py
MEASURED = {1.25: (4.2, 20.3), 1.5: (2.5, 23.0), 0.8: (15.4, 25.3)}


def _peak_and_deviation(y, period, scale):
    f, a, res = PM.harmonic_amplitudes(y, period, *FIT)
    hz = f * SR
    sel = (hz >= 300.0) & (hz <= 5000.0)
    dev = 20.0 * np.log10(a[sel] / (scale * PM._resonator_response(hz[sel], SR)))
    return hz, a, float(np.max(np.abs(dev))), res


@pytest.fixture(scope="module")
def voice():
    p = FM.period(PM.records_of([PERIOD])[0])
    x = PM.voice(p, N_ENV)
    x.setflags(write=False)
    f, a, res = PM.harmonic_amplitudes(x, p, *FIT)
    env = PM._resonator_response(f * SR, SR)
    assert res < 1e-6 and np.ptp(a / env) < 1e-3 * np.median(a / env)          # the input is its envelope sampled at the harmonics
    return p, x, float(np.median(a / env))


@pytest.mark.parametrize("ratio", [1.25, 1.5, 0.8])
def test_the_envelope_stays_and_the_pitch_moves(voice, ratio):
    """A pulse train of period 217.3 through resonators at 1200 and 2600 Hz.  After the shift the output is periodic at p / ratio (residual of the
    harmonic fit under 1 %) and its strongest harmonic is still at the first formant: one of the two harmonics on either side of 1200 Hz, and not the
    harmonic nearest 1200 * ratio, for every one of eight mark offsets across one period.  At 1.25 and 1.5 it is the harmonic nearest 1200 Hz; at 0.8
    the harmonics of the output on either side of the formant are 1060 and 1237 Hz and the stronger is 1060 Hz: the two input harmonics that feed
    1237 Hz lie on opposite sides of the resonance and arrive in opposite phase.  The deviation from the input's envelope is gated at twice MEASURED."""
    p, x, scale = voice
    nrec = N_ENV // HOP
    recs = PM.records_of([PERIOD] * nrec)
    worst, on_pulse = 0.0, None
    for j in range(8):
        offset = (j / 8.0 - 0.5) * p
        grains = PM.psola_plan(recs, HOP, HOP // 2, N_ENV, 256.0, 32, 1024, ratios=np.full(nrec, ratio), offset=offset)
        y = PM.process(x, grains)[0]
        hz, a, dev, res = _peak_and_deviation(y, p / ratio, scale)
        peak = float(hz[np.argmax(a)])
        f0 = SR * ratio / p
        assert res < 0.01, (j, res)
        assert abs(peak - 1200.0) < f0, (j, peak)
        assert peak != float(hz[np.argmin(np.abs(hz - 1200.0 * ratio))]), (j, peak)
        if ratio > 1.0:
            assert peak == float(hz[np.argmin(np.abs(hz - 1200.0))]), (j, peak)
        worst = max(worst, dev)
        if j == 4:
            on_pulse = dev
        print(f"ratio {ratio} offset {offset:+7.1f}: strongest {peak:6.0f} Hz, deviation {dev:5.2f} dB, residual {res:.1e}")
    print(f"ratio {ratio}: deviation with the marks on the pulses {on_pulse:.2f} dB, worst offset {worst:.2f} dB")
    assert on_pulse <= 2.0 * MEASURED[ratio][0] and worst <= 2.0 * MEASURED[ratio][1], (on_pulse, worst)


@pytest.mark.parametrize("ratio,hs,ha", [(1.25, 320, 256), (1.5, 384, 256), (0.8, 256, 320)])
def test_the_stretch_and_the_resampler_move_the_envelope_with_the_pitch(voice, ratio, hs, ha):
    """The same input through the time stretch and the variable-ratio resampler (the glide's path): the strongest harmonic lands at the harmonic nearest
    1200 * ratio, which is what the overlap-add path avoids."""
    p, x, _ = voice
    n = (8192 // ha) * ha
    s = SM.StretchModel(1024, ha, hs).process(x[None, :n])
    frames = n // ha
    y = VM.VariModel(hs, ha, ha).process(s, np.full(frames, ha))[0]
    f, a, _ = PM.harmonic_amplitudes(y, p / ratio, 3000, n - 1000)
    hz = f * SR
    peak = float(hz[np.argmax(a)])
    print(f"ratio {ratio}: strongest harmonic through the stretch and the resampler {peak:.0f} Hz")
    assert peak == float(hz[np.argmin(np.abs(hz - 1200.0 * ratio))]) and abs(peak - 1200.0) > SR * ratio / p / 2


# ---- the planner ------------------------------------------------------------------------------------------------------------------------------

def _random_track(seed):
    """Segments of 60 records at hop 64: voiced at a random period and ratio, unvoiced (negative lag) or empty."""
    rng = np.random.default_rng(seed)
    periods, ratios = [], []
    for s in range(10):
        kind = rng.integers(0, 4) if s else 1
        if kind == 0:
            p, r = (0.0 if rng.integers(0, 2) else -float(rng.integers(20, 300))), float(rng.uniform(0.5, 2.0))
        else:
            p, r = float(rng.uniform(20.0, 300.0)), float(rng.choice([0.5, 2.0, rng.uniform(0.5, 2.0)]))
        periods += [p] * 60
        ratios += [r] * 60
    recs = PM.records_of(periods)
    return recs, np.array(ratios), np.array([FM.period(r) for r in recs])


@pytest.mark.parametrize("seed", range(6))
def test_planner_properties_over_random_tracks(seed):
    hop, seg, mp, lo = 64, 60 * 64, (512, 300, 4096)[seed % 3], 20
    recs, ratios, periods = _random_track(seed)
    n = recs.shape[0] * hop - (0, 37)[seed % 2]
    unv = (96.0, 20.0, 300.0)[seed % 3]
    g = PM.psola_plan(recs, hop, hop // 2, n, unv, lo, mp, ratios=ratios).astype(np.int64)
    assert PM.check_grains(g, mp) is None
    c = g[:, 0] * 256 + g[:, 1]
    assert np.all(np.diff(c) > 0) and c[0] == 0 and c[-1] < 256 * n                 # strictly ascending, from 0, below the input's end
    assert np.all(np.abs(g[:, 2]) <= 128 * mp + 256) and np.all((g[:, 3] >= 2) & (g[:, 3] <= mp))
    # every output away from the ends is covered: n is inside (c / 256 - L, c / 256 + L) for some grain
    first = np.floor_divide(c - 256 * g[:, 3], 256) + 1
    last = -np.floor_divide(-(c + 256 * g[:, 3]), 256) - 1
    cover = np.zeros(n + 2 * mp + 2, np.int64)
    np.add.at(cover, np.clip(first, 0, None), 1)
    np.add.at(cover, np.clip(last + 1, 0, None), -1)
    cover = np.cumsum(cover)[:n]
    assert np.all(cover[min(mp, n):max(n - mp, 0)] >= 1)
    cap = 2 * mp - 4
    for s in range(recs.shape[0] // 60):
        s0, s1 = s * seg, min((s + 1) * seg, n)
        inside = np.nonzero((c >= 256 * (s0 + 1)) & (c < 256 * (s1 - 1)))[0]
        if periods[s * 60] > 0.0:
            # a voiced run of constant period and ratio: the centres advance by P / ratio (at most cap); T stays in fp64, so no rounding error accumulates
            if inside.size >= 2:
                step = min(min(max(periods[s * 60], lo), mp) / ratios[s * 60], cap)
                m = inside.size - 1
                assert abs((c[inside[-1]] - c[inside[0]]) / 256.0 - m * step) <= 1.01 / 256.0, (s, m)
        else:
            # an unvoiced stretch: after the first marks the synthesis marks sit on analysis marks
            deep = inside[c[inside] >= 256 * (s0 + 3 * max(unv, 300.0))]
            assert np.all(g[deep, 2] == 0), (s, g[deep, 2])
            if deep.size >= 2:
                assert np.all(np.diff(c[deep]) == np.diff(c[deep])[0]) or np.ptp(np.diff(c[deep])) <= 1
    # ratios = None plans 1 everywhere: every shift is 0
    assert np.all(PM.psola_plan(recs, hop, hop // 2, n, unv, lo, mp)[:, 2] == 0)


def test_unvoiced_material_passes_within_a_few_ulp():
    """Noise under unvoiced records: every grain has dq = 0, so the output is the input (4 ulp; measured 0) once the marks have snapped."""
    n = 6000
    x = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    recs = PM.records_of([-50.0] * (n // 64))
    g = PM.psola_plan(recs, 64, 32, n, 128.0, 20, 512, ratios=np.full(recs.shape[0], 1.7))
    assert np.all(g[:, 2] == 0)
    y = PM.process(x, g)[0]
    assert np.all(np.abs(y[512:-512] - x[512:-512]) <= 4.0 * np.spacing(np.abs(x[512:-512])))


def test_planner_arguments():
    recs = PM.records_of([100.0] * 8)
    for kw in (dict(min_period=1), dict(max_period=4097), dict(min_period=300, max_period=200), dict(unvoiced_period=10.0), dict(unvoiced_period=600.0),
               dict(input_len=-1), dict(input_len=1 << 30), dict(f0_hop=0), dict(ratios=np.full(8, 2.5)), dict(ratios=np.full(8, 0.4)), dict(ratios=np.full(7, 1.0)),
               dict(ratios=np.full(8, np.nan))):
        args = dict(f0_hop=64, f0_center=32, input_len=512, unvoiced_period=100.0, min_period=20, max_period=512)
        args.update(kw)
        with pytest.raises(ValueError):
            PM.psola_plan(recs, **args)
    assert PM.psola_plan(recs, 64, 32, 0, 100.0, 20, 512).shape == (0, 4)
    assert PM.psola_plan(np.zeros((0, 4), np.int32), 64, 32, 1000, 100.0, 20, 512)[:, 3].tolist() == [100] * 10      # no records: the unvoiced spacing
    r = PM.tune_ratios(FM.plan_records(452.0), SR)
    assert np.all(np.abs(r - 440.0 / 452.0) < 1.5e-3) and PM.tune_ratios(np.zeros((3, 4), np.int32), SR).tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError):
        PM.tune_ratios(recs, SR, scale_mask=0)
