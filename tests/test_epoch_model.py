"""CPU checks of the epoch records and of the epoch-aligned planner as tests/epoch_model.py defines them (DESIGN.md "Epoch marks"): without epoch
records the planner is tests/psola_model.py's bit for bit, the detector lands a constant few samples after the pulse at every phase, and with its
records the envelope deviation of the overlap-add path is the on-pulse figure whatever the phase of the input.  The C planner is compared with the
model bit for bit in tests/test_epoch_abi.py, the kernel in tests/test_gpu_epoch.py."""
import numpy as np
import pytest

import epoch_model as EM
import f0_model as FM
import psola_model as PM
import test_psola_model as TPM

SR = FM.SAMPLE_RATE
HOP = 256
WINDOW = 2048
MAX_PERIOD = 1024
PHASES = 8


def _p(period):
    """The period that records_of gives a tracker record for `period`, and its 1/256 form."""
    p = FM.period(PM.records_of([period])[0])
    return p, int(EM.periods(PM.records_of([period]))[0])


# ---- the planner without, and with arbitrary, epoch records --------------------------------------------------------------------------------------

def random_epochs(rng, nrec, window=WINDOW):
    """Arbitrary records: positions anywhere in a frame, a third without teeth, any strength."""
    return np.stack([rng.integers(0, window, nrec), rng.integers(0, 3, nrec) * rng.integers(1, 20, nrec), rng.integers(2, 512, nrec),
                     rng.integers(0, EM.S_ONE + 1, nrec)], axis=1).astype(np.int32)


def track_arguments(seed):
    """The planner arguments of tests/test_psola_model.py test_planner_properties_over_random_tracks."""
    recs, ratios, _ = TPM._random_track(seed)
    hop, mp = 64, (512, 300, 4096)[seed % 3]
    return recs, ratios, dict(f0_hop=hop, f0_center=hop // 2, input_len=recs.shape[0] * hop - (0, 37)[seed % 2], unvoiced_period=(96.0, 20.0, 300.0)[seed % 3],
                              min_period=20, max_period=mp)


@pytest.mark.parametrize("seed", range(6))
def test_without_epochs_the_plan_is_psola_plans_and_with_them_it_keeps_its_promises(seed):
    recs, ratios, kw = track_arguments(seed)
    want = PM.psola_plan(recs, ratios=ratios, **kw)
    assert np.array_equal(EM.epoch_plan(recs, ratios=ratios, **kw), want)
    assert np.array_equal(EM.epoch_plan(recs, **kw), PM.psola_plan(recs, **kw))
    rng = np.random.default_rng(100 + seed)
    ep = random_epochs(rng, recs.shape[0])
    assert np.array_equal(EM.epoch_plan(recs, ratios=ratios, epochs=np.zeros_like(ep), **kw), want)          # no teeth: no snap
    assert np.array_equal(EM.epoch_plan(recs, ratios=ratios, epochs=ep, min_strength=EM.S_ONE, **kw),
                          EM.epoch_plan(recs, ratios=ratios, epochs=np.where(ep[:, 3:] == EM.S_ONE, ep, 0), **kw))   # records under min_strength do not count
    moved = 0
    for lock in (EM.DEFAULT_LOCK, 1.0):
        g = EM.epoch_plan(recs, ratios=ratios, epochs=ep, lock=lock, **kw).astype(np.int64)
        assert PM.check_grains(g, kw["max_period"]) is None
        c = g[:, 0] * 256 + g[:, 1]
        assert np.all(np.diff(c) > 0) and c[0] == 0 and c[-1] < 256 * kw["input_len"]
        assert np.all(np.abs(g[:, 2]) <= 256 * kw["max_period"]) and np.all((g[:, 3] >= 2) & (g[:, 3] <= kw["max_period"]))
        k = min(len(g), len(want))
        moved += int(np.sum(g[:k, 2] != want[:k, 2]))
    assert moved > 100                                                            # the records do move the marks


def test_planner_arguments():
    recs = PM.records_of([100.0] * 8)
    base = dict(f0_hop=64, f0_center=32, input_len=512, unvoiced_period=100.0, min_period=20, max_period=512)
    for kw in (dict(lock=0.0), dict(lock=1.5), dict(lock=-0.125), dict(lock=float("nan")), dict(min_strength=-1), dict(min_strength=EM.S_ONE + 1),
               dict(epochs=np.zeros((7, 4), np.int32)), dict(min_period=1), dict(ratios=np.full(8, 2.5)), dict(input_len=1 << 30)):
        with pytest.raises(ValueError):
            EM.epoch_plan(recs, **dict(base, **kw))
    assert EM.epoch_plan(recs, **dict(base, input_len=0)).shape == (0, 4)
    assert EM.periods(PM.records_of([100.0, 0, -50.0, 217.3])).tolist() == [25600, 0, 0, int(np.floor(256 * FM.period(PM.records_of([217.3])[0]) + 0.5))]


# ---- the detector ---------------------------------------------------------------------------------------------------------------------------------

# measured with this file: position minus the nearest pulse, in samples, over eight phases and three frames (window 2048, hop 256)
MEASURED_LAG = {217.3: (5.86, 6.78), 100.37: (4.96, 5.91), 480.5: (4.25, 5.19)}


@pytest.mark.parametrize("period", [217.3, 100.37, 480.5])
def test_the_detector_trails_the_pulse_by_the_same_few_samples_at_every_phase(period):
    """PM.voice has a pulse at (phase + k) p.  The position of every record, less the nearest pulse, lies in a band a quarter period wide or less (the
    comb's own resolution is w = p / 4) -- measured: under one sample wide -- and inside the +-10 samples around the pulse over which the planner's
    envelope figures are flat (the offset scan of DESIGN.md "Epoch marks")."""
    p, p256 = _p(period)
    lags = []
    for j in range(PHASES):
        x = PM.voice(p, 8192, phase=j / PHASES)
        recs = EM.track(x, WINDOW, HOP, MAX_PERIOD, [p256] * 3)
        assert recs.shape == (3, 4) and np.all(recs[:, 1] >= 1) and np.all(recs[:, 2] == max(2, p256 >> 10)) and np.all(recs[:, 3] > EM.S_ONE // 2), recs
        for m in range(3):
            d = (m * HOP + int(recs[m, 0]) - j / PHASES * p) / p
            lags.append((d - np.floor(d + 0.5)) * p)
    lo, hi = min(lags), max(lags)
    print(f"period {period}: position - pulse in [{lo:+.2f}, {hi:+.2f}] samples; a quarter period is {p / 4:.1f}")
    assert hi - lo <= p / 4.0 and -10.0 <= lo and hi <= 10.0, (lo, hi)
    assert abs(lo - MEASURED_LAG[period][0]) < 0.02 and abs(hi - MEASURED_LAG[period][1]) < 0.02, (lo, hi)            # the record is an integer function: the figures do not move


def test_frames_without_a_record():
    p, p256 = _p(217.3)
    x = PM.voice(p, WINDOW)
    assert EM.record(x, p256, MAX_PERIOD)[1] >= 1
    assert EM.record(np.zeros(WINDOW, np.float32), p256, MAX_PERIOD) == [0, 0, 0, 0]
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[777] = v
        assert EM.record(y, p256, MAX_PERIOD) == [0, 0, 0, 0]
    for bad in (0, -p256, 256 * 8 - 1, 256 * MAX_PERIOD + 1, 1 << 30):
        assert EM.record(x, bad, MAX_PERIOD) == [0, 0, 0, 0]
    assert EM.record(x, 256 * 8, MAX_PERIOD)[1:3] == [(256 * (WINDOW - 4 - 8 + 2) - 1) // 2048 + 1, 2]
    assert EM.record(x, 256 * MAX_PERIOD, MAX_PERIOD)[1:3] == [1, 256]
    # a constant frame has no step anywhere: the first candidate, strength 0
    w = max(2, p256 >> 10)
    assert EM.record(np.full(WINDOW, 0.3, np.float32), p256, MAX_PERIOD)[::3] == [w, 0]
    # where the records are empty the planner leaves its marks alone: the grains of the unaligned path
    nrec = 8192 // HOP
    recs = PM.records_of([217.3] * nrec)
    silent = EM.track(np.zeros(8192, np.float32), WINDOW, HOP, MAX_PERIOD, [p256] * EM.frames(8192, WINDOW, HOP))
    ep = np.zeros((nrec, 4), np.int32)
    ep[:silent.shape[0]] = silent
    kw = dict(f0_hop=HOP, f0_center=HOP // 2, input_len=8192, unvoiced_period=256.0, min_period=32, max_period=MAX_PERIOD, ratios=np.full(nrec, 1.25))
    assert np.array_equal(EM.epoch_plan(recs, epochs=ep, **kw), PM.psola_plan(recs, **kw))


# ---- the envelope: the harness of tests/test_psola_model.py -----------------------------------------------------------------------------------------

N_ENV = TPM.N_ENV
RATIOS = (1.25, 1.5, 0.8)
# measured with this file at the default lock, the worst of eight phases: (deviation in dB, residual of the harmonic fit); on the pulses the unaligned
# path measures 4.16, 2.52 and 15.42 dB and half a period off 20.3, 23.0 and 25.3 dB (tests/test_psola_model.py)
MEASURED = {1.25: (3.57, 1.01e-2), 1.5: (2.56, 1.15e-2), 0.8: (14.32, 1.12e-2)}
_results = {}


@pytest.fixture(scope="module")
def voices():
    """Per phase j / 8: the voice and the model's epoch records of it, one per f0 record (zeros past the last whole frame)."""
    p, p256 = _p(TPM.PERIOD)
    nrec = N_ENV // HOP
    nf = EM.frames(N_ENV, WINDOW, HOP)
    out = []
    for j in range(PHASES):
        x = PM.voice(p, N_ENV, phase=j / PHASES)
        ep = np.zeros((nrec, 4), np.int32)
        ep[:nf] = EM.track(x, WINDOW, HOP, MAX_PERIOD, [p256] * nf)
        x.setflags(write=False)
        ep.setflags(write=False)
        out.append((x, ep))
    f, a, _ = PM.harmonic_amplitudes(out[0][0], p, *TPM.FIT)
    return p, float(np.median(a / PM._resonator_response(f * SR, SR))), PM.records_of([TPM.PERIOD] * nrec), out


def _aligned(voices, ratio, j, lock=EM.DEFAULT_LOCK):
    """(deviation dB, residual, strongest harmonic Hz) of phase j through the epoch-aligned plan; computed once per (ratio, j, lock)."""
    key = (ratio, j, lock)
    if key not in _results:
        p, scale, recs, vs = voices
        x, ep = vs[j]
        g = EM.epoch_plan(recs, HOP, HOP // 2, N_ENV, 256.0, 32, MAX_PERIOD, ratios=np.full(recs.shape[0], ratio), epochs=ep, lock=lock)
        assert PM.check_grains(g, MAX_PERIOD) is None
        hz, a, dev, res = TPM._peak_and_deviation(PM.process(x, g)[0], p / ratio, scale)
        _results[key] = (dev, res, float(hz[np.argmax(a)]))
    return _results[key]


@pytest.mark.parametrize("ratio", RATIOS)
def test_with_epoch_records_every_phase_has_the_on_pulse_envelope(voices, ratio):
    """The reference is the unaligned path with its marks on the pulses: PM.psola_plan(offset=0) on the phase-0 voice.  Every phase through the aligned
    plan deviates from the input's envelope by at most that figure plus 1 dB.  The margin: over marks within +-10 samples of the pulse the deviation moves by
    up to 1.9 dB, and over the detector's +4 .. +7 it is never more than 0.04 dB above the on-pulse figure (DESIGN.md "Epoch marks").  The strongest harmonic stays
    next to 1200 Hz."""
    p, scale, recs, vs = voices
    g0 = PM.psola_plan(recs, HOP, HOP // 2, N_ENV, 256.0, 32, MAX_PERIOD, ratios=np.full(recs.shape[0], ratio), offset=0.0)
    _, _, on_pulse, res0 = TPM._peak_and_deviation(PM.process(vs[0][0], g0)[0], p / ratio, scale)
    print(f"ratio {ratio}: unaligned with the marks on the pulses {on_pulse:.2f} dB, residual {res0:.1e}")
    worst = 0.0
    for j in range(PHASES):
        dev, res, peak = _aligned(voices, ratio, j)
        print(f"ratio {ratio} phase {j}/8: strongest {peak:6.0f} Hz, deviation {dev:5.2f} dB, residual {res:.1e}")
        assert dev <= on_pulse + 1.0, (j, dev, on_pulse)
        assert abs(peak - 1200.0) < SR * ratio / p, (j, peak)
        worst = max(worst, dev)
    assert abs(worst - MEASURED[ratio][0]) < 0.05, worst                       # the figure quoted in DESIGN.md


@pytest.mark.parametrize("ratio", RATIOS)
def test_the_lock_keeps_the_half_sample_of_the_records_out_of_the_marks(voices, ratio):
    """The residual of the harmonic fit is what is not periodic at p / ratio: mark jitter.  At the default lock it is gated at twice the measured figure (the
    convention of this test family; the unaligned path, whose marks are an exact lattice, measures 3e-4), and snapping every mark (lock = 1) is worse at
    every phase."""
    worst = max(_aligned(voices, ratio, j)[1] for j in range(PHASES))
    print(f"ratio {ratio}: worst residual at the default lock {worst:.2e}")
    assert worst <= 2.0 * MEASURED[ratio][1], worst
    for j in range(PHASES):
        hard = _aligned(voices, ratio, j, lock=1.0)[1]
        print(f"ratio {ratio} phase {j}/8: residual {_aligned(voices, ratio, j)[1]:.2e} at the default lock, {hard:.2e} at lock 1")
        assert hard > _aligned(voices, ratio, j)[1]
