"""CPU checks of the f0 tracker's specification as tests/f0_model.py restates it (DESIGN.md "Pitch tracking"): the integer ranges the kernel's
accumulators rely on, the frames that give empty and unvoiced records, the accuracy of the period against closed-form tones, and the planner's rows.
The device is compared with this model bit for bit in tests/test_gpu_f0.py, the C planner in tests/test_f0_abi.py."""
import math

import numpy as np
import pytest

import f0_model as FM

BIG = dict(W=1024, min_lag=32, max_lag=1024)
SMALL = dict(W=64, min_lag=2, max_lag=64)


# ---- invariants -----------------------------------------------------------------------------------------------------------------------------

def test_integer_ranges_on_a_full_scale_square_wave_at_the_largest_shape():
    """|q| <= 2048, d <= 2^36 and the dividend d tau 2^14 < 2^62 at W = max_lag = 4096.  The peak sits one ulp under 1.0, which rounds to q = 2048; the half
    period 100 does not divide 4096, so the full-flip lags (d = 2^36) stay below 4096."""
    W = ML = 4096
    n = np.arange(W + ML)
    x = np.where((n // 100) % 2 == 0, 1.0, -1.0).astype(np.float32) * np.nextafter(np.float32(1), np.float32(0))
    q = FM.quantise(x)
    assert int(np.max(np.abs(q))) == 2048
    d, cum, c = FM.curves(q, W, ML)
    assert int(d.max()) == 1 << 36                                         # lag 100: every sample flips
    tau = np.arange(ML + 1)
    assert max(int(a) * int(b) << 14 for a, b in zip(d, tau)) < 1 << 62
    assert int(cum.max()) < 1 << 49 and int(c.max()) < 1 << 31 and int(c.min()) >= 0
    rec = FM.pick(c, 2, ML, FM.DEFAULT_THRESHOLD)
    assert rec[0] == 200 and rec[2] == 0


def test_records_do_not_depend_on_the_amplitude():
    rng = np.random.default_rng(5)
    x = (FM.tone("harm", 100.37, 3000) + 0.01 * rng.standard_normal(3000)).astype(np.float32)
    a = FM.track(x, 257, 64, 2, 300)
    b = FM.track((x * np.float32(2.0 ** -13)).astype(np.float32), 257, 64, 2, 300)
    assert a.shape[0] > 30 and np.array_equal(a, b) and np.all(a[:, 0] > 0)


def test_empty_and_unvoiced_frames():
    W, ML = 64, 64
    assert FM.record(np.zeros(W + ML, np.float32), W, 2, ML) == [0, 0, 0, 0]
    x = FM.tone("sine", 20.0, W + ML)
    x[77] = np.nan
    assert FM.record(x, W, 2, ML) == [0, 0, 0, 0]
    x[77] = -np.inf
    assert FM.record(x, W, 2, ML) == [0, 0, 0, 0]
    rec = FM.record(np.full(W + ML, 0.3, np.float32), W, 2, ML)            # DC: d == 0 everywhere, cum == 0, c == 2^14
    assert rec == [-2, 16384, 16384, 16384] and FM.period(rec) == 0.0
    noise = np.random.default_rng(7).standard_normal(1024 + 1024 + 20 * 256).astype(np.float32)
    recs = FM.track(noise, 1024, 256, 32, 1024)
    assert recs.shape[0] == 21 and np.all(recs[:, 0] < 0)                  # white noise: no voiced frame


def test_thresholds_at_both_ends():
    x = FM.tone("harm", 23.3, 128)
    c = FM.curves(FM.quantise(x), 64, 64)[2]
    assert c[2:64].min() > 0 and FM.pick(c, 2, 64, 1)[0] < 0                # only c == 0 is under threshold 1: no multiple of 23.3 under 64 is whole
    assert FM.pick(c, 2, 64, 16384)[0] > 0                                  # every c below 2^14 is under the largest threshold
    n = np.arange(128)
    square = np.where((n // 10) % 2 == 0, 0.5, -0.5).astype(np.float32)     # period 20 exactly: c(20) == 0
    assert FM.record(square, 64, 2, 64, 1)[:3:2] == [20, 0]


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------------------

def _worst(geometry, periods, hop, nframes, kinds=("sine", "harm", "missing"), amplitudes=(0.9, 1e-4)):
    worst = {}
    for p in periods:
        for kind in kinds:
            for amp in amplitudes:
                x = FM.tone(kind, p, geometry["W"] + geometry["max_lag"] + (nframes - 1) * hop, amp)
                recs = FM.track(x, geometry["W"], hop, geometry["min_lag"], geometry["max_lag"])
                assert recs.shape[0] == nframes and np.all(recs[:, 0] > 0), (p, kind, amp, recs[:, 0])
                err = max(abs(FM.period(r) - p) / p for r in recs)
                worst[kind] = max(worst.get(kind, 0.0), err)
    return worst


def test_period_of_closed_form_tones_at_window_1024():
    """Sine, harmonics 1 .. 8 at 1 / k and a missing fundamental (harmonics 2 .. 6), periods 40.0 .. 900.0 samples, amplitudes 0.9 and 1e-4, five frames at
    hop 256: every frame voiced, relative period error under 1.5e-3.  Measured with this file: sine 9.7e-4 (worst: period 733.21), harmonics 3.8e-4,
    missing fundamental 3.5e-4."""
    worst = _worst(BIG, (40.0, 100.37, 217.3, 480.5, 733.21, 900.0), 256, 5)
    print("worst relative period error at W = 1024:", worst)
    assert max(worst.values()) <= 1.5e-3, worst


def test_period_of_closed_form_tones_at_window_64():
    """The same at W = 64, lags 2 .. 64, periods 20.0, 31.5 and 50.2, hop 16: under 3e-3.  Measured with this file: sine 1.6e-3, harmonics 2.7e-3, missing fundamental 2.1e-3.  (Period 7.3 measures 1e-2 at this
    window: seven samples per period leave the parabola too coarse, it is not a pitch-accuracy case.)"""
    worst = _worst(SMALL, (20.0, 31.5, 50.2), 16, 5)
    print("worst relative period error at W = 64:", worst)
    assert max(worst.values()) <= 3e-3, worst


# ---- the planner ------------------------------------------------------------------------------------------------------------------------------

def _note(freq, mask=0xFFF):
    return FM.nearest_allowed(69.0 + 12.0 * math.log2(freq / 440.0), mask)


@pytest.mark.parametrize("freq", FM.PLAN_TONES)
def test_plan_moves_a_detuned_tone_onto_its_note(freq):
    """strength = retune = 1, chromatic: the mean hop is 256 f / f_note within 1e-3 relative (the tracker's bound; the error diffusion adds at most half a
    sample over the row).  Measured: at most 7e-5."""
    recs = FM.plan_records(freq)
    assert np.all(recs[:, 0] > 0)
    hops, r = FM.plan(recs)
    want = 256.0 * freq / FM.note_frequency(_note(freq))
    print(freq, "mean hop", hops.mean(), "want", want, "relative", abs(hops.mean() - want) / want)
    assert abs(hops.mean() - want) / want <= 1e-3
    assert np.all((hops >= 128) & (hops <= 512))
    total = int(hops.sum())
    assert total <= FM.PLAN_LEN < total + 512                               # the row never passes input_len, and stops only when the next hop would


def test_plan_with_a_slow_retune_approaches_the_target_monotonically():
    recs = FM.plan_records(452.0)
    target = math.log2(440.0 / 452.0)                                       # octaves, negative: down to A4
    hops, r = FM.plan(recs, retune=0.25)
    # r_m = t (1 - 0.75^(m + 1)) for a constant target t: strictly monotone while the remaining gap, 0.75^m |t|, is far above the frame-to-frame jitter of
    # the tracked t; twelve frames leave 3 % of the gap.  The tracker's bound of 1.5e-3 relative on the period is log2(1.0015) = 2.2e-3 octaves on t
    tol = math.log2(1.0015)
    assert np.all(np.diff(r[:12]) < 0) and np.all(r > target - tol)
    assert abs(r[-1] - target) <= tol
    assert np.all(np.diff(hops[:12].astype(int)) >= -1)                     # the hop row follows, up to the rounding of the error diffusion
    assert hops[0] < hops[-1] and abs(hops[-8:].mean() - 256.0 * 452.0 / 440.0) <= 0.5


def test_plan_with_a_scale_mask_goes_to_the_nearest_allowed_class():
    freq = 470.0                                                            # 0.14 above A#4, which C major lacks: B4 (0.86 away) beats A4 (1.14 away)
    assert _note(freq) == 70 and _note(freq, FM.C_MAJOR) == 71
    recs = FM.track(FM.plan_tone(freq), **FM.PLAN_GEOMETRY)
    hops, _ = FM.plan(recs, scale_mask=FM.C_MAJOR)
    want = 256.0 * freq / FM.note_frequency(71)
    assert abs(hops.mean() - want) / want <= 1e-3


def test_nearest_note_ties_go_down_and_wrap_across_octaves():
    assert FM.nearest_allowed(60.5, 0xFFF) == 60                            # a tie between 60 and 61
    assert FM.nearest_allowed(61.0, 0b000000000101) == 60                   # C and D allowed: C#4 ties, down to C
    assert FM.nearest_allowed(59.2, 0b000000000001) == 60 and FM.nearest_allowed(65.9, 0b000000000001) == 60 and FM.nearest_allowed(66.1, 0b000000000001) == 72
    assert FM.nearest_allowed(-3.4, 0b100000000000) == -1                   # negative notes keep their class: -1 is a B


def test_plan_leaves_the_pitch_alone_without_strength_or_voicing():
    recs = FM.plan_records(452.0)
    hops, r = FM.plan(recs, strength=0.0)
    assert hops.size == FM.PLAN_LEN // 256 and np.all(hops == 256) and np.all(r == 0.0)
    unvoiced = np.array(recs)
    unvoiced[:, 0] = -unvoiced[:, 0]
    hops, r = FM.plan(unvoiced)
    assert hops.size == FM.PLAN_LEN // 256 and np.all(hops == 256)
    hops, _ = FM.plan(np.zeros((0, 4), np.int32))
    assert np.all(hops == 256)
    for bad in (dict(scale_mask=0), dict(scale_mask=0x1000), dict(strength=1.5), dict(retune=0.0), dict(min_hop=0), dict(max_hop=100)):
        with pytest.raises(ValueError):
            FM.plan(recs, **bad)
