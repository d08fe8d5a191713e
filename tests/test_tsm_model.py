"""CPU checks of time-scale modification on the overlap-add path as tests/tsm_model.py defines it (DESIGN.md "Time-scale modification"): at rate 1 the
planner is tests/epoch_model.py's bit for bit, its centres ascend, its grains cover the output, the output has the length the rates ask for and every
tile's source range fits the staged span; the model's process is tests/psola_model.py's on near tables; a stretched voice keeps its period and its
envelope.  The C planner is compared with the model bit for bit in tests/test_tsm_abi.py, the kernel against it in tests/test_gpu_tsm.py."""
import numpy as np
import pytest

import epoch_model as EM
import f0_model as FM
import psola_model as PM
import test_epoch_model as TEM
import test_psola_model as TPM
import tsm_model as TM

SR = FM.SAMPLE_RATE
HOP = 256


# ---- the planner ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(16))
def test_at_rate_one_the_plan_is_epoch_plans(seed):
    """rates None or all 1.0: V == T throughout, so the grains are EM.epoch_plan's after the change of notation, with and without epoch records, and the
    output is as long as the input."""
    recs, ratios, kw = TEM.track_arguments(seed)
    nrec = recs.shape[0]
    ep = TEM.random_epochs(np.random.default_rng(300 + seed), nrec)
    moved = 0
    for epochs in (None, ep):
        want = TM.from_psola(EM.epoch_plan(recs, ratios=ratios, epochs=epochs, **kw))
        for rates in (None, np.ones(nrec)):
            g, n = TM.tsm_plan(recs, ratios=ratios, rates=rates, epochs=epochs, **kw)
            assert g.dtype == np.int32 and np.array_equal(g, want), (seed, epochs is None, rates is None)
            assert n == kw["input_len"]
            assert TM.check_grains(g, kw["max_period"]) is None and TM.is_near(g, kw["max_period"])
            assert np.array_equal(TM.to_psola(g), EM.epoch_plan(recs, ratios=ratios, epochs=epochs, **kw))
        moved += int(np.sum(want[:, 2] != 0) + np.sum(want[:, 1] >= 256))
    assert moved > 100


def random_rates(rng, nrec, R, ends=30):
    """Per record, log-uniform in [1 / R, R]; constant over the first and the last `ends` records."""
    r = np.exp(rng.uniform(-np.log(R), np.log(R), nrec))
    r[:ends] = r[0]
    r[-ends:] = r[-1]
    return np.clip(r, 1.0 / R, float(R))


def _covered(g, n):
    """How many grains reach each output of [0, n): output j is inside (c / 256 - L, c / 256 + L)."""
    c = g[:, 0] * 256 + (g[:, 1] & 255)
    first = np.floor_divide(c - 256 * g[:, 3], 256) + 1
    last = -np.floor_divide(-(c + 256 * g[:, 3]), 256) - 1
    cover = np.zeros(n + 2 * TM.MAX_PERIOD + 4, np.int64)
    np.add.at(cover, np.clip(first, 0, n + 1), 1)
    np.add.at(cover, np.clip(last + 1, 0, n + 1), -1)
    return np.cumsum(cover)[:n]


@pytest.mark.parametrize("seed", range(24))
def test_order_coverage_and_span_over_random_tracks(seed):
    """Random voiced / unvoiced tracks (the tracks of tests/test_psola_model.py, ratios in [1/2, 2]) at random rates in [1 / R, R] per record, R = 2 and 4,
    max_period 64 / 256 / 1024, with and without epoch records: centres strictly ascending, every output of [max_period, output_len - max_period)
    covered, and every tile, of the one call and of a call that starts at an odd output, within span(max_period, R)."""
    recs, ratios, _ = TPM._random_track(seed)
    nrec = recs.shape[0]
    mp = (64, 256, 1024)[seed % 3]
    R = (2, 4)[(seed // 3) % 2]
    rng = np.random.default_rng(500 + seed)
    rates = random_rates(rng, nrec, R)
    ep = TEM.random_epochs(rng, nrec) if seed % 4 >= 2 else None
    n = nrec * 64 - (0, 37)[seed % 2]
    g, nout = TM.tsm_plan(recs, 64, 32, n, float(min(96, mp)), 20, mp, ratios=ratios, rates=rates, epochs=ep, lock=(EM.DEFAULT_LOCK, 1.0)[seed % 2])
    g = g.astype(np.int64)
    assert TM.check_grains(g, mp) is None
    c = g[:, 0] * 256 + (g[:, 1] & 255)
    assert np.all(np.diff(c) > 0) and c[0] == 0
    assert n / R - (2 * mp + 1) <= nout <= n * R + (2 * mp + 1)
    cover = _covered(g, nout)
    assert np.all(cover[min(mp, nout):max(nout - mp, 0)] >= 1)
    cap = TM.span(mp, R)
    extents = np.concatenate([TM.tiles(g, mp, 0, nout)[:, 3], TM.tiles(g, mp, 777, nout - 777)[:, 3]])
    frac = float(extents.max()) / cap
    print(f"seed {seed} max_period {mp} R {R}: {g.shape[0]} grains, output {nout} of input {n}, worst tile extent {extents.max()} = {frac:.3f} of span {cap}")
    assert np.all(extents <= cap), (int(extents.max()), cap)
    assert TM.check_span(g, mp, R, 0, nout) is None
    # rates outside [1/4, 4] are held there
    wild = np.where(np.arange(nrec) % 2 == 0, rates * 100.0, rates / 100.0)
    held, held_len = TM.tsm_plan(recs, 64, 32, n, float(min(96, mp)), 20, mp, ratios=ratios, rates=np.clip(wild, 0.25, 4.0), epochs=ep)
    got, got_len = TM.tsm_plan(recs, 64, 32, n, float(min(96, mp)), 20, mp, ratios=ratios, rates=wild, epochs=ep)
    assert np.array_equal(got, held) and got_len == held_len


@pytest.mark.parametrize("mp,R", [(64, 1), (64, 2), (64, 3), (64, 4), (256, 2), (256, 4), (1024, 2), (1024, 4), (4096, 1)])
def test_the_span_at_the_highest_rate_and_the_longest_period(mp, R):
    """The budget's own corner: the rate R throughout, periods at max_period and at its half, the ratios 1/2, 1 and 2, voiced and unvoiced, marks snapped at
    once onto arbitrary epoch records.  The grains that reach a tile have their centres within max_period of it, read positions R times as far apart, analysis
    marks within a period of those, and every grain reads max_period to either side."""
    rng = np.random.default_rng(mp + R)
    worst = 0
    for period in (float(mp), mp / 2.0, -float(mp)):
        for ratio in (0.5, 1.0, 2.0):
            nrec = (8 * 1024 * R + 8 * mp) // 64
            recs = PM.records_of([period] * nrec)
            ep = TEM.random_epochs(rng, nrec, 2 * min(mp, 2048))
            for epochs in (None, ep):
                g, nout = TM.tsm_plan(recs, 64, 32, nrec * 64, float(mp), min(20, mp), mp, ratios=np.full(nrec, ratio), rates=np.full(nrec, float(R)), epochs=epochs, lock=1.0)
                for first in (0, 511):
                    worst = max(worst, int(TM.tiles(g, mp, first, nout - first)[:, 3].max()))
    print(f"max_period {mp} rate {R}: worst tile extent {worst} = {worst / TM.span(mp, R):.3f} of span {TM.span(mp, R)}")
    assert worst <= TM.span(mp, R)


@pytest.mark.parametrize("rate", [0.25, 0.5, 0.8, 1.0, 1.7, 2.0, 4.0])
def test_an_all_voiced_track_at_a_constant_rate_has_the_length_over_the_rate(rate):
    for period, ratio, mp in ((217.3, 1.0, 1024), (100.37, 1.25, 512), (480.5, 0.8, 512), (40.0, 2.0, 64), (300.0, 0.5, 300)):
        n = 20000
        recs = PM.records_of([period] * (n // 64 + 1))
        g, nout = TM.tsm_plan(recs, 64, 32, n, float(min(128, mp)), 20, mp, ratios=np.full(recs.shape[0], ratio), rates=np.full(recs.shape[0], rate))
        cap = 2 * mp - 4
        assert abs(nout - n / rate) <= cap + 1, (period, ratio, nout, n / rate)
        assert abs(nout - n / rate) <= 1                                         # in fact the marks are two exact lattices: half a sample of rounding
        # the synthesis marks advance by P / ratio, the analysis marks used by rate times that
        c = (g[:, 0].astype(np.int64) * 256 + (g[:, 1] & 255)) / 256.0
        step = min(min(max(FM.period(recs[0]), 20.0), mp) / ratio, cap)
        assert np.all(np.abs(np.diff(c) - step) <= 1.01 / 256.0)
        assert TM.check_span(g, mp, TM.MAX_RATE, 0, nout) is None


def test_unvoiced_material_passes_at_whole_sample_shifts_at_any_rate():
    """Under unvoiced records every grain after the first marks has phi = 0: a pure copy.  At half speed every mark is used about twice, at double speed
    every other one.  The read position snaps onto the marks, so in an unvoiced stretch a rate is realised as a whole pattern of mark reuse: exactly where
    the rate or its inverse is a whole number, else only nearly (0.3 comes out as 5 / 12 and 3.1 as 3: the documented limit); the duration promise is for voiced
    material."""
    n = 6000
    recs = PM.records_of([-50.0] * (n // 64))
    x = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    for rate in (0.5, 1.0, 2.0, 0.3, 3.1):
        g, nout = TM.tsm_plan(recs, 64, 32, n, 128.0, 20, 512, rates=np.full(recs.shape[0], rate))
        assert np.all(g[2:, 1] < 256), (rate, nout)
        src = g[:, 0].astype(np.int64) - g[:, 2]                                # the analysis mark of every grain
        assert np.all(np.diff(src) >= 0) and np.all(src % 128 == 0)
        uses = np.bincount(src // 128)
        print(f"unvoiced at rate {rate}: output {nout} of input {n}, {uses[1:-1].mean():.2f} grains per mark")
        if rate in (0.5, 1.0, 2.0):
            assert abs(nout - n / rate) <= 2 * 512 and abs(uses[1:-1].mean() - 1.0 / rate) < 0.1 / rate, (rate, nout, uses.mean())
        else:
            assert n / 4 <= nout <= 4 * n
        y = TM.process(x, g, 0, nout)[0]
        if rate == 1.0:
            assert np.all(np.abs(y[512:-512] - x[512:-512]) <= 4.0 * np.spacing(np.abs(x[512:-512])))
        assert np.all(np.isfinite(y)) and np.all(_covered(g.astype(np.int64), nout)[512:nout - 512] >= 1)


def test_planner_arguments():
    recs = PM.records_of([100.0] * 8)
    base = dict(f0_hop=64, f0_center=32, input_len=512, unvoiced_period=100.0, min_period=20, max_period=512)
    for kw in (dict(rates=np.full(7, 1.0)), dict(rates=np.full(8, 0.0)), dict(rates=np.full(8, -1.0)), dict(rates=np.full(8, np.nan)), dict(rates=np.full(8, np.inf)),
               dict(lock=0.0), dict(min_strength=-1), dict(epochs=np.zeros((7, 4), np.int32)), dict(min_period=1), dict(ratios=np.full(8, 2.5)), dict(input_len=1 << 30)):
        with pytest.raises(ValueError):
            TM.tsm_plan(recs, **dict(base, **kw))
    g, n = TM.tsm_plan(recs, **dict(base, input_len=0))
    assert g.shape == (0, 4) and n == 0
    g, n = TM.tsm_plan(np.zeros((0, 4), np.int32), 64, 32, 1000, 100.0, 20, 512)          # no records: the unvoiced spacing at rate 1
    assert g[:, 3].tolist() == [100] * 10 and n == 1000 and np.all(g[:, 1:3] == 0)
    assert TM.span(1024, 4) == 16448 and TM.span(4096, 1) == 25664
    assert TM.lds_bytes(1024, 4) < TM.lds_bytes(4096, 1) <= TM.LDS_BYTES < TM.lds_bytes(4096, 2) < TM.lds_bytes(4096, 4)


# ---- the model's process ------------------------------------------------------------------------------------------------------------------------

def test_process_is_psola_models_on_near_tables():
    """A near table is psola's input after a change of notation: the same values, bound and poisoned outputs, to the bit."""
    rng = np.random.default_rng(8)
    n = 3 * 1024 + 37
    x = np.stack([rng.standard_normal(n), np.cos(0.05 * np.arange(n))]).astype(np.float32)
    x[1, 1500] = np.nan
    planned = PM.psola_plan(PM.records_of([217.3] * 30 + [-60.0] * 19), 64, 32, n, 128.0, 32, 512, ratios=np.full(49, 1.25))
    t = np.arange(0, n + 250, 47)
    mp = 300
    synthetic = np.stack([t, rng.integers(0, 256, t.size), rng.integers(-256 * mp, 256 * mp + 1, t.size), np.where(np.arange(t.size) % 2, 300, 32)], axis=1)
    synthetic[::5, 2] = (synthetic[::5, 2] >> 8) << 8
    synthetic[:2, 2] = [256 * mp, -256 * mp]
    for g, period in ((planned, 512), (synthetic, mp)):
        assert PM.check_grains(g, period) is None
        f = TM.from_psola(g)
        assert TM.check_grains(f, period) is None and TM.is_near(f, period) and np.array_equal(TM.to_psola(f), g)
        for first, count in ((0, n), (1001, 1500)):
            want = PM.process(x, g, first, count, bound=True)
            got = TM.process(x, f, first, count, bound=True)
            for a, b in zip(got, want):
                assert np.array_equal(a, b)
            assert np.array_equal(TM.process(x, f, first, count), want[0])
        assert TM.check_span(f, period, 1, 0, n) is None and TM.check_span(f, period, 1, 333, n) is None
    # a far grain reads where its D says, zeros outside the input
    one = np.array([[100, 0, -2000, 50], [300, 0, 5000, 50], [500, 256 * 128, 250, 50]], np.int32)
    y = TM.process(x[0], one, 0, 600)[0]
    assert np.all(np.abs(y[60:140] - x[0, 2060:2140]) <= 4 * np.spacing(np.abs(x[0, 2060:2140]))) and np.all(y[251:350] == 0.0) and np.any(y[460:540] != 0.0)
    assert TM.check_grains(one, 64) is None and not TM.is_near(one, 64)
    assert TM.check_span(one, 64, 1, 0, 600) == (0, 0, (150 + 2000 + 32) - (250 - 5000 - 33))
    for bad, why in (([[5, 65536, 0, 9]], "centre"), ([[5, -1, 0, 9]], "centre"), ([[5, 0, 1 << 30, 9]], "shift"), ([[5, 0, -(1 << 30), 9]], "shift"),
                     ([[5, 0, 0, 65]], "half length"), ([[5, 256 * 255 + 7, 0, 9], [5, 6, 0, 9]], "out of order")):
        assert TM.check_grains(np.array(bad), 64)[1] == why
    assert TM.check_grains(np.array([[5, 256 * 255 + 7, (1 << 30) - 1, 64], [5, 7, 1 - (1 << 30), 2]]), 64) is None


# ---- a stretched voice ----------------------------------------------------------------------------------------------------------------------------

PERIOD = TPM.PERIOD
RATES = (0.5, 2.0)
_env = {}


def _stretched(ratio, rate):
    """The voice of tests/test_psola_model.py, long enough that the output has N_ENV samples, through the plan at (ratio, rate) with its marks on the
    pulses: (p, output, grains, scale)."""
    key = (ratio, rate)
    if key not in _env:
        p = FM.period(PM.records_of([PERIOD])[0])
        n = int(TPM.N_ENV * max(rate, 1.0))
        x = PM.voice(p, n)
        f, a, _ = PM.harmonic_amplitudes(x, p, *TPM.FIT)
        scale = float(np.median(a / PM._resonator_response(f * SR, SR)))
        nrec = n // HOP
        g, nout = TM.tsm_plan(PM.records_of([PERIOD] * nrec), HOP, HOP // 2, n, 256.0, 32, 1024, ratios=np.full(nrec, ratio), rates=np.full(nrec, rate), offset=0.0)
        assert abs(nout - n / rate) <= 1 and nout >= TPM.N_ENV and TM.check_span(g, 1024, 4, 0, nout) is None
        _env[key] = (p, TM.process(x, g, 0, nout)[0], g, scale)
    return _env[key]


@pytest.mark.parametrize("ratio", [1.0, 1.25])
@pytest.mark.parametrize("rate", RATES)
def test_a_stretched_voice_has_the_period_over_the_ratio(ratio, rate):
    """PM.voice(217.3) at half and at double speed, unshifted and shifted by 1.25: three frames of the tracker in the middle of the output read p / ratio
    within the tracker's bound of 1.5e-3 relative (tests/test_psola_model.py applies the same)."""
    p, y, g, _ = _stretched(ratio, rate)
    assert (np.all(g[:, 2] == 0) and np.all(g[:, 1] < 256)) == (ratio == 1.0 and rate == 1.0)
    mid = y.size // 2
    recs = FM.track(y[mid - 1024:mid + 1024 + 2 * HOP].astype(np.float32), 1024, HOP, 16, 1024)
    assert recs.shape[0] == 3 and np.all(recs[:, 0] > 0), recs
    want = p / ratio
    err = max(abs(FM.period(r) - want) / want for r in recs)
    print(f"ratio {ratio} rate {rate}: period {want:.2f}, relative error {err:.2e}")
    assert err <= 1.5e-3, err


@pytest.mark.parametrize("ratio", [1.0, 1.25])
def test_a_stretched_voice_keeps_the_envelope(ratio):
    """The harness of tests/test_psola_model.py with the marks on the pulses: the deviation of a harmonic between 300 and 5000 Hz from the input's envelope at
    rates 1/2 and 2 is at most the figure at rate 1, computed here, plus 1 dB: the margin and the reasoning of the epoch gate (tests/test_epoch_model.py):
    over marks within a few samples of the pulse the figure moves by less than that.  Measured (dB) at ratio 1: 0.00 at the rates 1, 1/2 and 2; at ratio 1.25:
    4.16 at all three (the residual of the harmonic fit stays at 2e-4)."""
    p, y1, _, scale = _stretched(ratio, 1.0)
    _, _, base, res1 = TPM._peak_and_deviation(y1, p / ratio, scale)
    print(f"ratio {ratio} rate 1: deviation {base:.2f} dB, residual {res1:.1e}")
    for rate in RATES:
        _, y, _, _ = _stretched(ratio, rate)
        hz, a, dev, res = TPM._peak_and_deviation(y, p / ratio, scale)
        peak = float(hz[np.argmax(a)])
        print(f"ratio {ratio} rate {rate}: strongest {peak:.0f} Hz, deviation {dev:.2f} dB, residual {res:.1e}")
        assert dev <= base + 1.0, (rate, dev, base)
        assert abs(peak - 1200.0) < SR * ratio / p and res < 0.01
