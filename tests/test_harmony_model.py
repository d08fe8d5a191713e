"""CPU checks of the harmony model (tests/harmony_model.py) against the models it is built from: the ratio rule against tests/psola_model.py's one-pole
and against notes worked out by hand, the float32 fold, and the hull budget: voices planned by tsm_plan on one row of rates keep the hull of a tile
within the span of (max_period, max_rate)."""
import numpy as np
import pytest

import f0_model as FM
import harmony_model as HM
import psola_model as PM
import tsm_model as TM

C_MAJOR = sum(1 << k for k in (0, 2, 4, 5, 7, 9, 11))
SR = FM.SAMPLE_RATE


def _track(rng, nrec):
    """Voiced stretches of drifting period with unvoiced and empty records between them."""
    periods, p = [], 150.0
    while len(periods) < nrec:
        kind = rng.integers(0, 4)
        run = int(rng.integers(3, 20))
        if kind == 0:
            periods += [-60.0] * run
        elif kind == 1:
            periods += [0] * run
        else:
            p = float(rng.uniform(40.0, 900.0))
            periods += [p * (1.0 + 0.002 * k) for k in range(run)]
    return PM.records_of(periods[:nrec])


def test_degree_zero_is_the_psola_ratio_model_exactly():
    rng = np.random.default_rng(3)
    for mask, strength, retune in ((0xFFF, 1.0, 1.0), (C_MAJOR, 0.7, 0.25), (0x001, 1.0, 0.5), (0x821, 0.0, 1.0)):
        recs = _track(rng, 300)
        want = PM.tune_ratios(recs, SR, mask, strength, retune)
        got = HM.harmony_ratios(recs, SR, [0, 3, 0, -2], mask, strength, retune)
        assert got.shape == (4, 300) and np.array_equal(got[0], want) and np.array_equal(got[2], want)
        unvoiced = np.array([FM.period(r) <= 0.0 for r in recs])
        assert unvoiced.any() and np.array_equal(got[1][unvoiced], want[unvoiced]) and np.array_equal(got[3][unvoiced], want[unvoiced])     # i = 0 there
        assert np.any(got[1][~unvoiced] != want[~unvoiced])


def test_a_third_and_a_fifth_above_a3_in_c_major_are_c4_and_e4():
    """220 Hz is A3, note 57, in C major.  Two allowed notes up: B3, C4 = 3 semitones; four up: B3, C4, D4, E4 = 7 semitones.  Down two: G3, F3 = -4; down
    three: E3 = -5.  A little sharp of A3 the correction r is negative and every voice carries it."""
    for hz in (220.0, 223.0):
        recs = PM.records_of([SR / hz] * 8)
        lead = PM.tune_ratios(recs, SR, C_MAJOR)                              # the correction, 2^r
        got = HM.harmony_ratios(recs, SR, [0, 2, 4, -2, -3, 7, -7], C_MAJOR)
        assert np.array_equal(got[0], lead) and (np.all(np.abs(lead - 1.0) < 1e-5) if hz == 220.0 else np.all(lead < 0.99))
        for row, semis in zip(got, (0, 3, 7, -4, -5, 12, -12)):
            want = np.clip(lead * 2.0 ** (semis / 12.0), 0.5, 2.0)
            assert np.allclose(row, want, rtol=1e-14, atol=0.0), semis
        assert abs(got[1][0] / got[0][0] - 2.0 ** (3 / 12)) < 1e-12 and abs(got[2][0] / got[0][0] - 2.0 ** (7 / 12)) < 1e-12
    assert HM.interval(57, 2, C_MAJOR) == 3 and HM.interval(57, 4, C_MAJOR) == 7 and HM.interval(57, -2, C_MAJOR) == -4 and HM.interval(57, 0, C_MAJOR) == 0
    assert HM.interval(60, 7, C_MAJOR) == 12 and HM.interval(60, -7, C_MAJOR) == -12 and HM.interval(-3, 1, C_MAJOR) == 2 and HM.interval(-3, -1, C_MAJOR) == -2


def test_on_the_chromatic_mask_a_degree_is_a_semitone_and_the_clamp_is_the_octave():
    recs = PM.records_of([SR / 452.0] * 6 + [-60.0] * 3 + [0] * 2)
    lead = PM.tune_ratios(recs, SR, 0xFFF, 1.0, 0.5)
    r = np.log2(lead)
    degrees = [0, 1, -1, 5, 12, -12, 24, -24]
    got = HM.harmony_ratios(recs, SR, degrees, 0xFFF, 1.0, 0.5)
    voiced = np.arange(11) < 6
    for row, k in zip(got, degrees):
        want = np.clip(lead * 2.0 ** (np.where(voiced, k, 0) / 12.0), 0.5, 2.0)
        assert np.allclose(row, want, rtol=1e-14, atol=0.0), k
    # 452 Hz is sharp of A4: r < 0, so an octave up stays just inside the clamp, an octave down and two octaves either way saturate
    assert np.all(r[:6] < 0.0) and np.all(got[4][:6] < 2.0) and np.all(got[5][:6] == 0.5) and np.all(got[6][:6] == 2.0) and np.all(got[7][:6] == 0.5)
    assert np.array_equal(got[6][6:], got[0][6:]) and np.array_equal(got[7][6:], got[0][6:])                      # unvoiced and empty records: i = 0
    # a one-note scale: every degree is an octave
    one = HM.harmony_ratios(PM.records_of([SR / 440.0] * 3), SR, [0, 1, -1, 2], 1 << 9)
    assert np.allclose(one[1:], np.clip(one[0] * np.array([[2.0], [0.5], [4.0]]), 0.5, 2.0), rtol=1e-14, atol=0.0) and np.all(one[3] == 2.0)


def test_bad_arguments_are_refused():
    recs = PM.records_of([200.0] * 4)
    for kw in (dict(degrees=[]), dict(degrees=[0] * 9), dict(degrees=[25]), dict(degrees=[-25]), dict(scale_mask=0), dict(scale_mask=0x1000), dict(strength=1.5),
               dict(retune=0.0), dict(sample_rate=0.0), dict(a4=-1.0)):
        args = dict(records=recs, sample_rate=SR, degrees=[0, 2])
        args.update(kw)
        with pytest.raises(ValueError):
            HM.harmony_ratios(**args)
    assert HM.harmony_ratios(recs, SR, [24, -24] * 4).shape == (8, 4)
    assert HM.harmony_ratios(np.zeros((0, 4), np.int32), SR, [0, 2]).shape == (2, 0)


def test_the_fold_is_float32_in_voice_order_and_skips_muted_and_uncovered_voices():
    rng = np.random.default_rng(11)
    ys = rng.standard_normal((3, 2, 50)).astype(np.float32)
    covered = rng.random((3, 50)) < 0.7
    gains = np.array([[0.3, 0.0], [-1.7, 0.25], [0.5, 0.5]], np.float32)
    ys[1, 1, 7] = np.nan
    ys[0, 1, 9] = np.inf                                                     # under a muted voice: stays out
    got = HM.mix(ys, covered, gains)
    for c in range(2):
        for n in range(50):
            acc = np.float32(0.0)
            for v in range(3):
                if gains[v, c] != 0.0 and covered[v, n]:
                    acc = np.float32(acc + np.float32(gains[v, c] * ys[v, c, n]))
            assert (np.isnan(acc) and np.isnan(got[c, n])) or acc == got[c, n]
    assert np.isfinite(got[1, 9]) and (np.isnan(got[1, 7]) == bool(covered[1, 7]))
    none = ~covered.any(axis=0)
    assert none.any() and np.all(got[:, none] == 0.0)
    # process(): TM.process per voice, then the fold; one voice at gain 1 is TM.process rounded to float32
    x = rng.standard_normal((2, 3000)).astype(np.float32)
    g = np.array([[t, 0, 0, 40] for t in range(0, 3000, 31)], np.int32)
    far = np.array([[t, 256 * 77, -100, 50] for t in range(500, 2000, 41)], np.int32)
    y1 = HM.process(x, [g], [1.0])
    assert y1.dtype == np.float32 and np.array_equal(y1, TM.process(x, g).astype(np.float32) + np.float32(0.0))
    y2 = HM.process(x, [g, far, np.zeros((0, 4), np.int32)], [[0.5, 0.5], [0.25, 0.0], [9.0, 9.0]], 100, 2500)
    a, b = TM.process(x, g, 100, 2500).astype(np.float32), TM.process(x, far, 100, 2500).astype(np.float32)
    assert np.array_equal(y2[1], np.float32(0.5) * a[1])
    hit = np.abs(b[0]) > 0
    assert hit.any() and np.array_equal(y2[0][hit], (np.float32(0.5) * a[0] + np.float32(0.25) * b[0])[hit])
    yb, tol, poisoned = HM.process(x, [g, far], [0.5, 0.25], 100, 2500, bound=True)
    assert not poisoned.any() and np.all(np.abs(HM.process(x, [g, far], [0.5, 0.25], 100, 2500) - yb) <= tol)


def test_tiles_give_the_hull_and_per_voice_ranges():
    a = np.array([[t, 0, 0, 40] for t in range(0, 3000, 31)], np.int32)
    b = np.array([[t, 256 * 77, -5000, 50] for t in range(1100, 2000, 41)], np.int32)         # no grain on tile 0 and only the first outputs of tile 2
    empty = np.zeros((0, 4), np.int32)
    hull, ranges = HM.tiles([a, b, empty], 64, 0, 3000)
    ta, tb = TM.tiles(a, 64, 0, 3000), TM.tiles(b, 64, 0, 3000)
    assert hull.shape == (3, 2) and ranges.shape == (3, 3, 2)
    assert list(hull[0]) == list(ta[0, 2:]) and tb[0, 3] == 0                                # a voice without a grain on the tile is left out of the hull
    assert hull[1, 0] == min(ta[1, 2], tb[1, 2]) and hull[1, 0] + hull[1, 1] == max(ta[1, 2] + ta[1, 3], tb[1, 2] + tb[1, 3]) and hull[1, 1] > 5000
    assert np.array_equal(ranges[:, 0], ta[:, :2]) and np.array_equal(ranges[:, 1], tb[:, :2] + a.shape[0]) and np.all(ranges[:, 2] == a.shape[0] + b.shape[0])
    assert TM.check_span(a, 64, 1, 0, 3000) is None and TM.check_span(b, 64, 1, 0, 3000) is None           # each voice alone fits
    assert TM.span(64, 1) < 5000 and HM.check_span([a, b, empty], 64, 1, 0, 3000) == (1, 0, int(ta[1, 0]), int(hull[1, 1]))
    assert HM.check_span([b, a], 64, 1, 0, 3000)[:3] == (1, 0, int(tb[1, 0]))
    assert HM.check_span([a, b, empty], 64, 4, 0, 1024) is None
    none_hull, _ = HM.tiles([empty, empty], 64, 0, 2048)
    assert not none_hull.any()
    assert HM.check_voices([a, b, empty], 64) is None and HM.check_voices([a, b[::-1]], 64)[:2] == (1, 1) and HM.check_voices([a, b], 49)[:2] == (1, 0)


RATIOS = (1.0, 2.0 ** (3 / 12), 2.0 ** (7 / 12), 2.0 ** (-5 / 12), 2.0, 0.5)


def _planned(records, mp, nin, rate, ratios_rows):
    """One tsm_plan per voice on the same row of rates."""
    nrec = np.asarray(records).reshape(-1, 4).shape[0]
    f0_hop = 256
    out = [TM.tsm_plan(records, f0_hop, f0_hop // 2, nin, float(min(256, mp)), min(32, mp), mp, ratios=np.asarray(row, np.float64), rates=np.full(nrec, float(rate)))
           for row in ratios_rows]
    return [g for g, _ in out], [n for _, n in out]


def _worst_hull(tables, mp, R, nout):
    worst = single = 0
    for first in (0, 517):
        assert HM.check_span(tables, mp, R, first, nout - first) is None
        hull, _ = HM.tiles(tables, mp, first, nout - first)
        worst = max(worst, int(hull[:, 1].max()))
        single = max([single] + [int(TM.tiles(t, mp, first, nout - first)[:, 3].max()) for t in tables])
    return worst, single


@pytest.mark.parametrize("mp,R", [(64, 1), (64, 4), (256, 2), (256, 4), (1024, 2), (1024, 4), (4096, 1)])
def test_planned_voices_keep_the_hull_within_the_span(mp, R):
    """Six voices at the ratios 1, 2^(3/12), 2^(7/12), 2^(-5/12), 2 and 1/2 on a constant period near max_period, at rate 1 and at max_rate, tiles from
    outputs 0 and 517.  Worst hull / span seen here: 0.78 (64 / 1), 0.23 and 0.92 (64 / 4), 0.32 and 0.64 (256 / 2), 0.18 and 0.76 (256 / 4), 0.20 and
    0.44 (1024 / 2), 0.13 and 0.63 (1024 / 4), 0.18 (4096 / 1); the hull exceeds the widest single voice by at most 18 % (4096 / 1)."""
    period = mp - 1.7
    for rate in sorted({1, R}):
        nout = 6 * TM.TILE + 300
        nin = int(nout * rate)
        nrec = nin // 256 + 1
        recs = PM.records_of([period] * nrec)
        tables, lens = _planned(recs, mp, nin, rate, [np.full(nrec, q) for q in RATIOS])
        assert len(set(lens)) == 1 and abs(lens[0] - nout) <= 2 * mp, lens                       # one time base for all voices
        assert HM.check_voices(tables, mp) is None
        worst, single = _worst_hull(tables, mp, R, min(lens[0], nout))
        print(f"max_period {mp} max_rate {R} rate {rate}: worst hull {worst} = {worst / TM.span(mp, R):.3f} of the span, {worst / single:.3f} of the widest voice")
        assert single <= worst <= TM.span(mp, R)


def test_random_tracks_of_harmony_ratios_keep_the_hull_within_the_span():
    """Voiced and unvoiced stretches, the voices' ratios from harmony_ratios in C major at degrees (0, 2, 4, -3, 7, -7), rates 1, 1/2 and 2 at max_period 512 /
    max_rate 2."""
    rng = np.random.default_rng(23)
    mp, R = 512, 2
    worst = 0.0
    for rate in (1.0, 0.5, 2.0):
        nout = 5 * TM.TILE
        nin = int(nout * rate)
        nrec = nin // 256 + 1
        periods = []
        while len(periods) < nrec:
            run = int(rng.integers(2, 9))
            periods += [float(rng.uniform(60.0, 500.0))] * run if rng.random() < 0.7 else [-60.0] * run
        recs = PM.records_of(periods[:nrec])
        rows = HM.harmony_ratios(recs, SR, [0, 2, 4, -3, 7, -7], C_MAJOR, 1.0, 0.5)
        tables, lens = _planned(recs, mp, nin, rate, rows)
        n = min(lens)
        assert max(lens) - n <= 2 * mp and HM.check_voices(tables, mp) is None
        w, _ = _worst_hull(tables, mp, R, n)
        worst = max(worst, w / TM.span(mp, R))
    print(f"random tracks: worst hull / span = {worst:.3f}")
    assert worst <= 1.0
