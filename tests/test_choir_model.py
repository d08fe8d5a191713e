"""CPU checks of full-grain harmony voices on the overlap-add path as tests/choir_model.py defines them (DESIGN.md "Choir"): the model is its siblings'
wherever a sibling can say the table (formant_model without mirrored grains, mirror_model without warped ones, harmony_model on plain tables), with ==;
the mirrored warped grain reads the position the contract states and is the forward warped grain on the reversed input; every tap of a covered output
lies inside the range the tile stages; planned tables keep to the span at its corners, mirrored and with six voices; and the planner is mirror_plan and
formant_plan where either can say the plan.  The C planner and tile walk are compared with the model in tests/test_choir_abi.py, the kernel in
tests/test_gpu_choir.py."""
import numpy as np
import pytest

import choir_model as CM
import formant_model as FoM
import harmony_model as HM
import mirror_model as MM
import psola_model as PM
import test_epoch_model as TEM
import test_formant_abi as TFA
import test_gpu_harmony as TGH
import test_gpu_tsm as TGT
import test_mirror_model as TMM
import tsm_model as TM

STEP = CM.STEP
BIT = CM.MIRROR
STEPS = TFA.STEPS                                                           # (128, 129, 200, 255, 257, 300, 511, 512)
NOUT = TGT.NOUT


def mirror_table(g, every=2, start=1):
    """The far table g with every `every`-th grain mirrored about the position its forward twin reads at its centre: D' = 2 t - D, so it reads the same stretch
    of the input, backwards.  Fractions stay."""
    m = np.array(g, np.int64).reshape(-1, 4)
    k = np.arange(start, m.shape[0], every)
    m[k, 1] += BIT
    m[k, 2] = 2 * m[k, 0] - m[k, 2]
    return np.ascontiguousarray(m, np.int32)


def full_table(g, mode):
    """The far table g with the full grain word.  mode "thirds": grain i is mirrored for i % 3 == 0, warped for i % 3 == 1 and mirrored and warped for
    i % 3 == 2, every third grain of each kind, and every tenth grain (i % 10 == 9) stays plain, so all four kinds meet in one tile.  mode "all": every grain
    is mirrored and warped.  Steps are drawn in turn from STEPS; on the mirrored warped grains phi is forced through 0, 1, 255 and the table's own value, tf
    through 0, 255 and its own value where that keeps the centres in order (test_formant_abi.warp_table's rule).  A mirrored grain gets D' = 2 t - D: it reads
    about the position its forward twin reads at its centre."""
    m = np.array(g, np.int64).reshape(-1, 4)
    i = np.arange(m.shape[0])
    if mode == "all":
        mir = wr = np.ones(m.shape[0], bool)
    else:
        plain = i % 10 == 9
        mir, wr = ~plain & (i % 3 != 1), ~plain & (i % 3 != 0)
    tf, phi = m[:, 1] & 255, (m[:, 1] >> 8) & 255
    for j, k in enumerate(np.flatnonzero(mir & wr).tolist()):
        if j % 4 < 3:
            phi[k] = (0, 1, 255)[j % 4]
        alone = (k == 0 or m[k - 1, 0] < m[k, 0]) and (k == m.shape[0] - 1 or m[k + 1, 0] > m[k, 0])
        if alone and (j // 4) % 3 < 2:
            tf[k] = (0, 255)[(j // 4) % 3]
    m[:, 1] = tf + 256 * phi
    w = np.flatnonzero(wr)
    m[w, 1] += STEP * np.array(STEPS)[np.arange(w.size) % len(STEPS)]
    m[mir, 1] += BIT
    m[mir, 2] = 2 * m[mir, 0] - m[mir, 2]
    return np.ascontiguousarray(m, np.int32)


# ---- the model against its siblings ---------------------------------------------------------------------------------------------------------------

def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", ["small", "mid", "tiny", "huge", "sweep", "gap", "empty", "slow"])
def test_one_voice_is_formant_model_without_mirrored_grains_and_mirror_model_without_warped_ones(name):
    """voice() (values, bound and poisoned outputs), tiles, check_grains and check_span with == on the tables of tests/test_gpu_tsm.py, plain, with every third
    grain warped, with all grains warped, and with every second grain mirrored; process() with one voice at gain 1 is the float32 of the sibling's output."""
    mp, R, nin, g = TGT._grains(name)
    x = TGT._signals(nin, 3)[:2]
    x[1, nin // 2] = np.nan
    mp_f = min(mp, 3753)
    for table, sib in ((g, FoM), (TFA.warp_table(g), FoM), (TFA.warp_table(g, 1, 0), FoM), (g, MM), (mirror_table(g), MM), (mirror_table(g, 1, 0), MM)):
        assert CM.check_grains(table, mp) is None and sib.check_grains(table, mp) is None
        for first, count in ((0, NOUT), (1001, 1500)):
            want = sib.process(x, table, first, count, bound=True)
            _same(CM.voice(x, table, first, count, bound=True), want)
            assert np.array_equal(CM.voice(x, table, first, count), want[0], equal_nan=True)
            one = CM.process(x, [table], [1.0], first, count)
            assert one.dtype == np.float32 and np.array_equal(one, want[0].astype(np.float32), equal_nan=True)
            assert np.array_equal(CM.tiles(table, mp, first, count), sib.tiles(table, mp, first, count))
            hull, ranges = CM.hull([table], mp, first, count)
            t = sib.tiles(table, mp, first, count)
            assert np.array_equal(hull, t[:, 2:]) and np.array_equal(ranges[:, 0], t[:, :2])
        if sib is FoM:                                                         # the span is formant_model's; mirror_model's is narrower
            bad = FoM.check_span(table, mp_f, 1, 0, NOUT)
            got = CM.check_span([table], mp_f, 1, 0, NOUT)
            assert (got is None) == (bad is None) and (bad is None or got == (bad[0], 0, bad[1], bad[2]))
    assert CM.span is FoM.span and CM.fits is FoM.fits and CM.span(1024, 2) == MM.span(1024, 2) + 2 * 1024 + 128


def test_check_grains_is_each_siblings_on_the_tables_that_sibling_can_say():
    """Random single-field damage to a table: the verdict is formant_model's where no grain is mirrored and mirror_model's where none is warped, apart from the
    name of the reason for a bad word, which is "step" here and "centre" in mirror_model."""
    rng = np.random.default_rng(4)
    mp, R, nin, g = TGT._grains("small")
    checked = 0
    for table, sib in ((TFA.warp_table(g), FoM), (mirror_table(g), MM)):
        for _ in range(60):
            bad = np.array(table, np.int64)
            col = rng.integers(0, 4)
            bad[rng.integers(0, g.shape[0]), col] = rng.choice([-1, 1, 65535, 1 << 30, -(1 << 30), mp + 1, 5, 1 << 27, 127 * STEP, 513 * STEP])
            want = sib.check_grains(bad, mp)
            if sib is FoM and CM.mirrored(bad).any() or sib is MM and np.any((bad[:, 1] >= 2 * BIT) | (bad[:, 1] < 0)):
                continue                                                     # the damage made a word the sibling refuses for a reason of its own
            assert CM.check_grains(bad, mp) == want, (bad, want)
            checked += want is not None
    assert checked > 40
    for bad, why in (([[5, 1 << 27, 0, 9]], "step"), ([[5, -1, 0, 9]], "step"), ([[5, BIT + 127 * STEP, 0, 9]], "step"), ([[5, BIT + STEP, 0, 9]], "step"),
                     ([[5, BIT + 513 * STEP + 7, 0, 9]], "step"), ([[-1, BIT, 0, 9]], "centre"), ([[1 << 30, BIT + 300 * STEP, 0, 9]], "centre"),
                     ([[5, 300 * STEP, 1 << 30, 9]], "shift"), ([[5, BIT + 300 * STEP, -(1 << 30), 9]], "shift"), ([[5, 300 * STEP, -(1 << 30), 9]], "shift"),
                     ([[5, BIT + 128 * STEP + 7, 0, 65]], "half length"), ([[5, BIT + 512 * STEP + 7, 0, 9], [5, 200 * STEP + 6, 0, 9]], "out of order")):
        assert CM.check_grains(np.array(bad), 64)[1] == why, bad
    assert CM.check_grains(np.array([[5, BIT + 128 * STEP + 65535, (1 << 31) - 1, 64], [5, BIT + 512 * STEP + 65535, 1 - (1 << 30), 2],
                                     [5, BIT + 256 * STEP + 65535, 1 << 30, 2], [5, 512 * STEP + 65535, (1 << 30) - 1, 2]]), 64) is None
    assert CM.check_voices([g, np.array([[5, 7, 0, 9], [5, 6, 0, 9]])], mp) == (1, 1, "out of order")


@pytest.mark.parametrize("name", ["small2", "small8", "mid2"])
def test_plain_voices_are_harmony_models(name):
    """The voices of tests/test_gpu_harmony.py, plain far tables: process (the float32 fold and the bounded form), the hull, the ranges and check_span, ==."""
    mp, R, nin, tables = TGH._voices(name)
    nv = len(tables)
    x = TGT._signals(nin, 11 + len(name))[:2]
    gains = np.random.default_rng(99 + nv).uniform(-1.5, 1.5, (nv, 2)).astype(np.float32)
    gains[nv - 1, 1] = 0.0
    assert np.array_equal(CM.process(x, tables, gains, 0, NOUT), HM.process(x, tables, gains, 0, NOUT))
    _same(CM.process(x, tables, gains, 777, 1200, bound=True), HM.process(x, tables, gains, 777, 1200, bound=True))
    for first, count in ((0, NOUT), (777, NOUT - 777)):
        a, b = CM.hull(tables, mp, first, count), HM.tiles(tables, mp, first, count)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert CM.check_voices(tables, mp) is None and CM.check_span(tables, mp, R, 0, NOUT) is None
    wide = [np.array(t) for t in tables]
    wide[1][:, 2] -= 3 * CM.span(mp, R)
    assert CM.check_span(wide, mp, R, 0, NOUT)[:3] == HM.check_span(wide, mp, R, 0, NOUT)[:3]


# ---- the new grain --------------------------------------------------------------------------------------------------------------------------------

def test_a_mirrored_warped_grain_reads_the_position_the_contract_states():
    """On a ramp x[p] = p an interpolated sample is its position: (D - t - tf / 256 - phi / 256) - (s / 256) (n - t - tf / 256), at every step and fraction; at
    s = 256 written as z = 256 the rule is the mirrored grain's, and the integers land where the contract says they do."""
    ramp = np.arange(6000, dtype=np.float32)
    for s in STEPS:
        for tf, phi in ((0, 0), (200, 77), (255, 255), (0, 1), (255, 0), (0, 255), (255, 1)):
            t, D, L = 500, 3500, 100
            y = CM.voice(ramp, np.array([[t, tf + 256 * phi + BIT + STEP * s, D, L]]), 0, 700)[0]
            k = np.arange(t - L + 1, t + L)
            want = (D - t - tf / 256.0 - phi / 256.0) - (s / 256.0) * (k - t - tf / 256.0)
            assert np.all(np.abs(y[k] - want) < 4e-3), (s, tf, phi, float(np.max(np.abs(y[k] - want))))       # the interpolator's error on a ramp
            assert np.all(y[:t - L] == 0.0) and np.all(y[t + L + 1:] == 0.0)
    rng = np.random.default_rng(1)
    t, tf, phi = rng.integers(0, 1 << 20, 2000), rng.integers(0, 256, 2000), rng.integers(0, 256, 2000)
    D, n = rng.integers(-(1 << 20), 1 << 21, 2000), t + rng.integers(-4096, 4097, 2000)
    m, r = CM._m(t, tf, phi, D, 256, True, n)
    assert np.array_equal(m, np.where(phi == 0, D - n, D - n - 1)) and np.array_equal(r, np.where(phi == 0, 0, 256 * (256 - phi)))
    x = TGT._signals(4000, 2)[:1]
    for phi in (0, 1, 77, 255):
        g = np.array([[500, 9 + 256 * phi + BIT, 2500, 100]])
        assert np.array_equal(CM.voice(x, g + [0, 256 * STEP, 0, 0], 0, 700), MM.process(x, g, 0, 700))


def test_a_mirrored_warped_grain_is_the_forward_warped_grain_on_the_reversed_input():
    """A mirrored warped grain (D, phi) on x against the forward warped grain on x[::-1] with (D - N + 1, 0) for phi = 0 and (D - N, 256 - phi) otherwise, N the
    input length: the same real positions, so the same taps with the same distances, but met in the opposite order (tap i of one is tap 2 W - 1 - i of the
    other, shifted by one where r = 0), so the sums round differently: the two agree within the sum of their derived bounds, not in bits.  Worst
    |diff| / (bound + bound) seen: 5.2e-11 (the model sums in fp64; the bounds are the f32 kernel's, which tests/test_gpu_choir.py holds the kernel to)."""
    rng = np.random.default_rng(12)
    worst = 0.0
    N = 5000
    x = TGT._signals(N, 9)
    for s in STEPS:
        t = np.sort(rng.integers(0, 700, 12))
        tf, phi = rng.integers(0, 256, 12), rng.choice([0, 1, 255, 77, 128], 12)
        order = np.argsort(256 * t + tf, kind="stable")
        t, tf, phi = t[order], tf[order], phi[order]
        D = t + rng.integers(-100, N + 100, 12)                                # reads inside the input and across both of its ends
        L = rng.integers(2, 65, 12)
        m = np.stack([t, tf + 256 * phi + BIT + STEP * s, D, L], axis=1)
        f = np.stack([t, tf + 256 * np.where(phi == 0, 0, 256 - phi) + STEP * s, np.where(phi == 0, D - N + 1, D - N), L], axis=1)
        assert CM.check_grains(m, 64) is None and FoM.check_grains(f, 64) is None
        a, ta, pa = CM.voice(x, m, 0, 800, bound=True)
        b, tb, pb = FoM.process(x[:, ::-1], f, 0, 800, bound=True)
        assert np.array_equal(ta > 0, tb > 0) and np.array_equal(pa, pb) and np.any(a != 0.0)
        live = ta > 0
        worst = max(worst, float(np.max(np.abs(a - b)[live] / (ta + tb)[live])))
        assert np.all(np.abs(a - b) <= ta + tb), s
    print(f"mirror symmetry: worst |diff| / (bound + bound) = {worst:.3e}")
    assert worst < 1.0


def test_every_tap_of_every_covered_output_lies_inside_the_range_of_its_tile():
    """Brute force on random tables of all four kinds: for every tile, every grain that reaches it and every output of the tile the grain covers with a non-zero
    window weight, the taps lie within [lo + 2, hi - 1] of the grain's range on that tile for a mirrored warped grain (and a forward warped one), and within
    [lo + 1, hi - 1] for the unwarped kinds, as their headers state."""
    rng = np.random.default_rng(7)
    Hn = PM.window()
    seen = {(0, 0): 0, (0, 1): 0, (1, 0): 0, (1, 1): 0}
    for trial in range(40):
        mp = int(rng.choice([8, 64, 300]))
        first, nout = int(rng.integers(0, 3000)), int(rng.integers(1, 2500))
        ng = 30
        t = np.sort(rng.integers(max(first - 2 * mp, 0), first + nout + 2 * mp, ng))
        tf = np.sort(rng.integers(0, 256, ng)) if trial % 5 == 0 else rng.integers(0, 256, ng)
        order = np.argsort(256 * t + tf, kind="stable")
        t, tf = t[order], tf[order]
        phi = rng.choice([0, 1, 255, 100], ng)
        s = rng.choice([0, 128, 129, 200, 255, 256, 257, 300, 511, 512], ng)
        mir = rng.integers(0, 2, ng)
        D = rng.integers(-5000, 5000, ng)
        L = rng.integers(2, mp + 1, ng)
        for k in range(ng):
            grain = np.array([[t[k], tf[k] + 256 * phi[k] + BIT * mir[k] + STEP * s[k], D[k], L[k]]], np.int64)
            assert CM.check_grains(grain, mp) is None
            step = 256 if s[k] == 0 else int(s[k])
            for tile, (a, b, lo, cnt) in enumerate(CM.tiles(grain, mp, first, nout).tolist()):
                j0 = first + tile * 1024
                j1 = min(j0 + 1024, first + nout)
                n = np.arange(max(j0, t[k] - L[k] - 1), min(j1, t[k] + L[k] + 2), dtype=np.int64)
                if n.size == 0:
                    continue
                n = n[PM.grain_weights(n, int(t[k]), int(tf[k]), int(L[k]), Hn)[2]]
                if n.size == 0:
                    continue
                assert (a, b) == (0, 1) and cnt > 0
                if step == 256:
                    at = D[k] - n if mir[k] else n - D[k]
                    low, high = (at.min(), at.max()) if phi[k] == 0 else (at.min() - 32, at.max() + 31)
                    assert lo + 1 <= low and high <= lo + cnt - 1
                else:
                    W = 32 if step < 256 else 64
                    m = CM._m(int(t[k]), int(tf[k]), int(phi[k]), int(D[k]), step, bool(mir[k]), n)[0]
                    assert lo + 2 <= m.min() - W + 1 and m.max() + W <= lo + cnt - 1
                seen[(int(mir[k]), int(step != 256))] += n.size
    assert all(v > 2000 for v in seen.values()), seen


# ---- the planner ----------------------------------------------------------------------------------------------------------------------------------

def _warps(seed, nrec):
    w = np.random.default_rng(700 + seed).uniform(0.5, 2.0, nrec)
    w[::7] = 1.0
    w[1::7] = 0.5
    w[2::7] = 2.0
    return w


_both = {"grains": 0}


@pytest.mark.parametrize("seed", range(24))
def test_the_plan_is_mirror_plan_without_warps_and_formant_plan_without_mirror(seed):
    """On the 24 random tracks of tests/test_tsm_model.py: warps=None is mirror_plan bit for bit (mirror on and off), mirror=False formant_plan bit for bit;
    with both the plan differs from mirror_plan in L and in bits 17 .. 26 of w only, L and z are formant_plan's for every grain, and a mirrored warped grain
    reads its own analysis mark at its centre.  Every tile of the full plan stays within the span."""
    args, kw, mp, R = TMM.track(seed)
    nrec = np.asarray(args[0]).reshape(-1, 4).shape[0]
    warps = _warps(seed, nrec)
    for mirror in (False, True):
        want = MM.mirror_plan(*args, mirror=mirror, **kw)
        got = CM.choir_plan(*args, warps=None, mirror=mirror, **kw)
        assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and got[1] == want[1]
        got = CM.choir_plan(*args, warps=np.ones(nrec), mirror=mirror, **kw)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]          # the step 256 is written as z = 0
    fo, fo_len = FoM.formant_plan(*args, warps=warps, **kw)
    got = CM.choir_plan(*args, warps=warps, mirror=False, **kw)
    assert np.array_equal(got[0], fo) and got[1] == fo_len
    mi, mi_len = MM.mirror_plan(*args, mirror=True, **kw)
    g, n, A, voiced = CM.choir_plan(*args, warps=warps, mirror=True, details=True, **kw)
    assert g.dtype == np.int32 and g.shape == mi.shape and n == mi_len == fo_len and CM.check_grains(g, mp) is None
    g = g.astype(np.int64)
    assert np.array_equal(g[:, [0, 2]], mi[:, [0, 2]]) and np.array_equal(g[:, 1] & 0x1FFFF, mi[:, 1])
    assert np.array_equal(g[:, 3], fo[:, 3]) and np.array_equal(g[:, 1] >> 17, fo[:, 1] >> 17) and np.any(g[:, 3] != mi[:, 3])
    both = CM.mirrored(g) & CM.warped(g)
    _both["grains"] += int(both.sum())
    # D - t - tf / 256 - phi / 256, the position of the contract at the grain's centre, is the mark A to the two roundings of the planner
    centre = 256 * g[both, 2] - ((g[both, 1] >> 8) & 255) - (256 * g[both, 0] + (g[both, 1] & 255))
    assert np.all(np.abs(centre - 256.0 * A[both]) <= 1.0) and not np.any(both & voiced)
    assert CM.check_span([g], mp, R, 0, n) is None and CM.check_span([g], mp, R, 777, max(n - 777, 0)) is None
    for bad in (dict(warps=np.full(nrec, 0.49)), dict(warps=np.full(nrec, 2.01)), dict(warps=np.full(nrec, np.nan)), dict(warps=np.ones(nrec + 1)), dict(mirror=2)):
        with pytest.raises(ValueError):
            CM.choir_plan(*args, **dict(kw, **bad))
    if seed == 23:
        assert _both["grains"] > 60, _both                                   # the tracks are mostly voiced


# ---- the span -------------------------------------------------------------------------------------------------------------------------------------

PAIRS = [(mp, R) for R in (1, 2, 3, 4) for mp in (64, 256, 1024, 2048, max(m for m in range(1024, 4097) if CM.fits(m, R))) if CM.fits(mp, R)]
CORNER = [(ratio, warp) for ratio in (0.5, 1.0, 2.0) for warp in (0.5, 2.0)]                                    # tests/test_formant_model.py's corner, as six voices
CHORD = list(zip((1.0, 2.0 ** (3 / 12), 2.0 ** (7 / 12), 2.0 ** (-5 / 12), 2.0, 0.5), (1.0, 0.5, 2.0, 0.8, 1.25, 2.0)))      # harmony's ratios, mixed warps
_table = {}


@pytest.mark.parametrize("mp,R", PAIRS)
def test_planned_voices_keep_the_hull_within_the_span_at_its_corners(mp, R):
    """tests/test_formant_model.py's corner sweep (the rate R throughout, periods at max_period and at its half, ratios 1/2, 1 and 2, voiced and unvoiced, marks
    snapped onto arbitrary epoch records, steps 1/2 and 2, tiles from outputs 0 and 511) with mirror = 1, and at the rate 1 / R as well, where the unvoiced
    track has its reuses and so its mirrored warped grains.  Every plan is held to the span alone (the sweep of that file with mirror = 1), and so is the hull
    of six voices on one row of rates: the six corner plans together, and six voices at harmony's ratios with mixed warps."""
    assert (1024, 4) in PAIRS and (3753, 1) in PAIRS and (1925, 4) in PAIRS and len(PAIRS) == 19
    rng = np.random.default_rng(mp + R)
    cap = CM.span(mp, R)
    alone = corner = chord = both = 0
    for period in (float(mp), mp / 2.0, -float(mp)):
        for rate in (float(R), 1.0 / R):
            nrec = int(4 * 1024 * rate + 8 * mp) // 64
            recs = PM.records_of([period] * nrec)
            ep = TEM.random_epochs(rng, nrec, 2 * min(mp, 2048))
            for epochs in (None, ep):
                for voices, name in ((CORNER, "corner"), (CHORD, "chord")):
                    plans = [CM.choir_plan(recs, 64, 32, nrec * 64, float(mp), min(20, mp), mp, ratios=np.full(nrec, ratio), rates=np.full(nrec, rate),
                                           warps=np.full(nrec, warp), epochs=epochs, lock=1.0, mirror=True) for ratio, warp in voices]
                    tables = [g for g, _ in plans]
                    nout = plans[0][1]
                    both += sum(int((CM.mirrored(g) & CM.warped(g)).sum()) for g in tables)
                    for first in (0, 511):
                        per = max(int(CM.tiles(g, mp, first, nout - first)[:, 3].max()) for g in tables)
                        hull = int(CM.hull(tables, mp, first, nout - first)[0][:, 1].max())
                        alone = max(alone, per)
                        if name == "corner":
                            corner = max(corner, hull)
                        else:
                            chord = max(chord, hull)
    _table[(mp, R)] = (alone, corner, chord)
    print(f"| {mp} | {R} | {cap} | {alone} ({alone / cap:.3f}) | {corner} ({corner / cap:.3f}) | {chord} ({chord / cap:.3f}) | {both} |")
    assert (both > 0) == (R > 1)                                               # at R = 1 no mark is used twice
    assert alone <= cap and corner <= cap and chord <= cap, (alone, corner, chord, cap)
