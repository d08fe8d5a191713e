"""CPU checks of mirrored grains on the overlap-add path as tests/mirror_model.py defines them (DESIGN.md "Mirrored grains"): a table without mirrored
grains is tests/tsm_model.py's in every respect; the planner with mirror=False is tsm_plan bit for bit, and with mirror=True differs from it in the read
side of the reuses of unvoiced marks only; a mirrored grain is the forward grain on the reversed input; every tile of a mirrored plan fits the span; and
the buzz of repeated noise grains, the reason for all this, falls to less than half.  The C planner and tile walk are compared with the model in
tests/test_mirror_abi.py, the kernel in tests/test_gpu_mirror.py."""
import numpy as np
import pytest

import epoch_model as EM
import mirror_model as MM
import psola_model as PM
import test_epoch_model as TEM
import test_gpu_tsm as TGT
import test_psola_model as TPM
import test_tsm_model as TTM
import tsm_model as TM

BIT = MM.MIRROR


def track(seed):
    """The 24 random tracks of tests/test_tsm_model.py with their rates, epoch records and planner arguments: (args, kwargs, max_period, R)."""
    recs, ratios, _ = TPM._random_track(seed)
    nrec = recs.shape[0]
    mp = (64, 256, 1024)[seed % 3]
    R = (2, 4)[(seed // 3) % 2]
    rng = np.random.default_rng(500 + seed)
    rates = TTM.random_rates(rng, nrec, R)
    ep = TEM.random_epochs(rng, nrec) if seed % 4 >= 2 else None
    n = nrec * 64 - (0, 37)[seed % 2]
    return (recs, 64, 32, n, float(min(96, mp)), 20, mp), dict(ratios=ratios, rates=rates, epochs=ep, lock=(EM.DEFAULT_LOCK, 1.0)[seed % 2]), mp, R


# ---- tables without mirrored grains ---------------------------------------------------------------------------------------------------------------

def test_a_table_without_mirrored_grains_is_tsm_models():
    """process (values, bound and poisoned outputs), tiles and check_grains, with ==, on the tables of tests/test_gpu_tsm.py."""
    rng = np.random.default_rng(4)
    for name in ("small", "mid", "tiny", "huge", "sweep", "gap", "empty", "slow"):
        mp, R, nin, g = TGT._grains(name)
        x = TGT._signals(nin, 3)[:2]
        x[1, nin // 2] = np.nan
        for first, count in ((0, TGT.NOUT), (1001, 1500)):
            want = TM.process(x, g, first, count, bound=True)
            got = MM.process(x, g, first, count, bound=True)
            for a, b in zip(got, want):
                assert np.array_equal(a, b, equal_nan=True), name
            assert np.array_equal(MM.process(x, g, first, count), want[0])
            assert np.array_equal(MM.tiles(g, mp, first, count), TM.tiles(g, mp, first, count))
            assert MM.check_span(g, mp, R, first, count) == TM.check_span(g, mp, R, first, count)
        assert MM.check_grains(g, mp) is None
        if g.shape[0] > 40:
            for _ in range(20):
                bad = np.array(g)
                bad[rng.integers(0, g.shape[0]), rng.integers(0, 4)] = rng.choice([-1, 1, 65535, 1 << 30, -(1 << 30), mp + 1, 5])
                assert MM.check_grains(bad, mp) == TM.check_grains(bad, mp)
    for bad, why in (([[5, 131072, 0, 9]], "centre"), ([[5, -1, 0, 9]], "centre"), ([[5, 0, 1 << 30, 9]], "shift"), ([[5, 0, -(1 << 30), 9]], "shift"),
                     ([[5, BIT, -(1 << 30), 9]], "shift"), ([[5, BIT + 7, 0, 65]], "half length"), ([[5, BIT + 256 * 255 + 7, 0, 9], [5, 6, 0, 9]], "out of order")):
        assert MM.check_grains(np.array(bad), 64)[1] == why
    assert MM.check_grains(np.array([[5, BIT + 7, (1 << 31) - 1, 64], [5, BIT + 65535, 1 - (1 << 30), 2], [5, 65535, (1 << 30) - 1, 2]]), 64) is None


def test_a_whole_sample_mirrored_table_is_the_forward_table_on_the_reversed_input():
    """x[D - n] is x[::-1][n - (D - (nin - 1))]: this ties the mirrored rule to the forward model, bit for bit, bound and poisoned outputs included.  And a
    fractional mirrored grain reads at D - n - phi / 256: on a ramp x[p] = p that is its value, so the taps and their weights sit where they should."""
    rng = np.random.default_rng(11)
    n = TGT.NOUT
    for name in ("small", "tiny", "sweep"):
        mp, R, nin, g = TGT._grains(name)
        x = TGT._signals(nin, 5)
        x[0, nin // 3] = np.inf
        m = np.array(g, np.int64)
        m[:, 1] = (m[:, 1] & 255) + BIT                                      # phi = 0, mirrored
        m[:, 2] = rng.integers(-200, nin + 200, m.shape[0]) + m[:, 0]        # reads fall inside the input and across both of its ends
        f = np.stack([m[:, 0], m[:, 1] - BIT, m[:, 2] - (nin - 1), m[:, 3]], axis=1)
        assert MM.check_grains(m, mp) is None and TM.check_grains(f, mp) is None
        got = MM.process(x, m, 0, n, bound=True)
        want = TM.process(x[:, ::-1], f, 0, n, bound=True)
        for a, b in zip(got, want):
            assert np.array_equal(a, b, equal_nan=True), name
        assert np.any(got[0] != 0.0)
    ramp = np.arange(4000, dtype=np.float32)
    for phi in (1, 77, 128, 255):
        for tf in (0, 200):
            y = MM.process(ramp, np.array([[500, tf + 256 * phi + BIT, 2500, 100]]), 0, 700)[0]
            k = np.arange(401, 600)
            assert np.all(np.abs(y[k] - (2500 - k - phi / 256.0)) < 2e-3), (phi, tf)               # the interpolator's error on a ramp
            assert np.all(y[:400] == 0.0) and np.all(y[601:] == 0.0)


# ---- the planner ------------------------------------------------------------------------------------------------------------------------------------

_worst = {}


@pytest.mark.parametrize("with_epochs", [False, True])
@pytest.mark.parametrize("seed", range(24))
def test_the_plan_differs_from_tsm_plan_in_the_read_side_of_reuses_only(seed, with_epochs):
    """On the 24 random tracks of tests/test_tsm_model.py, with and without epoch records: mirror=False is tsm_plan bit for bit; mirror=True keeps t, tf, L
    and output_len of every grain and every field of the forward ones; a mirrored grain sits on an unvoiced mark that the grain before it used too; no two
    consecutive grains on one unvoiced mark share a direction; a mirrored grain reads about its mark; and every tile, from output 0 and from 777, stays
    within span(max_period, R)."""
    args, kw, mp, R = track(seed)
    nrec = np.asarray(args[0]).reshape(-1, 4).shape[0]
    own = kw["epochs"] if kw["epochs"] is not None else TEM.random_epochs(np.random.default_rng(900 + seed), nrec)
    kw = dict(kw, epochs=own if with_epochs else None)
    want, want_len = TM.tsm_plan(*args, **kw)
    off, off_len = MM.mirror_plan(*args, mirror=False, **kw)
    assert off.dtype == np.int32 and np.array_equal(off, want) and off_len == want_len
    g, n, A, voiced = MM.mirror_plan(*args, mirror=True, details=True, **kw)
    assert g.dtype == np.int32 and g.shape == want.shape and n == want_len and MM.check_grains(g, mp) is None
    g, want = g.astype(np.int64), want.astype(np.int64)
    m = MM.mirrored(g)
    assert np.array_equal(g[~m], want[~m])
    assert np.array_equal(g[:, [0, 3]], want[:, [0, 3]]) and np.array_equal(g[:, 1] & 255, want[:, 1] & 255)
    assert not np.any(m & voiced) and not m[0]
    same = np.concatenate([[False], (A[1:] == A[:-1]) & ~voiced[1:]])       # a reuse: the walk did not advance, on an unvoiced mark
    assert np.all(same[m])
    assert np.all(m[1:][same[1:]] != m[:-1][same[1:]]) and not np.any(m & ~same)
    # input A - (tau - T) lands at output tau: 256 D - phi is 256 (T + A) rounded, and T itself is rounded to 1/256 in c
    sq = 256 * g[m, 2] - ((g[m, 1] >> 8) & 255)
    c = 256 * g[m, 0] + (g[m, 1] & 255)
    assert np.all(np.abs(sq - (c + 256.0 * A[m])) <= 1.0)
    # the forward grain of the same slot reads about the same mark: 256 (T - A)
    dq = 256 * want[m, 2] + (want[m, 1] >> 8)
    assert np.all(np.abs((c - dq) - 256.0 * A[m]) <= 1.0)
    cap = MM.span(mp, R)
    ext = np.concatenate([MM.tiles(g, mp, 0, n)[:, 3], MM.tiles(g, mp, 777, n - 777)[:, 3]])
    fwd = np.concatenate([TM.tiles(want, mp, 0, n)[:, 3], TM.tiles(want, mp, 777, n - 777)[:, 3]])
    key = (mp, R)
    _worst[key] = max(_worst.get(key, (0.0, 0.0)), (float(ext.max()) / cap, float(fwd.max()) / cap))
    print(f"seed {seed} max_period {mp} R {R}: {g.shape[0]} grains, {int(m.sum())} mirrored, worst tile {ext.max()} = {ext.max() / cap:.3f} of span {cap} "
          f"(forward plan {fwd.max() / cap:.3f}); worst so far at ({mp}, {R}): {_worst[key][0]:.3f} (forward {_worst[key][1]:.3f})")
    assert np.all(ext <= cap) and MM.check_span(g, mp, R, 0, n) is None


def test_mirrored_grains_exist_on_the_random_tracks_and_none_on_a_voiced_one():
    total = 0
    for seed in range(24):
        args, kw, mp, R = track(seed)
        total += int(MM.mirrored(MM.mirror_plan(*args, **kw)[0]).sum())
    assert total > 100, total                                                # 164: the tracks are mostly voiced
    recs = PM.records_of([217.3] * 100)
    for rate in (0.25, 0.5, 1.0, 3.0):
        a = MM.mirror_plan(recs, 64, 32, 6400, 128.0, 20, 512, rates=np.full(100, rate), ratios=np.full(100, 1.25))
        b = TM.tsm_plan(recs, 64, 32, 6400, 128.0, 20, 512, rates=np.full(100, rate), ratios=np.full(100, 1.25))
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    # without records every mark is empty: at half speed every second grain is mirrored, at rate 1 none
    g, n = MM.mirror_plan(np.zeros((0, 4), np.int32), 64, 32, 4000, 100.0, 20, 512)
    assert not MM.mirrored(g).any() and n == 4000


@pytest.mark.parametrize("mp,R", [(64, 1), (64, 2), (64, 3), (64, 4), (256, 2), (256, 4), (1024, 2), (1024, 4), (4096, 1)])
def test_the_span_at_the_highest_rate_and_the_longest_period_with_mirrored_grains(mp, R):
    """The corner cases of tests/test_tsm_model.py test_the_span_at_the_highest_rate_and_the_longest_period with mirror=True, and the same at the rate 1 / R,
    where the unvoiced track has its reuses."""
    rng = np.random.default_rng(mp + R)
    worst = mirrored = 0
    for period in (float(mp), mp / 2.0, -float(mp)):
        for ratio in (0.5, 1.0, 2.0):
            for rate in (float(R), 1.0 / R):
                nrec = int(8 * 1024 * rate + 8 * mp) // 64
                recs = PM.records_of([period] * nrec)
                ep = TEM.random_epochs(rng, nrec, 2 * min(mp, 2048))
                for epochs in (None, ep):
                    g, nout = MM.mirror_plan(recs, 64, 32, nrec * 64, float(mp), min(20, mp), mp, ratios=np.full(nrec, ratio), rates=np.full(nrec, rate), epochs=epochs,
                                             lock=1.0)
                    mirrored += int(MM.mirrored(g).sum())
                    for first in (0, 511):
                        worst = max(worst, int(MM.tiles(g, mp, first, nout - first)[:, 3].max()))
    print(f"max_period {mp} rate {R}: worst tile extent {worst} = {worst / MM.span(mp, R):.3f} of span {MM.span(mp, R)}, {mirrored} mirrored grains")
    assert worst <= MM.span(mp, R) and (mirrored > 0) == (R > 1)


def test_planner_arguments():
    recs = PM.records_of([100.0] * 8)
    base = dict(f0_hop=64, f0_center=32, input_len=512, unvoiced_period=100.0, min_period=20, max_period=512)
    for kw in (dict(rates=np.full(7, 1.0)), dict(rates=np.full(8, 0.0)), dict(rates=np.full(8, np.nan)), dict(lock=0.0), dict(min_strength=-1),
               dict(epochs=np.zeros((7, 4), np.int32)), dict(min_period=1), dict(ratios=np.full(8, 2.5)), dict(input_len=1 << 30)):
        with pytest.raises(ValueError):
            MM.mirror_plan(recs, **dict(base, **kw))
    g, n = MM.mirror_plan(recs, **dict(base, input_len=0))
    assert g.shape == (0, 4) and n == 0


# ---- the buzz ---------------------------------------------------------------------------------------------------------------------------------------

N_BUZZ, P_BUZZ = 24000, 128
_buzz = {}


def _buzz_case(rate):
    """White noise under an all-unvoiced track, unvoiced_period 128, max_period 256, 24000 inputs: per mirror setting (the largest normalised
    autocorrelation of output[2000 : len - 2000] over the lags 32 .. 1100, its lag, the figure at lag 128, grains, mirrored grains)."""
    if rate not in _buzz:
        x = (0.1 * np.random.default_rng(1).standard_normal(N_BUZZ)).astype(np.float32)
        nrec = N_BUZZ // 256 + 1
        recs = np.zeros((nrec, 4), np.int32)
        out = []
        for mirror in (False, True):
            g, nout = MM.mirror_plan(recs, 256, 0, N_BUZZ, float(P_BUZZ), 32, 256, rates=np.full(nrec, rate), mirror=mirror)
            y = MM.process(x, g, 0, nout)[0]
            top, lag, r = MM.buzz(y)
            out.append((top, lag, float(r[P_BUZZ - 32]), g.shape[0], int(MM.mirrored(g).sum())))
        _buzz[rate] = out
    return _buzz[rate]


@pytest.mark.parametrize("rate", [0.5, 1.0 / 3.0, 0.3])
def test_mirroring_halves_the_buzz_of_repeated_noise_grains(rate):
    """The gate is relative to the forward plan's figure of the same run: the mirrored figure is at most half of it.  Measured (forward -> mirrored):
    rate 1/2 0.570 -> 0.087, 1/3 0.468 -> 0.107, 0.3 0.460 -> 0.119, the forward peak at lag 128 each time; rate 1: 0.022 both (the noise floor)."""
    (f_top, f_lag, f_p, ng, _), (m_top, m_lag, m_p, ng2, nm) = _buzz_case(rate)
    print(f"rate {rate:.3f}: forward {f_top:.3f} at lag {f_lag}, mirrored {m_top:.3f} at lag {m_lag} (ratio {m_top / f_top:.2f}); lag {P_BUZZ}: {f_p:.3f} -> {m_p:.3f}; "
          f"{nm} of {ng} grains mirrored")
    assert ng == ng2 and nm > ng // 3 and f_lag == P_BUZZ
    assert m_top <= 0.5 * f_top, (m_top, f_top)


def test_at_three_uses_per_mark_the_figure_at_the_mark_spacing_is_held_to_the_same_gate():
    """Rate 1/4: every mark serves three grains, forward, mirrored, forward.  The component at the mark spacing goes (0.634 -> -0.003); the first and the
    third use are both forward, so one at twice the spacing stays (0.345 at lag 256): the documented limit."""
    (f_top, f_lag, f_p, ng, _), (m_top, m_lag, m_p, _, nm) = _buzz_case(0.25)
    print(f"rate 0.25: forward {f_top:.3f} at lag {f_lag}, mirrored {m_top:.3f} at lag {m_lag}; lag {P_BUZZ}: {f_p:.3f} -> {m_p:.3f}; {nm} of {ng} grains mirrored")
    assert f_lag == P_BUZZ and abs(3 * nm - ng) <= 3
    assert m_p <= 0.5 * f_p
    assert m_lag == 2 * P_BUZZ and m_top < f_top


def test_at_rate_one_nothing_is_mirrored_and_the_figure_is_the_noise_floor():
    (f_top, _, _, _, _), (m_top, _, _, _, nm) = _buzz_case(1.0)
    assert nm == 0 and m_top == f_top < 0.05
