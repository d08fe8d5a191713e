"""The definition of the pitch contour tracker, on the CPU: tests/contour_model.py against the signals that break the frame-by-frame tracker
(tests/f0_model.py), and the path against an exhaustive search.  Geometry: W = 512, hop 128, lags 32 .. 512, K = 8, default costs; a frame counts as gross
when it is voiced and more than 20 % off the true period.  The figures quoted are those of DESIGN.md "Pitch contour"."""
import itertools

import numpy as np
import pytest

import contour_model as CM
import f0_model as FM

G = CM.GEOMETRY
ML = G["max_lag"]
# twice the worst relative error of a voiced path period on the fading tones, measured on the model: 1.940e-3 at P = 217.3, depth 0.97
PERIOD_GATE = 2 * 1.940e-3


def _periods(records):
    return np.array([FM.period(r) for r in records])


def test_dips_of_a_curve_worked_out_by_hand():
    c = np.array([16384, 9000, 500, 500, 700, 300, 300, 200, 900, 100, 400], np.int64)       # lags 0 .. 10: a plateau counts at its first lag
    assert CM.dips(c, 2, 10, 5, 0).tolist() == [[9, 900, 100, 400], [7, 300, 200, 900], [5, 700, 300, 300], [2, 9000, 500, 500], [0, 0, 0, 0]]
    assert CM.dips(c, 2, 10, 2, 16384)[:, 0].tolist() == [2, 5]                                 # keys 500 + 3276, 300 + 8192, 200 + 11468, 100 + 14745
    assert CM.dips(c, 3, 9, 8, 0)[:, 0].tolist() == [7, 5, 0, 0, 0, 0, 0, 0]                     # lag 9 = max_lag is outside, lag 2 below min_lag
    assert np.all(CM.frame_candidates(np.zeros(1024, np.float32), 512, 32, 512, 8, 1024) == 0)
    x = np.array(CM.signal(CM.FADES[0])[:1024])
    x[77] = np.inf
    assert np.all(CM.frame_candidates(x, 512, 32, 512, 8, 1024) == 0)


@pytest.mark.parametrize("name", CM.FADES)
def test_the_fading_tone_breaks_the_f0_tracker_and_not_the_path(name):
    P = float(name.split()[1])
    old = FM.track(CM.signal(name), G["W"], G["hop"], G["min_lag"], ML)
    rec, states = CM.path(CM.table(name), ML)
    per = _periods(rec)
    worst = float(np.max(np.abs(per - P) / P))
    print(f"{name}: f0 tracker {CM.gross(old, P)} gross of {len(old)}; path {CM.gross(rec, P)} gross, {int(np.sum(rec[:, 0] <= 0))} unvoiced, worst relative {worst:.3e}")
    assert len(old) == len(rec) == 86 and CM.gross(old, P) >= 10                # measured: 16 at depth 0.9, 22 at depth 0.97
    assert CM.gross(rec, P) == 0 and np.all(rec[:, 0] > 0) and np.all(states < 8)
    assert worst <= PERIOD_GATE


@pytest.mark.parametrize("K", [8, 2])
@pytest.mark.parametrize("name", CM.NOISY)
def test_a_noisy_tone_has_no_gross_frame_at_bias_1024(name, K):
    P = float(name.split()[1])
    rec, _ = CM.path(CM.table(name, K), ML)
    assert CM.gross(rec, P) == 0, (name, K)
    if K == 8:
        assert np.all(rec[:, 0] > 0)


def test_heavy_noise_is_unvoiced_in_both_trackers():
    x = CM.fading_tone(100.37, 0.0, 0.45)
    old = FM.track(x, G["W"], G["hop"], G["min_lag"], ML)
    rec = CM.track(x, G["W"], G["hop"], G["min_lag"], ML)
    assert len(rec) == 86 and np.all(old[:, 0] < 0) and np.all(rec[:, 0] < 0)


def test_an_octave_leap_is_followed_within_the_frames_that_straddle_it():
    rec, _ = CM.path(CM.table("leap"), ML)
    m = np.arange(len(rec))
    span = G["W"] + ML
    straddle = (m * G["hop"] < 8000) & (m * G["hop"] + span > 8000)
    true = np.where(m * G["hop"] + span <= 8000, 200.0, 100.0)
    per = _periods(rec)
    bad = (per > 0) & (np.abs(per - true) > 0.2 * true) & ~straddle
    assert len(rec) == 118 and not np.any(bad), np.nonzero(bad)[0].tolist()
    assert np.all(per[~straddle] > 0)                                          # voiced on both sides


def test_tone_noise_tone_is_voiced_unvoiced_voiced():
    rec, _ = CM.path(CM.table("tnt"), ML)
    v = rec[:, 0] > 0
    m = np.arange(len(rec))
    assert CM.gross(rec, 100.37) == 0
    assert int(np.sum(v[1:] != v[:-1])) == 2                                   # at most one change of voicing at each edge, and both are there
    inside = (m * G["hop"] >= 6000) & (m * G["hop"] + G["W"] + ML <= 10000)
    outside = (m * G["hop"] + G["W"] + ML <= 6000) | (m * G["hop"] >= 10000)
    assert np.all(~v[inside]) and np.all(v[outside])


def test_the_path_is_a_minimum_over_every_state_sequence():
    rng = np.random.default_rng(7)
    costs = [CM.DEFAULTS, dict(bias=0, unvoiced_cost=100, voicing_cost=0, jump_cost=0), dict(bias=16384, unvoiced_cost=16384, voicing_cost=5000, jump_cost=1 << 20),
             dict(bias=1024, unvoiced_cost=1, voicing_cost=1 << 20, jump_cost=300)]
    seen_empty = seen_voiced = 0
    for trial in range(240):
        T, K = int(rng.integers(1, 7)), int(rng.integers(1, 4))
        t = CM.random_table(rng, T, K, max_lag=64, lead=int(rng.integers(0, 2)))
        kw = costs[trial % len(costs)]
        rec, states = CM.path(t, 64, **kw)
        mine = CM.path_cost(t, states, 64, **kw)
        assert mine is not None
        best = min(c for c in (CM.path_cost(t, s, 64, **kw) for s in itertools.product(range(K + 1), repeat=T)) if c is not None)
        assert mine == best, (trial, t.tolist(), states.tolist())
        for m in range(T):                                                     # the records say what the states say
            s = int(states[m])
            if s < K:
                assert rec[m].tolist() == t[m, s].tolist() and rec[m, 0] > 0
                seen_voiced += 1
            elif t[m, 0, 0] > 0:
                assert rec[m].tolist() == [-t[m, 0, 0]] + t[m, 0, 1:].tolist()
            else:
                assert np.all(rec[m] == 0)
                seen_empty += 1
    assert seen_empty > 50 and seen_voiced > 50
    assert CM.path(np.zeros((0, 3, 4), np.int32), 64)[0].shape == (0, 4)
