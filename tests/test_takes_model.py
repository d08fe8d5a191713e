"""CPU checks of the model of per-take plans (tests/takes_model.py): the class boundaries follow from the LDS formula, the launch order is a stable
permutation grouped by class, a take split at a multiple of the tile gives the union of its tiles, and the fixture call that tests/test_takes_abi.py and
tests/test_gpu_takes.py share has tiles in all four classes."""
import numpy as np

import takes_model as KM
import test_gpu_tsm as TGT
import tsm_model as TM

TILE = KM.TILE
NOUT = TGT.NOUT
RAGGED_NOUTS = [3 * TILE + 37, 1, 1023, 1024, 1025, 0]


def class_fixture():
    """A call on a (4096, 1) configuration whose tiles fall into all four classes: (max_period, max_rate, input lengths, tables, out_firsts, nouts).
    `big` of tests/test_gpu_tsm.py (displacements spread over 16000 samples), a far table with a displacement jitter of 2500, `tiny` (a tile reads
    little more than it writes) and a take of 500 outputs under short grains."""
    _, _, nin_big, big = TGT._grains("big")
    _, _, nin_tiny, tiny = TGT._grains("tiny")
    rng = np.random.default_rng(91)
    t = np.arange(0, NOUT + 300, 23)
    mid = TGT._far_table(rng, t, rng.integers(2, 200, t.size), 0.0, 2500)
    mid[:, 2] -= 2600
    t = np.arange(5, 520, 13)
    short = TGT._far_table(rng, t, rng.integers(2, 30, t.size), 0.0, 3)
    short[:, 2] -= 40
    tables = [np.ascontiguousarray(g, np.int32).reshape(-1, 4) for g in (big, mid, tiny, short)]
    nins = [nin_big, NOUT + 5300, nin_tiny, 600]
    nouts = [NOUT, NOUT, NOUT, 500]
    firsts = [0, 0, 0, 0]
    for g in tables:
        assert TM.check_grains(g, 4096) is None
    assert KM.check_span(tables, 4096, 1, firsts, nouts) is None
    return 4096, 1, nins, tables, firsts, nouts


def test_class_boundaries_follow_from_the_lds_formula():
    """lds_bytes(s) is tsm_model.lds_bytes with the span given; the largest staged count of each class is where 163840 div lds_bytes(s) steps down."""
    for mp, R in ((64, 4), (1024, 4), (4096, 1), (512, 2)):
        assert KM.lds_bytes(TM.span(mp, R)) == TM.lds_bytes(mp, R)
    tables_only = KM.lds_bytes(0) - 4 * 4
    assert 36800 <= tables_only <= 37000 and TM.LDS_BYTES // KM.lds_bytes(128) == 4          # P and Hn take 36.9 KB: four workgroups are the ceiling
    for last, c in ((960, 4), (4352, 3), (11072, 2)):
        assert last % 64 == 0 and KM.cls(last) == c and KM.cls(last + 1) == c - 1, (last, KM.cls(last), KM.cls(last + 1))
        assert TM.LDS_BYTES // KM.lds_bytes(last) == c and TM.LDS_BYTES // KM.lds_bytes(last + 64) == c - 1
        assert KM.cls(last - 63) == c
    assert KM.cls(0) == KM.cls(1) == KM.cls(128) == 4 and KM.cls(TM.span(4096, 1)) == 1 and KM.cls(TM.span(2048, 4)) == 1
    assert KM.launch_span(0) == 128 and KM.launch_span(129) == 192 and KM.launch_span(960) == 960 and KM.launch_span(961) == 1024
    for s in range(0, 26000, 37):
        assert 1 <= KM.cls(s) <= 4 and KM.cls(s) >= KM.cls(s + 37)


def largest_spans():
    """The accepted (max_period, max_rate) pairs with the largest spans, per max_rate, and the largest count that fits the LDS at all."""
    top = max(s for s in range(31000, 31400) if KM.lds_bytes(s) <= TM.LDS_BYTES)
    pairs = []
    for R in (1, 2, 3, 4):
        fitting = [mp for mp in range(2, TM.MAX_PERIOD + 1) if KM.lds_bytes(TM.span(mp, R)) <= TM.LDS_BYTES]       # (== TM.lds_bytes(mp, R), asserted below)
        pairs.append((max(fitting), R))
    return top, pairs


def test_every_count_a_configuration_accepts_has_a_class_and_a_launch_that_fits():
    """A configuration's span need not be a multiple of 64.  Counts within 63 samples of the largest count that fits the LDS would, rounded up to 64, not fit:
    the quotient of the class formula is 0 there.  Such a launch stages the count itself and the class is 1; everywhere else the formula stands."""
    top, pairs = largest_spans()
    assert KM.lds_bytes(top) <= TM.LDS_BYTES < KM.lds_bytes(top + 1)
    assert pairs == [(4096, 1), (3641, 2), (2811, 3), (2257, 4)] and all(TM.lds_bytes(mp, R) == KM.lds_bytes(TM.span(mp, R)) <= TM.LDS_BYTES for mp, R in pairs)
    assert all(TM.lds_bytes(mp + 1, R) > TM.LDS_BYTES for mp, R in pairs[1:])
    assert [TM.span(mp, R) for mp, R in pairs] == [25664, 31240, 31246, 31244] and top == 31247
    hole = 0
    for s in range(0, top + 1):
        rounded = max(128, (s + 63) & ~63)
        quotient = TM.LDS_BYTES // KM.lds_bytes(rounded)
        span, c = KM.launch_span(s), KM.cls(s)
        assert 1 <= c <= 4 and span >= max(s, 128) and KM.lds_bytes(span) <= TM.LDS_BYTES and TM.LDS_BYTES // KM.lds_bytes(span) >= c
        if quotient >= 1:
            assert span == rounded and c == min(4, quotient)                 # the formula
        else:
            assert span == s and c == 1 and s > top - 63
            hole += 1
    assert hole == top - (top & ~63)                                          # the counts past the last multiple of 64 that fits
    for mp, R in pairs:                                                       # every accepted span has a class
        assert KM.cls(TM.span(mp, R)) == 1 and KM.launch_span(TM.span(mp, R)) in (TM.span(mp, R), (TM.span(mp, R) + 63) & ~63)


def widest_tile_table(max_period, max_rate, slack=4):
    """Two short grains in one tile whose source ranges lie as far apart as the span of the pair allows (slack samples less): the widest tile the
    configuration accepts, beside the largest span that fits the LDS at all."""
    cap = TM.span(max_period, max_rate) - slack
    # grain {100, L 2} reads from 98 - 33; grain {900, L 2, D} reads up to 902 - D + 32: extent 902 - D + 32 - 65
    D = 902 + 32 - 65 - cap
    return np.array([[100, 0, 0, 2], [900, 0, D, 2]], np.int32), cap


def test_the_widest_tiles_of_the_largest_configurations_are_of_class_one():
    top, pairs = largest_spans()
    for mp, R in pairs:
        for slack in (0, 4, 70):
            g, cap = widest_tile_table(mp, R, slack)
            assert TM.check_grains(g, mp) is None and TM.check_span(g, mp, R, 0, 1024) is None
            t = KM.tiles([g], mp, [0], [1024])
            assert t.tolist() == [[0, 0, 0, 2, 65, cap, 1, 0]]
        g, cap = widest_tile_table(mp, R, -1)
        assert TM.check_span(g, mp, R, 0, 1024) == (0, 0, cap)


def test_the_fixture_call_has_tiles_in_every_class():
    mp, R, nins, tables, firsts, nouts = class_fixture()
    t = KM.tiles(tables, mp, firsts, nouts)
    assert t.shape == (4 + 4 + 4 + 1, 8)
    per_take = [t[t[:, 0] == k] for k in range(4)]
    print([p[:, 5].tolist() for p in per_take])
    # the classes are what the extents give, not what the tables were meant to give: big's two narrower tiles read less than 11072 samples and are of
    # class 2, the last tile of the jittered table (37 outputs) of class 3, and tiny's last tiles (37 outputs; no grain) of class 4
    assert per_take[0][:, 6].tolist() == [2, 2, 1, 1] and np.all(per_take[0][2:, 5] > 11072) and np.all(per_take[0][:2, 5] > 4352)
    assert per_take[1][:, 6].tolist() == [2, 2, 2, 3] and np.all((per_take[1][:3, 5] > 4352) & (per_take[1][:3, 5] <= 11072))
    assert per_take[2][:, 6].tolist() == [3, 3, 4, 4] and np.all((per_take[2][:2, 5] > 1024) & (per_take[2][:2, 5] <= 4352)) and per_take[2][3, 5] == 0
    assert per_take[3][:, 6].tolist() == [4] and 500 < per_take[3][0, 5] <= 960
    assert set(t[:, 6].tolist()) == {1, 2, 3, 4}
    assert np.array_equal(t[:, 6], [KM.cls(int(c)) for c in t[:, 5]]) and np.all(t[:, 7] == 0)
    assert np.array_equal(t[:, 1], np.concatenate([np.arange(len(p)) * TILE for p in per_take]))


def test_order_is_a_stable_permutation_grouped_by_class():
    mp, R, nins, tables, firsts, nouts = class_fixture()
    rng = np.random.default_rng(3)
    perm = [2, 0, 3, 1, 0, 2]                                                # takes repeated and out of class order
    t = KM.tiles([tables[k] for k in perm], mp, [firsts[k] for k in perm], [nouts[k] for k in perm])
    o = KM.order(t)
    assert sorted(o.tolist()) == list(range(t.shape[0]))
    c = t[o, 6]
    assert np.all(np.diff(c) >= 0)                                            # grouped, ascending
    for k in range(1, 5):
        assert np.all(np.diff(o[c == k]) > 0)                                 # (take, tile) order kept within a class
    assert not np.array_equal(o, np.arange(t.shape[0]))
    for _ in range(20):                                                       # random classes
        fake = np.zeros((int(rng.integers(0, 40)), 8), np.int64)
        fake[:, 6] = rng.integers(1, 5, fake.shape[0])
        o = KM.order(fake)
        assert sorted(o.tolist()) == list(range(fake.shape[0])) and np.all(np.diff(fake[o, 6]) >= 0)
        assert all(np.all(np.diff(o[fake[o, 6] == k]) > 0) for k in range(1, 5))


def test_a_take_split_at_a_multiple_of_the_tile_gives_the_union_of_its_tiles():
    """Tiles count from the take's own out_first: cut at 1024 j, the two halves have the take's tiles (first counted from the half's own beginning).  Cut
    elsewhere the tiles differ, and only the outputs agree."""
    for name in ("small", "gap", "slow", "tiny"):
        mp, R, nin, g = TGT._grains(name)
        whole = KM.tiles([g], mp, [0], [NOUT])
        for cut in (TILE, 2 * TILE, 3 * TILE):
            two = KM.tiles([g, g], mp, [0, cut], [cut, NOUT - cut])
            assert two.shape == whole.shape
            assert np.array_equal(two[:, 2:], whole[:, 2:])
            assert np.array_equal(two[:, 0], (np.arange(whole.shape[0]) >= cut // TILE).astype(np.int64))
            assert np.array_equal(two[:, 1], np.where(two[:, 0] == 0, whole[:, 1], whole[:, 1] - cut))
        two = KM.tiles([g, g], mp, [0, 700], [700, NOUT - 700])
        assert two.shape[0] == 1 + 3 and not np.array_equal(two[1:, 4:6], whole[1:, 4:6])
    x = TGT._signals(TGT._grains("small")[2], 3)[:1]
    g = TGT._grains("small")[3]
    whole = TM.process(x, g, 0, NOUT)
    for cut in (700, 2048):
        a, b = KM.process([x, x], [g, g], [0, cut], [cut, NOUT - cut])
        assert np.array_equal(np.concatenate([a, b], axis=1), whole)


def test_ragged_calls_have_one_record_per_tile_of_each_take():
    mp, R, nin, g = TGT._grains("small")
    for first in (0, 517, (1 << 20) + 17):
        t = KM.tiles([g] * 6, mp, [first] * 6, RAGGED_NOUTS)
        assert t[:, 0].tolist() == [0] * 4 + [1, 2, 3, 4, 4] and t[:, 1].tolist() == [0, 1024, 2048, 3072, 0, 0, 0, 0, 1024]
        for k, n in enumerate(RAGGED_NOUTS):
            assert np.array_equal(t[t[:, 0] == k][:, 2:6], TM.tiles(g, mp, first, n))
