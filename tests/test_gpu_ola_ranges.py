"""The overlap-add kernels (pv_psola_*, pv_tsm_*, pv_epoch_*) on the GPU at the far ends of their position and sample ranges.  tests/test_gpu_psola.py and
tests/test_gpu_tsm.py keep every table within [0, ~7200) and every sample O(1); the contract allows centres, outputs and nin up to 2^30, displacements
|D| < 2^30, and any finite float32.  tests/test_ola_ranges_model.py asks the same of the models and of a float32 restatement on the CPU.

1. TRANSLATION.  A far table shifted by K (t += K, D += K, out_first = K) reads the same input: the kernel must give the bits of its K = 0 run, from the
   host form, the device form in one call and in pieces, and a one-tile staging handle, for K = 1, 1023, 2^20 + 17 and K_far = 2^30 - 1 - max(t, D, NOUT).
   The same for the psola kernel with the input moved to [K, K + n) of a longer buffer, K up to 2^24 + 1, and once at K_far in the device form.
2. DISPLACEMENT EXTREMES.  Accepted calls with D = +-(2^30 - 1): reads near 2^31 and near -2^30 give exact +0.0 on covered outputs; one whose last taps
   reach input samples 0 .. 31 gives the model's values; one call mixes tiles that read real input with tiles that read wholly outside it.
3. EXACT SCALING.  y(2^k x) == ldexp(y(x), k) bit for bit at k = -20, 20, 100 and k_top, the largest k at which nothing can overflow; the conditions are
   computed from the model and asserted (tests/ola_f32.py scaling_conditions).
4. SMALL MAGNITUDES.  Inputs scaled by 2^-125 (normal samples, subnormal products) and by 2^-140 (everything subnormal) against the model with the
   re-derived subnormal term, tol(subnormal="derived") of tests/psola_model.py: 2^-150 ((Z + G) / D + 2).  No sample is left out; uncovered outputs are
   exact +0.0; every form and partition gives the same bits.  A kernel that flushes subnormal numbers fails by a factor of hundreds
   (tests/test_ola_ranges_model.py shows it on the restatement).
5. EPOCH RECORDS.  The records are an exact function of the block-scaled integers round(x 2^(10 - e)): rows scaled by 2^k, k = +-20, +-100, and a row
   whose peak is FLT_MAX give the unscaled records.
Worst observed |err| / bound in the new regimes (one MI355X), input scaled by 2^-125 and by 2^-140: tsm small 0.79 and 0.61, tiny 0.18 and 0.50, slow 0.38
and 0.50; psola tiny 0.17 and 0.65, voice 0.59 and 0.67.  The table whose last taps reach x[0 .. 31] from 2^30 - 1 samples away: 0.02."""
import numpy as np
import pytest

import epoch_model as EM
import f0_model as FM
import psola_model as PM
import test_gpu_epoch as TGE
import test_gpu_psola as TGP
import test_gpu_tsm as TGT
import test_ola_ranges_model as ORM
import tsm_model as TM

pytestmark = pytest.mark.gpu

TILE = TGT.TILE
NOUT = TGT.NOUT
NCH = TGT.NCH
TOP = (1 << 30) - 1
PSOLA_KS = ORM.KS + ((1 << 24) + 1,)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _tables():
    import phaze_amd
    return phaze_amd.vari_prototype(), phaze_amd.psola_window()


def _rows_on_device(x, before=0, pad=7):
    """Device rows [nch, before + n + pad], four bytes off their alignment: zeros in the first `before` samples, x, NaN in the padding.  Returns (the
    tensor that owns them, the pointer of row 0, nin, stride)."""
    import torch
    nch, n = x.shape
    nin = before + n
    d = torch.full((nch * (nin + pad) + 1,), float("nan"), dtype=torch.float32, device="cuda")
    rows = d[1:].view(nch, nin + pad)
    if before:
        rows[:, :before] = 0.0
    rows[:, before:nin] = torch.from_numpy(np.array(x, np.float32)).cuda()
    torch.cuda.synchronize()
    assert (d.data_ptr() + 4) % 16 == 4
    return d, d.data_ptr() + 4, nin, nin + pad


def _device(h, rows, nch, g, K, cuts=(0, NOUT)):
    """The device form of either handle: outputs [K + a, K + b) per pair of `cuts` into rows of padded stride four bytes off their alignment; checks that
    nothing around the rows was written."""
    import torch
    _, ptr, nin, stride = rows
    d_out = torch.full((nch * (NOUT + 5) + 1,), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for a, b in zip(cuts[:-1], cuts[1:]):
        h.process_device(ptr, nin, stride, nch, g, d_out.data_ptr() + 4 + 4 * a, K + a, b - a, NOUT + 5)
    h.synchronize()
    got = d_out.cpu().numpy()
    assert got[0] == -77.0 and np.all(got[1:].reshape(nch, NOUT + 5)[:, NOUT:] == -77.0)
    return got[1:].reshape(nch, NOUT + 5)[:, :NOUT].copy()


# ---- 1. translation -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", TGT.CASES)
def test_a_far_table_shifted_towards_2_to_the_30_changes_no_bit(name):
    import phaze_amd
    k = TGT.case(name)
    x, g, mp, R = k["x"], k["g"], k["mp"], k["R"]
    h = phaze_amd.Tsm(mp, R, max_channels=NCH, max_outputs=NOUT)
    small = phaze_amd.Tsm(mp, R, max_channels=NCH, max_outputs=1)
    rc, want, clean = TGT._raw(h, x, g, 0, NOUT, 5, 129, lead=1)
    assert rc == 0 and clean, h._L.pv_tsm_last_error(h._h)
    assert np.all(np.abs(want.astype(np.float64) - k["y"]) <= k["tol"])                       # the K = 0 run is within the model's bound, as today
    zeros = (slice(None), np.r_[0:900, NOUT - 900:NOUT]) if name == "sweep" else None        # those outputs read outside the input
    if zeros:
        assert not _bits(want[zeros]).any() and want.any()
    rows = _rows_on_device(x)
    assert _same(_device(h, rows, NCH, g, 0), want)
    cuts = TGT._fitting(np.random.default_rng(5 + len(name)), k)
    far = ORM.k_far(g)
    for K in ORM.KS + (far,):
        s = ORM.shifted(g, K)
        assert TM.check_grains(s, mp) is None and TM.check_span(s, mp, R, K, NOUT) is None
        rc, y, clean = TGT._raw(h, x, s, K, NOUT, 5, 129, lead=1)
        assert rc == 0 and clean, (K, h._L.pv_tsm_last_error(h._h))
        assert _same(y, want), (K, "host", int(np.sum(_bits(y) != _bits(want))))
        y = _device(h, rows, NCH, s, K)
        assert _same(y, want), (K, "device", int(np.sum(_bits(y) != _bits(want))))
        y = _device(h, rows, NCH, s, K, cuts)
        assert _same(y, want), (K, "device in pieces", int(np.sum(_bits(y) != _bits(want))))
        rc, y, clean = TGT._raw(small, x, s, K, NOUT, 3, 2, lead=1)
        assert rc == 0 and clean and _same(y, want), (K, "one tile per piece", int(np.sum(_bits(y) != _bits(want))))
        if zeros:
            assert not _bits(y[zeros]).any()                                                   # the exact zeros survive the shift
    del rows
    h.close()
    small.close()


@pytest.mark.parametrize("name", TGP.CASES)
def test_a_psola_table_moved_with_its_input_changes_no_bit(name):
    """The input at [K, K + n) of a longer buffer that is zero before it (and NaN in the padding beyond nin), the centres moved by K, outputs from K on."""
    import phaze_amd
    k = TGP.case(name)
    x, g, mp = k["x"], k["g"], k["mp"]
    n = x.shape[1]
    ps = phaze_amd.Psola(mp, max_channels=NCH, max_outputs=1024)
    rc, want, clean = TGP._raw(ps, x, g, 0, NOUT, 5, 3, lead=1)
    assert rc == 0 and clean and np.all(np.abs(want.astype(np.float64) - k["y"]) <= k["tol"])
    cuts = TGP._partition(np.random.default_rng(5 + len(name)), NOUT)
    for K in PSOLA_KS:
        s = ORM.psola_shifted(g, K)
        assert PM.check_grains(s, mp) is None
        xk = np.zeros((NCH, K + n), np.float32)
        xk[:, K:] = x
        rc, y, clean = TGP._raw(ps, xk, s, K, NOUT, 5, 3, lead=1)
        del xk
        assert rc == 0 and clean, (K, ps._L.pv_psola_last_error(ps._h))
        assert _same(y, want), (K, "host", int(np.sum(_bits(y) != _bits(want))))
        rows = _rows_on_device(x, before=K)
        y = _device(ps, rows, NCH, s, K)
        assert _same(y, want), (K, "device", int(np.sum(_bits(y) != _bits(want))))
        y = _device(ps, rows, NCH, s, K, cuts)
        assert _same(y, want), (K, "device in pieces", int(np.sum(_bits(y) != _bits(want))))
        del rows
    ps.close()


def test_the_psola_table_huge_at_the_last_positions_below_2_to_the_30():
    """One channel of `huge` in the device form at K_far = 2^30 - 1 - (NOUT + 4000): the last centre is 2^30 - 1 and nin = 2^30 - 4001.  The input is the end
    of an uninitialised buffer of K_far + n floats: the last n hold the samples, and the 2 max_period + 64 before them, which the grains of this table
    reach and which the K = 0 run reads as zeros outside the input, are zeroed; nothing else is written, so allocation is the whole cost."""
    import phaze_amd
    import torch
    k = TGP.case("huge")
    x, g, mp = k["x"][:1], k["g"], k["mp"]
    n = x.shape[1]
    K = TOP - (NOUT + 4000)
    s = ORM.psola_shifted(g, K)
    assert PM.check_grains(s, mp) is None and int(s[:, 0].max()) == TOP and K + n < 1 << 30
    ps = phaze_amd.Psola(mp, max_channels=1, max_outputs=NOUT)
    want = ps.process(x, g, 0, NOUT)
    assert np.all(np.abs(want.astype(np.float64) - k["y"][:1]) <= k["tol"][:1]) and want.any()
    reach = 2 * mp + 64
    d = torch.empty(K + n, dtype=torch.float32, device="cuda")
    d[K - reach:K] = 0.0
    d[K:] = torch.from_numpy(x[0].copy()).cuda()
    d_out = torch.full((NOUT + 2,), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    try:
        ps.process_device(d.data_ptr(), K + n, K + n, 1, s, d_out.data_ptr(), K, NOUT, NOUT)
        ps.synchronize()
        got = d_out.cpu().numpy()
    finally:
        del d
        torch.cuda.empty_cache()
        ps.close()
    assert np.all(got[NOUT:] == -77.0) and _same(got[None, :NOUT], want), int(np.sum(_bits(got[None, :NOUT]) != _bits(want)))


# ---- 2. displacement extremes -------------------------------------------------------------------------------------------------------------------

def _extreme(kind):
    """(far grains, out_first, nin) of a table with max_period 64 at max_rate 1 whose every grain has |D| = 2^30 - 1."""
    rng = np.random.default_rng(90 + len(kind))
    if kind == "up":                   # t near 2^30, D = -(2^30 - 1): reads near 2^31
        first = (1 << 30) - NOUT - 50
        g = TGT._far_table(rng, first + np.arange(0, NOUT + 40, 31), 40, 0.0, 0)
        g[:, 2] = -TOP
    elif kind == "down":               # outputs from 0 on, D = 2^30 - 1: reads near -2^30
        first = 0
        g = TGT._far_table(rng, np.arange(0, NOUT + 40, 31), 40, 0.0, 0)
        g[:, 2] = TOP
    elif kind == "touch":              # t near 2^30, D = 2^30 - 1, the last output is 2^30 - 1: it reads x[0], and the taps of the last outputs reach x[0 .. 31]
        first = (1 << 30) - NOUT
        g = TGT._far_table(rng, first + np.arange(0, NOUT - 40, 31), 40, 0.0, 0)
        g = np.concatenate([g, [[TOP - 20, 9 + 256 * 77, 0, 40], [TOP - 3, 200 + 256 * 255, 0, 40], [TOP, 0, 0, 40]]])
        g[:, 2] = TOP
    else:
        raise KeyError(kind)
    g = np.ascontiguousarray(g, np.int32).reshape(-1, 4)
    assert TM.check_grains(g, 64) is None and TM.check_span(g, 64, 1, first, NOUT) is None
    return g, first, 5000


@pytest.mark.parametrize("kind", ["up", "down", "touch"])
def test_displacements_of_2_to_the_30_less_one_are_accepted_and_read_what_the_model_reads(kind):
    import phaze_amd
    g, first, nin = _extreme(kind)
    x = TGT._signals(nin, 31)
    y, tol, poisoned, G, _ = TM.process(x, g, first, NOUT, *_tables(), bound=True, subnormal="derived")
    assert np.all(G > 0) and not poisoned.any()
    n = first + np.arange(NOUT)
    if kind == "up":
        assert int(n.max()) + TOP + 32 > (1 << 31) - 200 and not y.any()
    elif kind == "down":
        assert int(n.min()) - TOP - 32 < -(1 << 30) and not y.any()
    else:
        assert not y[:, :NOUT - 33].any() and np.count_nonzero(y[:, NOUT - 32:]) > 60
    rows = _rows_on_device(x)
    for mo in (NOUT, 1):
        h = phaze_amd.Tsm(64, 1, max_channels=NCH, max_outputs=mo)
        rc, host, clean = TGT._raw(h, x, g, first, NOUT, 5, 129, lead=1)
        assert rc == 0 and clean, h._L.pv_tsm_last_error(h._h)
        dev = _device(h, rows, NCH, g, first)
        h.close()
        assert _same(dev, host)
        if kind == "touch":
            err = np.abs(host.astype(np.float64) - y)
            print(f"{kind}: worst |err| / bound = {float(np.max(err / tol)):.3f}")
            assert np.all(err <= tol) and host[:, NOUT - 32:].any() and not _bits(host[:, :NOUT - 33]).any()
        else:
            assert not _bits(host).any()                                                      # every output covered, every one exact +0.0


def test_one_call_mixes_tiles_that_read_real_input_with_tiles_that_read_wholly_outside_it():
    """Four tiles, no grain reaching two of them: the first and the last read the input 5000 samples ahead, the second reads 2^30 - 1 samples before it,
    the third 2^30 - 1 samples past it.  The host form with a staging buffer of four tiles takes them in one piece, whose input range is the union of the
    two real ones; with one tile per piece two pieces stage nothing."""
    import phaze_amd
    rng = np.random.default_rng(91)
    t = np.arange(20, NOUT + 60, 41)
    t = t[((t % TILE > 61) & (t % TILE < TILE - 61)) | (t >= 3 * TILE + 61)]
    g = TGT._far_table(rng, t, 60, 0.0, 10)
    g[:, 2] -= 5000
    g[t // TILE == 1, 2] = TOP
    g[t // TILE == 2, 2] = -TOP
    g = np.ascontiguousarray(g, np.int32)
    assert TM.check_grains(g, 64) is None and TM.check_span(g, 64, 1, 0, NOUT) is None
    tiles = TM.tiles(g, 64, 0, NOUT)
    assert tiles[1, 2] < -(1 << 29) and tiles[2, 2] > 1 << 30 and 0 < tiles[0, 2] < tiles[3, 2] < 9000 and np.all(tiles[:, 3] > 0)
    x = TGT._signals(9000, 32)
    y, tol, _, G, _ = TM.process(x, g, 0, NOUT, *_tables(), bound=True, subnormal="derived")
    covered = G > 0
    assert all(covered[j * TILE + 100:(j + 1) * TILE - 100].all() for j in range(3)) and covered[3 * TILE + 10:].all() and not y[:, TILE:3 * TILE].any() and y[:, 100:TILE - 100].any() and y[:, 3 * TILE + 10:].any()
    rows = _rows_on_device(x)
    outs = []
    for mo in (4096, 1):
        h = phaze_amd.Tsm(64, 1, max_channels=NCH, max_outputs=mo)
        rc, host, clean = TGT._raw(h, x, g, 0, NOUT, 5, 129, lead=1)
        assert rc == 0 and clean, h._L.pv_tsm_last_error(h._h)
        outs += [host, _device(h, rows, NCH, g, 0), _device(h, rows, NCH, g, 0, [0, TILE, 3 * TILE, NOUT])]
        h.close()
    err = np.abs(outs[0].astype(np.float64) - y)
    assert np.all(err <= tol) and all(_same(o, outs[0]) for o in outs[1:])
    assert not _bits(outs[0][:, TILE:3 * TILE]).any() and outs[0][:, :TILE].any() and outs[0][:, 3 * TILE:].any()


# ---- 3. exact scaling ---------------------------------------------------------------------------------------------------------------------------

def _exactly_scaled(x, k):
    y = np.ldexp(x, k)
    assert y.dtype == np.float32 and np.array_equal(np.ldexp(y, -k), x)                        # nothing under- or overflows in the input
    return y


@pytest.mark.parametrize("kind,name", [("psola", n) for n in ORM.PSOLA_SCALED] + [("tsm", n) for n in ORM.TSM_SCALED])
def test_the_output_scales_exactly_with_a_power_of_two(kind, name):
    """The window weights and the tap weights do not depend on the signal, so every product, partial sum and quotient of 2^k x is 2^k times that of x as
    long as none leaves the normal range: checked on the model and the tables, not assumed (tests/ola_f32.py scaling_conditions)."""
    import phaze_amd
    c = ORM.scaling_conditions()
    k_top = c["k_top"]
    print({key: (f"{v:.4g}" if isinstance(v, float) else v) for key, v in c.items()})
    assert c["smallest"] * 2.0 ** -20 >= 2.0 ** -126 and c["largest"] * 2.0 ** k_top < 2.0 ** 128 and k_top >= 120
    if kind == "psola":
        k = TGP.case(name)
        h = phaze_amd.Psola(k["mp"], max_channels=NCH, max_outputs=NOUT)
    else:
        k = TGT.case(name)
        h = phaze_amd.Tsm(k["mp"], k["R"], max_channels=NCH, max_outputs=NOUT)
    x, g = k["x"], k["g"]
    base = h.process(x, g, 0, NOUT)
    assert np.all(np.abs(base.astype(np.float64) - k["y"]) <= k["tol"])
    for e in ORM.SCALE_KS + (k_top,):
        want = np.ldexp(base, e)
        assert np.all(np.isfinite(want)) and np.array_equal(np.ldexp(want, -e), base)          # the expectation itself is exact
        y = h.process(_exactly_scaled(x, e), g, 0, NOUT)
        assert _same(y, want), (e, int(np.sum(_bits(y) != _bits(want))))
    xs = _exactly_scaled(x, k_top)
    rc, y, clean = (TGP if kind == "psola" else TGT)._raw(h, xs, g, 0, NOUT, 5, 129, lead=1)
    assert rc == 0 and clean and _same(y, want)
    assert _same(_device(h, _rows_on_device(xs), NCH, g, 0, [0, 1025, NOUT]), want)
    h.close()


# ---- 4. small magnitudes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name", ORM.SMALL_CASES)
def test_subnormal_products_and_subnormal_inputs_stay_within_the_derived_bound(kind, name):
    import phaze_amd
    for e in ORM.SMALL_SCALES:
        mp, R, far, g, xs = ORM.small_case(kind, name, e)
        y, tol, poisoned, G, den = TM.process(xs, far, 0, NOUT, *_tables(), bound=True, subnormal="derived")
        covered = G > 0
        assert not poisoned.any() and covered.sum() > NOUT // 2
        strong = float(np.mean(np.abs(y[:, covered]) > 4.0 * tol[:, covered]))
        assert strong >= 1.0 / 3.0                                                             # the gate has power at either scale
        if kind == "psola":
            h, mod = phaze_amd.Psola(mp, max_channels=NCH, max_outputs=1024), TGP
            cuts = TGP._partition(np.random.default_rng(17), NOUT)
        else:
            h, mod = phaze_amd.Tsm(mp, R, max_channels=NCH, max_outputs=1024), TGT
            cuts = TGT._fitting(np.random.default_rng(17), dict(g=g, mp=mp, R=R))
        rc, got, clean = mod._raw(h, xs, g, 0, NOUT, 5, 129, lead=1)
        assert rc == 0 and clean
        err = np.abs(got.astype(np.float64) - y)
        worst = float(np.max(err[:, covered] / tol[:, covered]))
        print(f"{kind} {name} 2^{e}: worst |err| / bound = {worst:.3f}, max |err| = {err.max() * 2.0 ** 149:.2f} * 2^-149, |y| > 4 tol on {strong:.2f} of the covered outputs")
        assert np.all(err <= tol), (e, int(np.sum(err > tol)), worst)                          # no sample left out
        assert not _bits(got[:, ~covered]).any()                                               # no grain: exact +0.0
        parts = np.concatenate([h.process(xs, g, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
        assert _same(parts, got)
        rows = _rows_on_device(xs)
        assert _same(_device(h, rows, NCH, g, 0), got) and _same(_device(h, rows, NCH, g, 0, cuts), got)
        h.close()


# ---- 5. epoch records under scaling -------------------------------------------------------------------------------------------------------------

def test_epoch_records_do_not_move_with_a_power_of_two():
    """The voice of tests/test_gpu_epoch.py at its three phases.  The block scaling takes the exponent e of the frame's peak and rounds x 2^(10 - e): 2^k x has
    the same integers, up to a peak of FLT_MAX, the largest exponent there is.  The FLT_MAX rows are the voice at the amplitude 1 - 2^-24 times 2^128, so
    their unscaled rows exist, and the model is run on them as they are."""
    import phaze_amd
    window, hop, mp, F = 2048, 256, 1024, 6
    p = FM.period(PM.records_of([217.3])[0])
    p256 = int(EM.periods(PM.records_of([217.3]))[0])
    n = TGE._span(window, hop, F)
    periods = np.full(F, p256, np.int32)
    phases = (0, 3, 4)
    x = np.stack([PM.voice(p, n, phase=j / 8) for j in phases])
    want = TGE._want(x, window, hop, mp, periods)
    assert np.all(want[:, :, 1] >= 1) and np.all(want[:, :, 3] > EM.S_ONE // 2)
    ks = (-100, -20, 20, 100)
    one = np.nextafter(np.float32(1), np.float32(0))
    full = np.stack([PM.voice(p, n, phase=j / 8, amplitude=float(one)) for j in phases])
    top = np.ldexp(full, 128)
    assert top.dtype == np.float32 and np.all(np.isfinite(top)) and np.all(np.max(np.abs(top), axis=1) == np.finfo(np.float32).max)
    want_full = TGE._want(full, window, hop, mp, periods)
    want_top = TGE._want(top, window, hop, mp, periods)
    assert np.array_equal(want_top, want_full) and np.all(want_top[:, :, 1] >= 1)              # the model agrees on the FLT_MAX rows
    rows = np.concatenate([x] + [_exactly_scaled(x, e) for e in ks] + [full, top])
    expect = np.concatenate([want] * (1 + len(ks)) + [want_full, want_top])
    trk = phaze_amd.EpochTracker(window, hop, mp, max_channels=rows.shape[0], max_frames=F)
    host = TGE._host(trk, rows, periods)
    dev = TGE._device(trk, rows, periods)
    trk.close()
    for c in range(rows.shape[0]):
        assert np.array_equal(host[c], expect[c]) and np.array_equal(dev[c], expect[c]), (c, host[c].tolist(), expect[c].tolist())
