"""The mirrored-grain kernel (Mirror / pv_mirror_*) on the GPU against the numpy model (tests/mirror_model.py), bit equality with Tsm.process on tables without
mirrored grains and on the reversed input, and partition invariance.

Tolerance against the model: the DERIVED bound of tests/test_gpu_psola.py's docstring, unchanged (tests/test_gpu_tsm.py restates it).  The kernel's
arithmetic per (output, grain, tap) is pv_tsm_kernel's operation for operation; the direction of a grain, like its displacement, enters the addresses
only, never a rounded value, so mirror_model.process(bound=True) returns that bound for the same arithmetic.  No sample is left out; an output no grain
covers must be exactly 0.  Everything else is bit for bit.
Worst observed |err| / bound over all cases: 0.24 (the planned table of tone then noise at half speed, two channels); over the mixed tables 0.15 (`tiny`
and `small`, three channels).  One MI355X."""
import ctypes as C
import json
import shutil
import subprocess

import numpy as np
import pytest

import f0_model as FM
import mirror_model as MM
import psola_model as PM
import test_gpu_tsm as TGT
import tsm_model as TM

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int32)
TILE = TGT.TILE
NOUT = TGT.NOUT
NCH = TGT.NCH
BIT = MM.MIRROR
MIXED = ["small", "mid", "big", "tiny", "sweep", "gap"]


def _mixed(name):
    """(max_period, max_rate, nin, grains): the far table `name` of tests/test_gpu_tsm.py with every third grain mirrored about the position its centre
    reads, D = 2 t - D_forward plus a little: the mirrored grain reads the stretch the forward one read, downwards, so the tile's extent stays within the
    span; "sweep" reads across both ends of the input (exact zeros), "mid" and "big" thousands of samples from where they write.  phi keeps the table's
    values: 0, 1, 255 and random ones."""
    mp, R, nin, g = TGT._grains(name)
    rng = np.random.default_rng(1000 + len(name))
    m = np.array(g, np.int64)
    k = np.arange(1, m.shape[0], 3)
    m[k, 1] += BIT
    m[k, 2] = 2 * m[k, 0] - m[k, 2] + rng.integers(-3, 4, k.size)
    m = np.ascontiguousarray(m, np.int32)
    assert MM.check_grains(m, mp) is None and MM.check_span(m, mp, R, 0, NOUT) is None, (MM.check_grains(m, mp), MM.check_span(m, mp, R, 0, NOUT), MM.span(mp, R))
    phi = (m[k, 1] >> 8) & 255
    assert k.size < 20 or ({0, 1, 255} <= set(phi.tolist()) and len(set(phi.tolist())) > 6)      # (the tables of long grains have a dozen grains in all)
    return mp, R, nin, m


_CACHE = {}


def case(name):
    """Shared per mixed table, computed once and never written: the input, the grains, the model's output on the library's tables and its bound."""
    if name not in _CACHE:
        import phaze_amd
        mp, R, nin, g = _mixed(name)
        x = TGT._signals(nin, 7 + len(name))
        y, tol, poisoned = MM.process(x, g, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
        assert not poisoned.any()
        for a in (x, g, y, tol):
            a.setflags(write=False)
        _CACHE[name] = dict(mp=mp, R=R, n=nin, g=g, x=x, y=y, tol=tol)
    return _CACHE[name]


def _raw(h, x, g, out_first, nout, pad_in=0, pad_out=0, lead=0, fn="pv_mirror_process"):
    return TGT._raw(h, x, g, out_first, nout, pad_in, pad_out, lead, fn)


@pytest.mark.parametrize("name", TGT.CASES)
def test_forward_tables_give_the_bits_of_tsm_process(name):
    """The far tables of tests/test_gpu_tsm.py have no mirrored grain: Tsm.process's output with ==, from the host form, a range in the middle and the device
    form."""
    import phaze_amd
    k = TGT.case(name)
    x, g, mp, R = k["x"], k["g"], k["mp"], k["R"]
    ts = phaze_amd.Tsm(mp, R, max_channels=NCH, max_outputs=NOUT)
    want = ts.process(x, g, 0, NOUT)
    ts.close()
    h = phaze_amd.Mirror(mp, R, max_channels=NCH, max_outputs=NOUT)
    got = h.process(x, g, 0, NOUT)
    assert got.dtype == np.float32 and np.array_equal(got, want), (name, int(np.sum(got != want)))
    assert np.array_equal(h.process(x, g, 1001, 1500), want[:, 1001:2501])
    assert np.array_equal(TGT._device(h, x, g, [0, 1500, NOUT]), want)
    h.close()


@pytest.mark.parametrize("name", MIXED)
def test_every_sample_of_a_mixed_table_is_within_the_derived_bound_of_the_model(name):
    import phaze_amd
    k = case(name)
    covered = k["tol"][0] > 0
    mir = MM.mirrored(k["g"])
    assert mir.sum() >= k["g"].shape[0] // 3 - 1 and not mir.all()
    if name == "gap":
        assert not covered[975:2210].any() and not covered[TILE:2 * TILE].any()
    if name == "sweep":                # the first and the last outputs read outside the input in either direction: covered, and exactly zero in the model too
        assert covered[:900].all() and covered[-900:].all() and np.all(k["y"][:, :900] == 0.0) and np.all(k["y"][:, -900:] == 0.0) and np.any(k["y"][:, 1200:1900] != 0.0)
    if name == "tiny":
        assert np.all(MM.tiles(k["g"], k["mp"], 0, NOUT)[:3, 1] - MM.tiles(k["g"], k["mp"], 0, NOUT)[:3, 0] > 300)
    for nch, pads, lead in ((1, (0, 0), 0), (3, (5, 129), 1)):
        h = phaze_amd.Mirror(k["mp"], k["R"], max_channels=nch, max_outputs=NOUT)
        rc, y, clean = _raw(h, k["x"][:nch], k["g"], 0, NOUT, *pads, lead=lead)
        assert rc == 0 and clean, h._L.pv_mirror_last_error(h._h)
        err = np.abs(y.astype(np.float64) - k["y"][:nch])
        tol = k["tol"][:nch]
        live = covered[None, :] & (tol > 0)
        worst = float(np.max(err[live] / tol[live])) if live.any() else 0.0
        print(f"{name} nch {nch}: worst |err| / bound = {worst:.3f}, max |err| = {err.max():.3e}")
        assert np.all(err <= tol), (nch, int(np.sum(err > tol)), worst)
        assert np.all(y[:, ~covered] == 0.0) and not np.any(np.signbit(y[:, ~covered]))          # no grain: exact zeros
        if name == "sweep":
            assert np.all(y[:, :900] == 0.0) and np.all(y[:, -900:] == 0.0)                       # zeros read: exact zeros
        h.close()


@pytest.mark.parametrize("name", ["small", "tiny", "sweep", "big"])
def test_a_whole_sample_mirrored_table_gives_the_bits_of_tsm_process_on_the_reversed_input(name):
    """x[D - n] is x[::-1][n - (D - (nin - 1))]: every grain mirrored with phi = 0 on x against Tsm.process of {t, w - 65536, D - (nin - 1), L} on the reversed
    input, with ==."""
    import phaze_amd
    mp, R, nin, g = TGT._grains(name)
    x = TGT._signals(nin, 9 + len(name))
    f = np.array(g, np.int64)
    f[:, 1] &= 255                                                           # whole-sample displacements
    m = np.stack([f[:, 0], f[:, 1] + BIT, f[:, 2] + (nin - 1), f[:, 3]], axis=1)
    f, m = np.ascontiguousarray(f, np.int32), np.ascontiguousarray(m, np.int32)
    assert TM.check_grains(f, mp) is None and MM.check_grains(m, mp) is None and TM.check_span(f, mp, R, 0, NOUT) is None and MM.check_span(m, mp, R, 0, NOUT) is None
    ts = phaze_amd.Tsm(mp, R, max_channels=NCH, max_outputs=NOUT)
    want = ts.process(np.ascontiguousarray(x[:, ::-1]), f, 0, NOUT)
    ts.close()
    h = phaze_amd.Mirror(mp, R, max_channels=NCH, max_outputs=NOUT)
    got = h.process(x, m, 0, NOUT)
    h.close()
    assert np.any(want != 0.0) and np.array_equal(got, want), (name, int(np.sum(got != want)))


@pytest.mark.parametrize("name", MIXED)
def test_any_partition_and_every_form_give_the_same_bits(name):
    """One call, a repeated call, three calls split at odd outputs, a range in the middle, a channel alone, the host form in pieces of one tile, the device
    form in one call and in three on a user stream."""
    import phaze_amd
    import torch
    k = case(name)
    x, g, mp, R = k["x"], k["g"], k["mp"], k["R"]
    h = phaze_amd.Mirror(mp, R, max_channels=NCH, max_outputs=NOUT)
    rc, want, clean = _raw(h, x, g, 0, NOUT)
    assert rc == 0 and clean
    assert np.array_equal(h.process(x, g, 0, NOUT), want)                                    # the binding, and a repeated call
    cuts = [0, 1001, 2333, NOUT]                                                             # the tiles of a call start at its first output
    assert all(MM.check_span(g, mp, R, a, b - a) is None for a, b in zip(cuts[:-1], cuts[1:]))
    parts = [h.process(x, g, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts, axis=1), want)
    assert np.array_equal(h.process(x, g, 1001, 1500), want[:, 1001:2501])
    assert np.array_equal(h.process(x, g, 5, 0), np.zeros((NCH, 0), np.float32))
    for c in range(NCH):
        assert np.array_equal(h.process(x[c], g, 0, NOUT), want[c])
    assert np.array_equal(TGT._device(h, x, g, [0, NOUT]), want)
    h.close()
    small = phaze_amd.Mirror(mp, R, max_channels=NCH, max_outputs=1)
    rc, y, clean = _raw(small, x, g, 0, NOUT, 3, 2, lead=1)
    assert rc == 0 and clean and np.array_equal(y, want)
    small.close()
    h = phaze_amd.Mirror(mp, R, max_channels=NCH)
    assert np.array_equal(TGT._device(h, x, g, cuts, stream=torch.cuda.Stream()), want)
    h.close()


@pytest.mark.parametrize("mp,R", [(64, 1), (4096, 1), (1024, 4)])
def test_a_mirrored_grain_may_bring_a_tile_to_exactly_the_span_and_no_further(mp, R):
    """Tile 0 holds a forward grain that reads from position 3 on and a mirrored one whose range ends at D - 504: with D = span + 507 the tile's extent is
    exactly span(max_period, max_rate) and the call is accepted and within the bound; one sample more is refused with PV_ERR_ARGUMENT, the message names the
    tile's first grain and the extent, and the output keeps its fill."""
    import phaze_amd
    from phaze_amd import capi
    cap = MM.span(mp, R)
    nin = cap + 700
    x = TGT._signals(nin, 3)[:2]
    table = lambda D: np.array([[100, 7, 0, 64], [600, BIT + 256 * 77 + 200, D, 64]], np.int32)
    g = table(cap + 507)
    assert MM.check_grains(g, mp) is None and MM.tiles(g, mp, 0, TILE).tolist() == [[0, 2, 3, cap]]
    h = phaze_amd.Mirror(mp, R, max_channels=2, max_outputs=TILE)
    y, tol, _ = MM.process(x, g, 0, TILE, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
    for fn in ("pv_mirror_process", "pv_mirror_process_device"):
        wide = table(cap + 508)
        assert MM.check_grains(wide, mp) is None and MM.check_span(wide, mp, R, 0, TILE) == (0, 0, cap + 1)
        rc, out, clean = _raw(h, x, wide, 0, TILE, fn=fn)                   # host rows never reach the device: refused before any device work
        msg = h._L.pv_mirror_last_error(h._h).decode()
        assert rc == capi.PV_ERR_ARGUMENT and "grain 0:" in msg and "span" in msg and str(cap + 1) in msg and str(cap) in msg, msg
        assert clean and np.all(out == -77.0)
    rc, out, clean = _raw(h, x, g, 0, TILE)
    assert rc == 0 and clean and np.all(np.abs(out - y) <= tol) and np.any(out[:, 540:660] != 0.0)
    assert np.array_equal(_device_tile(h, x, g), out)
    h.close()


def _device_tile(h, x, g):
    """The device form on one tile of outputs."""
    import torch
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((x.shape[0], TILE), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    h.process_device(d_in.data_ptr(), x.shape[1], x.shape[1], x.shape[0], g, d_out.data_ptr(), 0, TILE, TILE)
    h.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_outputs_are_exactly_the_models(value):
    """A non-finite sample reaches exactly the outputs that have it under a tap of a grain with a non-zero weight, whichever way the grain reads: at the
    far end of a mirrored grain's reach, under its centre, and under a forward grain.  The finite outputs keep their bits in every form."""
    import phaze_amd
    for name in ("small", "tiny"):
        k = case(name)
        g, mp = k["g"], k["mp"]
        x = np.array(k["x"])
        n = x.shape[1]
        mir = np.flatnonzero(MM.mirrored(g))
        for j, c in ((mir[mir.size // 2], 0), (mir[mir.size // 3], 1), (mir[mir.size // 5], 2), (mir[1], 0), (mir[2] + 1, 1)):
            t, w, D, L = (int(v) for v in g[j])
            if w & BIT:
                x[c, min(max(D - (t - L + 1) + 31, 0), n - 1)] = value      # the highest tap of the grain's first output
                x[c, min(max(D - t, 0), n - 1)] = -value if value == value else value
            else:
                x[c, min(max(t - D, 0), n - 1)] = value
        y, tol, poisoned = MM.process(x, g, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
        h = phaze_amd.Mirror(mp, k["R"], max_channels=NCH, max_outputs=1024)
        got = h.process(x, g, 0, NOUT)
        assert np.array_equal(~np.isfinite(got), poisoned), (name, int(np.sum(~np.isfinite(got) != poisoned)))
        assert poisoned.any() and not poisoned.all()
        ok = ~poisoned
        assert np.all(np.abs(got[ok] - y[ok]) <= tol[ok])
        parts = np.concatenate([h.process(x, g, a, b - a) for a, b in ((0, 1001), (1001, 2333), (2333, NOUT))], axis=1)
        assert np.array_equal(np.isfinite(parts), ok) and np.array_equal(parts[ok], got[ok])
        dev = TGT._device(h, x, g, [0, NOUT])
        assert np.array_equal(np.isfinite(dev), ok) and np.array_equal(dev[ok], got[ok])
        h.close()


def test_refused_calls_leave_the_output_untouched_and_name_the_grain():
    import phaze_amd
    from phaze_amd import capi
    k = case("small")
    x, g, mp, R = k["x"], k["g"], k["mp"], k["R"]
    h = phaze_amd.Mirror(mp, R, max_channels=2, max_outputs=1024)

    def refused(grains, word, xx=x[:2], **kw):
        args = dict(out_first=0, nout=NOUT)
        args.update(kw)
        for fn in ("pv_mirror_process", "pv_mirror_process_device"):       # both forms check before any device work: host rows never reach the device
            rc, y, clean = _raw(h, xx, grains, args["out_first"], args["nout"], fn=fn)
            msg = h._L.pv_mirror_last_error(h._h).decode()
            assert rc == args.get("rc", capi.PV_ERR_ARGUMENT) and word in msg, (fn, rc, msg)
            assert clean and np.all(y == -77.0)

    assert g[10, 1] & BIT and g[13, 1] & BIT and not g[11, 1] & BIT and not g[9, 1] & BIT
    last = g.shape[0] - 1
    for idx, col, val, word in [(9, 1, 131072, "grain 9"), (10, 1, 131072 + int(g[10, 1]), "grain 10"), (9, 1, -1, "grain 9"),          # w >= 131072, w < 0
                                (10, 2, -(1 << 30), "grain 10"), (13, 2, -(1 << 31), "grain 13"),                                         # mirrored, D <= -2^30
                                (11, 2, 1 << 30, "grain 11"), (11, 2, -(1 << 30), "grain 11"),                                            # forward, |D| >= 2^30
                                (7, 3, 1, "grain 7"), (7, 3, mp + 1, "grain 7"), (10, 3, 0, "grain 10"),                                  # L out of range
                                (0, 0, -1, "grain 0"), (5, 0, 1 << 30, "grain 5"), (last, 0, 5, f"grain {last}"), (20, 0, int(g[19, 0]) - 1, "grain 20")]:
        bad = np.array(g)
        bad[idx, col] = val
        assert MM.check_grains(bad, mp)[0] == idx
        refused(bad, word)
    swapped = np.array(g)
    swapped[[30, 31]] = swapped[[31, 30]]
    refused(swapped, "grain 31")
    # a mirrored grain may have any D above -2^30 as far as validation goes; then the span refuses the tile and names its first grain
    for idx, val in ((10, (1 << 31) - 1), (13, 1 - (1 << 30)), (61, 100000)):
        wide = np.array(g)
        assert wide[idx, 1] & BIT
        wide[idx, 2] = val
        assert MM.check_grains(wide, mp) is None
        tile, first, extent = MM.check_span(wide, mp, R, 0, NOUT)
        assert extent > MM.span(mp, R) and tile == max(int(g[idx, 0]) - int(g[idx, 3]), 0) // TILE
        refused(wide, f"grain {first}:")
        msg = h._L.pv_mirror_last_error(h._h).decode()
        assert "span" in msg and str(extent) in msg and str(MM.span(mp, R)) in msg, msg
    refused(g, "max_channels", xx=x[:3], rc=capi.PV_ERR_CAPACITY)
    refused(g, "2^30", out_first=(1 << 30) - 5)
    out = np.full(8, -77.0, np.float32)
    xp, gp, op = x[0].ctypes.data_as(FP), g.ctypes.data_as(IP), out.ctypes.data_as(FP)
    for args in ((None, 100, 100, 1, gp, 3, op, 0, 8, 8), (xp, 100, 100, 1, None, 3, op, 0, 8, 8), (xp, 100, 100, 1, gp, 3, None, 0, 8, 8), (xp, -1, 100, 1, gp, 3, op, 0, 8, 8),
                 (xp, 100, 100, -1, gp, 3, op, 0, 8, 8), (xp, 100, 100, 1, gp, -3, op, 0, 8, 8), (xp, 100, 100, 1, gp, 3, op, -1, 8, 8), (xp, 100, 100, 1, gp, 3, op, 0, -8, 8),
                 (x.ctypes.data_as(FP), 100, 99, 2, gp, 3, op, 0, 4, 4), (x.ctypes.data_as(FP), 100, 100, 2, gp, 3, op, 0, 4, 3)):
        for fn in (h._L.pv_mirror_process, h._L.pv_mirror_process_device):
            assert fn(h._h, *args) == capi.PV_ERR_ARGUMENT and np.all(out == -77.0), args[1:6]
    assert "null" in h._L.pv_mirror_last_error(h._h).decode() or "stride" in h._L.pv_mirror_last_error(h._h).decode()
    # a wrong struct_size, with a device present
    hh = C.c_void_p()
    for delta in (-4, 4):
        cfg = capi.make_mirror_config(mp, R)
        cfg.struct_size += delta
        assert h._L.pv_mirror_create(C.byref(cfg), C.byref(hh)) == capi.PV_ERR_ARGUMENT and "struct_size" in h._L.pv_mirror_last_error(None).decode()
    # the handle still works, and a call without channels or outputs does nothing
    assert h._L.pv_mirror_process(h._h, None, 0, 0, 0, None, 0, None, 0, 0, 0) == 0
    assert np.all(np.abs(h.process(x[:2], g, 0, NOUT) - k["y"][:2]) <= k["tol"][:2])
    h.close()
    assert h._L.pv_mirror_destroy(None) == capi.PV_ERR_ARGUMENT


def test_a_planned_table_of_tone_then_noise_at_half_speed_and_process_tuned():
    """The voice-like tone at 452 Hz, then white noise, twelve thousand samples in all, at half speed.  process_tuned returns the model's grains (the
    device's f0 records are the model's, tests/test_gpu_f0.py) with the noise's reuses mirrored and no voiced grain mirrored, an output of the model's
    output_len and the bits of process(x, grains); the kernel's output is within the derived bound of the model on that table; mirror=False gives
    Tsm.process_tuned's grains and bits."""
    import phaze_amd
    n = FM.PLAN_LEN
    rng = np.random.default_rng(12)
    x = np.stack([PM.voice(FM.SAMPLE_RATE / 452.0, n), PM.voice(FM.SAMPLE_RATE / 452.0, n, phase=0.3)]).astype(np.float32)
    x[:, n // 2:] = (0.1 * rng.standard_normal((2, n - n // 2))).astype(np.float32)
    h = phaze_amd.Mirror(1024, 2, max_channels=2)
    y, grains = h.process_tuned(x, FM.SAMPLE_RATE, rate=0.5)
    recs = FM.track(x[0], 1024, 256, 32, 1024)
    nrec = recs.shape[0]
    ratios = PM.tune_ratios(recs, FM.SAMPLE_RATE)
    want, want_len, A, voiced = MM.mirror_plan(recs, 256, 1024, n, 256.0, 32, 1024, ratios=ratios, rates=np.full(nrec, 0.5), details=True)
    mir = MM.mirrored(want)
    print(f"{nrec} records, {int(np.sum(recs[:, 0] > 0))} voiced; {want.shape[0]} grains, {int(mir.sum())} mirrored; output {want_len} of {n}")
    assert np.array_equal(grains, want) and y.shape == (2, want_len) and mir.sum() >= 10 and not np.any(mir & voiced) and voiced.sum() > 50
    assert np.array_equal(y, h.process(x, grains, 0, want_len))
    model, tol, poisoned = MM.process(x, want, 0, want_len, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
    err = np.abs(y.astype(np.float64) - model)
    print(f"worst |err| / bound = {float(np.max(err[tol > 0] / tol[tol > 0])):.3f}")
    assert not poisoned.any() and np.all(err <= tol) and np.all(y[tol == 0] == 0.0)
    y_off, g_off = h.process_tuned(x, FM.SAMPLE_RATE, rate=0.5, mirror=False)
    ts = phaze_amd.Tsm(1024, 2, max_channels=2)
    y_ts, g_ts = ts.process_tuned(x, FM.SAMPLE_RATE, rate=0.5)
    ts.close()
    assert np.array_equal(g_off, g_ts) and np.array_equal(y_off, y_ts) and not MM.mirrored(g_off).any()
    # the reason for it all, on the device's output: the noise part of the mirrored output has at most half the forward one's figure at the mark spacing
    lo, hi = 5 * want_len // 8, 7 * want_len // 8
    fig = [MM.buzz(v[0, lo:hi], 256, 256, 0)[0] for v in (y_off, y)]
    print(f"autocorrelation of the noise part at lag 256: forward {fig[0]:.3f}, mirrored {fig[1]:.3f}")
    assert fig[1] <= 0.5 * fig[0]
    with pytest.raises(ValueError):
        h.process_tuned(x, FM.SAMPLE_RATE, rate=np.full(nrec - 1, 0.5))
    h.close()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_mirror_example_lowers_the_buzz_and_its_pieces_equal_the_whole(tmp_path):
    import test_mirror_abi as TMA
    exe = TMA.build_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    print(j)
    assert j["pieces_equal_whole"] is True and j["forward"]["mirrored"] == 0 and j["mirrored"]["mirrored"] > 50
    assert j["forward"]["samples"] == j["mirrored"]["samples"] and abs(j["forward"]["samples"] - 2 * j["samples"]) <= 2 * 1024
    assert j["mirrored"]["autocorrelation"] <= 0.5 * j["forward"]["autocorrelation"]
