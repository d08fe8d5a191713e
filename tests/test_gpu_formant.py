"""The warped-grain kernel (Formant / pv_formant_*) on the GPU against the numpy model (tests/formant_model.py), bit equality with Tsm.process on tables
without warped grains, and partition invariance.

Tolerance against the model, DERIVED, u = 2^-24.  For the unwarped grains of a table the kernel's arithmetic is pv_tsm_kernel's operation for operation and
the bound of tests/test_gpu_psola.py's docstring holds unchanged (tests/test_gpu_tsm.py restates it): per grain with a fractional displacement
|xt^ - xt| <= e_g = u [64 (a_g + |xt| s_g) / |d_g| + |xt|], 0 for a whole-sample displacement; the window weight is within 3 u m of h, m = |h| + |f d|; and
with G grains covering an output
    |y_gpu - y| <= [ (G + 3) u (A + |y| S) + E ] / D + u |y|,   A = sum m_g |xt_g|, S = sum m_g, D = sum h_g, E = sum |h_g| e_g,
times 1 + 2^-10 for the second order, plus 2^-149 (1 + (G + 3 + T) / D) for an intermediate in the subnormal range, T the most taps of a grain of the table.
Only e_g changes for a WARPED grain, and it is the bound of tests/test_gpu_vari.py's docstring for the same weight rule: the kernel's weight is
w^ = fl(fma(f^, d^, P[q])) with f^ = fl(rem * fl(1 / den)) (rem < 2^16 and den <= 512 are exact in f32) and d^ = fl(P[q + 1] - P[q]): three roundings on
the product f d and one on the result, so |w^ - w| <= 3 u m_i with m_i = |w_i| + |f_i d_i|.  A tap whose weight is exactly 0 adds nothing and rounds
nothing; with Tloc <= 128 non-zero taps the numerator, Tloc fused multiply-adds into one f32 accumulator, is within (Tloc + 3) u a_g of sum w x,
a_g = sum m_i |x_i|, and the weight sum within (Tloc + 3) u s_g of d_g = sum w_i, s_g = sum m_i; the one division adds the two relative errors and rounds
once:
    e_g = u [ (Tloc + 3) (a_g + |xt| s_g) / |d_g| + |xt| ].
The window and fold terms are unchanged.  formant_model.process(bound=True) returns the bound per sample; the model forms its sums in fp64 from the
library's own P and Hn and the same f32 input, with the integer rule for m, r, q and rem.  No sample is left out; an output no grain covers must be exactly
0.  Everything else is bit for bit.
Worst observed |err| / bound over all cases: 0.156 (`small` with every third grain warped); 0.05 and below on the other mixed tables, 0.046 on the planned
table.  One MI355X."""
import ctypes as C
import json
import shutil
import subprocess

import numpy as np
import pytest

import f0_model as FM
import formant_model as FoM
import psola_model as PM
import test_formant_abi as TFA
import test_gpu_tsm as TGT
import test_psola_model as TPM

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int32)
TILE = TGT.TILE
NOUT = TGT.NOUT
NCH = TGT.NCH
STEP = FoM.STEP
UNWARPED = ["small", "mid", "tiny", "sweep", "gap", "empty", "slow", "fast"]          # the tables of tests/test_gpu_tsm.py whose max_period the handle accepts
MIXED = [("small", 3), ("tiny", 3), ("mid", 3), ("sweep", 3), ("gap", 3), ("small", 1), ("tiny", 1), ("mid", 1)]


def _mixed(name, every):
    """(max_period, max_rate, nin, grains): the far table `name` of tests/test_gpu_tsm.py with every third grain (every = 3) or every grain (every = 1) warped,
    steps from {128, 129, 200, 255, 257, 300, 511, 512}, phi through 0, 1, 255 and tf through 0, 255 (test_formant_abi.warp_table).  A warped grain reads up
    to max_period further to either side than its unwarped twin; the handle's span has that room."""
    mp, R, nin, g = TGT._grains(name)
    m = TFA.warp_table(g, every, 1 if every > 1 else 0)
    assert FoM.check_grains(m, mp) is None and FoM.check_span(m, mp, R, 0, NOUT) is None, (FoM.check_grains(m, mp), FoM.check_span(m, mp, R, 0, NOUT), FoM.span(mp, R))
    k = FoM.warped(m)
    s, phi, tf = FoM.steps(m)[k], (m[k, 1] >> 8) & 255, m[k, 1] & 255
    assert k.sum() < 16 or (set(s.tolist()) == set(TFA.STEPS) and {0, 1, 255} <= set(phi.tolist()) and {0, 255} <= set(tf.tolist()))
    return mp, R, nin, m


_CACHE = {}


def case(name, every=3):
    """Shared per mixed table, computed once and never written: the input, the grains, the model's output on the library's tables and its bound."""
    if (name, every) not in _CACHE:
        import phaze_amd
        mp, R, nin, g = _mixed(name, every)
        x = TGT._signals(nin, 7 + len(name))
        y, tol, poisoned = FoM.process(x, g, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
        assert not poisoned.any()
        for a in (x, g, y, tol):
            a.setflags(write=False)
        _CACHE[(name, every)] = dict(mp=mp, R=R, n=nin, g=g, x=x, y=y, tol=tol)
    return _CACHE[(name, every)]


def _raw(h, x, g, out_first, nout, pad_in=0, pad_out=0, lead=0, fn="pv_formant_process"):
    return TGT._raw(h, x, g, out_first, nout, pad_in, pad_out, lead, fn)


@pytest.mark.parametrize("name", UNWARPED)
def test_unwarped_tables_give_the_bits_of_tsm_process(name):
    """The far tables of tests/test_gpu_tsm.py have no warped grain, written with z = 0 or with z = 256: Tsm.process's output with ==, from the host form, a
    range in the middle and the device form."""
    import phaze_amd
    k = TGT.case(name)
    x, g, mp, R = k["x"], k["g"], k["mp"], k["R"]
    ts = phaze_amd.Tsm(mp, R, max_channels=NCH, max_outputs=NOUT)
    want = ts.process(x, g, 0, NOUT)
    ts.close()
    same = np.array(g)
    same[:, 1] += 256 * STEP
    h = phaze_amd.Formant(mp, R, max_channels=NCH, max_outputs=NOUT)
    for table in (g, same):
        got = h.process(x, table, 0, NOUT)
        assert got.dtype == np.float32 and np.array_equal(got, want), (name, int(np.sum(got != want)))
        assert np.array_equal(h.process(x, table, 1001, 1500), want[:, 1001:2501])
        assert np.array_equal(TGT._device(h, x, table, [0, 1500, NOUT]), want)
    h.close()


@pytest.mark.parametrize("name,every", MIXED)
def test_every_sample_of_a_mixed_table_is_within_the_derived_bound_of_the_model(name, every):
    import phaze_amd
    k = case(name, every)
    covered = k["tol"][0] > 0
    wr = FoM.warped(k["g"])
    assert wr.all() if every == 1 else (wr.sum() >= k["g"].shape[0] // 3 - 1 and not wr.all())
    if name == "gap":
        assert not covered[975:2210].any() and not covered[TILE:2 * TILE].any()
    if name == "tiny":
        assert np.all(FoM.tiles(k["g"], k["mp"], 0, NOUT)[:3, 1] - FoM.tiles(k["g"], k["mp"], 0, NOUT)[:3, 0] > 300)
    for nch, pads, lead in ((1, (0, 0), 0), (3, (5, 129), 1)):
        h = phaze_amd.Formant(k["mp"], k["R"], max_channels=nch, max_outputs=NOUT)
        rc, y, clean = _raw(h, k["x"][:nch], k["g"], 0, NOUT, *pads, lead=lead)
        assert rc == 0 and clean, h._L.pv_formant_last_error(h._h)
        err = np.abs(y.astype(np.float64) - k["y"][:nch])
        tol = k["tol"][:nch]
        live = covered[None, :] & (tol > 0)
        worst = float(np.max(err[live] / tol[live])) if live.any() else 0.0
        print(f"{name} every {every} nch {nch}: worst |err| / bound = {worst:.3f}, max |err| = {err.max():.3e}")
        assert np.all(err <= tol), (nch, int(np.sum(err > tol)), worst)
        assert np.all(y[:, ~covered] == 0.0) and not np.any(np.signbit(y[:, ~covered]))          # no grain: exact zeros
        h.close()


@pytest.mark.parametrize("name,every", [("small", 3), ("tiny", 3), ("mid", 3), ("sweep", 3), ("tiny", 1)])
def test_any_partition_and_every_form_give_the_same_bits(name, every):
    """One call, a repeated call, three calls split at odd outputs, a range in the middle, a channel alone, the host form in pieces of one tile, the device
    form in one call and in three on a user stream."""
    import phaze_amd
    import torch
    k = case(name, every)
    x, g, mp, R = k["x"], k["g"], k["mp"], k["R"]
    h = phaze_amd.Formant(mp, R, max_channels=NCH, max_outputs=NOUT)
    rc, want, clean = _raw(h, x, g, 0, NOUT)
    assert rc == 0 and clean
    assert np.array_equal(h.process(x, g, 0, NOUT), want)                                    # the binding, and a repeated call
    cuts = [0, 1001, 2333, NOUT]                                                             # the tiles of a call start at its first output
    assert all(FoM.check_span(g, mp, R, a, b - a) is None for a, b in zip(cuts[:-1], cuts[1:]))
    parts = [h.process(x, g, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts, axis=1), want)
    assert np.array_equal(h.process(x, g, 1001, 1500), want[:, 1001:2501])
    assert np.array_equal(h.process(x, g, 5, 0), np.zeros((NCH, 0), np.float32))
    for c in range(NCH):
        assert np.array_equal(h.process(x[c], g, 0, NOUT), want[c])
    assert np.array_equal(TGT._device(h, x, g, [0, NOUT]), want)
    h.close()
    small = phaze_amd.Formant(mp, R, max_channels=NCH, max_outputs=1)
    rc, y, clean = _raw(small, x, g, 0, NOUT, 3, 2, lead=1)
    assert rc == 0 and clean and np.array_equal(y, want)
    small.close()
    h = phaze_amd.Formant(mp, R, max_channels=NCH)
    assert np.array_equal(TGT._device(h, x, g, cuts, stream=torch.cuda.Stream()), want)
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


@pytest.mark.parametrize("mp,R", [(64, 1), (1024, 4), (3753, 1)])
def test_a_warped_grain_may_bring_a_tile_to_exactly_the_span_and_no_further(mp, R):
    """Tile 0 holds an unwarped grain that reads from position 3 on and a grain of step 512 whose range ends at 791 - D: with D = 788 - span the tile's extent
    is exactly span(max_period, max_rate) and the call is accepted and within the bound; one sample more is refused with PV_ERR_ARGUMENT, the message names
    the tile's first grain and the extent, and the output keeps its fill."""
    import phaze_amd
    from phaze_amd import capi
    cap = FoM.span(mp, R)
    nin = cap + 700
    x = TGT._signals(nin, 3)[:2]
    table = lambda D: np.array([[100, 7, 0, 64], [600, 512 * STEP + 256 * 77 + 200, D, 64]], np.int32)
    g = table(788 - cap)
    assert FoM.check_grains(g, mp) is None and FoM.tiles(g, mp, 0, TILE).tolist() == [[0, 2, 3, cap]], FoM.tiles(g, mp, 0, TILE).tolist()
    h = phaze_amd.Formant(mp, R, max_channels=2, max_outputs=TILE)
    y, tol, _ = FoM.process(x, g, 0, TILE, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
    for fn in ("pv_formant_process", "pv_formant_process_device"):
        wide = table(787 - cap)
        assert FoM.check_grains(wide, mp) is None and FoM.check_span(wide, mp, R, 0, TILE) == (0, 0, cap + 1)
        rc, out, clean = _raw(h, x, wide, 0, TILE, fn=fn)                   # host rows never reach the device: refused before any device work
        msg = h._L.pv_formant_last_error(h._h).decode()
        assert rc == capi.PV_ERR_ARGUMENT and "grain 0:" in msg and "span" in msg and str(cap + 1) in msg and str(cap) in msg, msg
        assert clean and np.all(out == -77.0)
    rc, out, clean = _raw(h, x, g, 0, TILE)
    assert rc == 0 and clean and np.all(np.abs(out - y) <= tol) and np.any(out[:, 540:660] != 0.0)
    assert np.array_equal(_device_tile(h, x, g), out)
    h.close()


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_outputs_are_exactly_the_models(value):
    """A non-finite sample reaches exactly the outputs that have it under a tap of a grain with a non-zero weight: the zero-weight rule.  Under the outermost
    tap of a warped grain's first output (weight 0 for most fractions), under its centre, and under an unwarped grain.  The finite outputs keep their bits in
    every form."""
    import phaze_amd
    for name in ("small", "tiny"):
        k = case(name)
        g, mp = k["g"], k["mp"]
        x = np.array(k["x"])
        n = x.shape[1]
        wr = np.flatnonzero(FoM.warped(g))
        for j, c in ((wr[wr.size // 2], 0), (wr[wr.size // 3], 1), (wr[wr.size // 5], 2), (wr[1], 0), (wr[2] + 1, 1), (wr[3], 2)):
            t, w, D, L = (int(v) for v in g[j])
            if w >> 17:
                s, W = w >> 17, 32 if (w >> 17) < 256 else 64
                m0 = int(FoM._m(t, w & 255, (w >> 8) & 255, D, s, t - L + 1)[0])
                x[c, min(max(m0 - W + 1, 0), n - 1)] = value                # tap 0 of the grain's first output: weight 0 unless r is 0
                x[c, min(max(m0 + W, 0), n - 1)] = value                    # its last tap
                x[c, min(max(t - D, 0), n - 1)] = -value if value == value else value
            else:
                x[c, min(max(t - D, 0), n - 1)] = value
        y, tol, poisoned = FoM.process(x, g, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
        h = phaze_amd.Formant(mp, k["R"], max_channels=NCH, max_outputs=1024)
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
    h = phaze_amd.Formant(mp, R, max_channels=2, max_outputs=1024)

    def refused(grains, word, xx=x[:2], **kw):
        args = dict(out_first=0, nout=NOUT)
        args.update(kw)
        for fn in ("pv_formant_process", "pv_formant_process_device"):     # both forms check before any device work: host rows never reach the device
            rc, y, clean = _raw(h, xx, grains, args["out_first"], args["nout"], fn=fn)
            msg = h._L.pv_formant_last_error(h._h).decode()
            assert rc == args.get("rc", capi.PV_ERR_ARGUMENT) and word in msg, (fn, rc, msg)
            assert clean and np.all(y == -77.0)

    assert g[10, 1] >> 17 and g[13, 1] >> 17 and not g[11, 1] >> 17 and not g[9, 1] >> 17
    last = g.shape[0] - 1
    for idx, col, val, word in [(9, 1, 1 << 27, "grain 9"), (10, 1, (1 << 27) + int(g[10, 1]), "grain 10"), (9, 1, -1, "grain 9"),           # w >= 2^27, w < 0
                                (9, 1, 127 * STEP + 5, "grain 9"), (10, 1, 513 * STEP, "grain 10"), (9, 1, STEP, "grain 9"),                   # z = 127, 513, 1
                                (9, 1, 65536 + int(g[9, 1]), "grain 9"), (10, 1, 65536 + int(g[10, 1]), "grain 10"),                            # a set mirror bit
                                (10, 2, -(1 << 30), "grain 10"), (11, 2, 1 << 30, "grain 11"), (13, 2, 1 << 30, "grain 13"),                    # |D| >= 2^30
                                (7, 3, 1, "grain 7"), (7, 3, mp + 1, "grain 7"), (10, 3, 0, "grain 10"),                                       # L out of range
                                (0, 0, -1, "grain 0"), (5, 0, 1 << 30, "grain 5"), (last, 0, 5, f"grain {last}"), (20, 0, int(g[19, 0]) - 1, "grain 20")]:
        bad = np.array(g)
        bad[idx, col] = val
        assert FoM.check_grains(bad, mp)[0] == idx
        refused(bad, word)
    swapped = np.array(g)
    swapped[[30, 31]] = swapped[[31, 30]]
    refused(swapped, "grain 31")
    # a displacement of any size passes validation; then the span refuses the tile and names its first grain
    for idx, val in ((10, (1 << 30) - 1), (13, 1 - (1 << 30)), (61, 100000)):
        wide = np.array(g)
        assert wide[idx, 1] >> 17
        wide[idx, 2] = val
        assert FoM.check_grains(wide, mp) is None
        tile, first, extent = FoM.check_span(wide, mp, R, 0, NOUT)
        assert extent > FoM.span(mp, R) and tile == max(int(g[idx, 0]) - int(g[idx, 3]), 0) // TILE
        refused(wide, f"grain {first}:")
        msg = h._L.pv_formant_last_error(h._h).decode()
        assert "span" in msg and str(extent) in msg and str(FoM.span(mp, R)) in msg, msg
    refused(g, "max_channels", xx=x[:3], rc=capi.PV_ERR_CAPACITY)
    refused(g, "2^30", out_first=(1 << 30) - 5)
    out = np.full(8, -77.0, np.float32)
    xp, gp, op = x[0].ctypes.data_as(FP), g.ctypes.data_as(IP), out.ctypes.data_as(FP)
    for args in ((None, 100, 100, 1, gp, 3, op, 0, 8, 8), (xp, 100, 100, 1, None, 3, op, 0, 8, 8), (xp, 100, 100, 1, gp, 3, None, 0, 8, 8), (xp, -1, 100, 1, gp, 3, op, 0, 8, 8),
                 (xp, 100, 100, -1, gp, 3, op, 0, 8, 8), (xp, 100, 100, 1, gp, -3, op, 0, 8, 8), (xp, 100, 100, 1, gp, 3, op, -1, 8, 8), (xp, 100, 100, 1, gp, 3, op, 0, -8, 8),
                 (x.ctypes.data_as(FP), 100, 99, 2, gp, 3, op, 0, 4, 4), (x.ctypes.data_as(FP), 100, 100, 2, gp, 3, op, 0, 4, 3)):
        for fn in (h._L.pv_formant_process, h._L.pv_formant_process_device):
            assert fn(h._h, *args) == capi.PV_ERR_ARGUMENT and np.all(out == -77.0), args[1:6]
    # the handle still works, and a call without channels or outputs does nothing
    assert h._L.pv_formant_process(h._h, None, 0, 0, 0, None, 0, None, 0, 0, 0) == 0
    assert np.all(np.abs(h.process(x[:2], g, 0, NOUT) - k["y"][:2]) <= k["tol"][:2])
    h.close()
    assert h._L.pv_formant_destroy(None) == capi.PV_ERR_ARGUMENT


def test_a_planned_table_at_warp_five_quarters_and_half_speed_and_process_tuned():
    """The voice of tests/test_psola_model.py (period 217.3, resonators at 1200 and 2600 Hz), twelve thousand samples, at warp 1.25 and rate 1/2, strength 0
    (the pitch stays).  process_tuned returns the model's grains (the device's f0 records are the model's, tests/test_gpu_f0.py) and output_len and the bits
    of process(x, grains); the kernel's output is within the derived bound of the model on that table; its strongest harmonic lies within one f0 of
    1200 * 1.25 and is not the harmonic nearest 1200 Hz; warp = 1.0 gives Tsm.process_tuned's grains and bits."""
    import phaze_amd
    n = FM.PLAN_LEN
    p = FM.period(PM.records_of([TPM.PERIOD])[0])
    x = np.stack([PM.voice(p, n), PM.voice(p, n, phase=0.3)]).astype(np.float32)
    h = phaze_amd.Formant(1024, 2, max_channels=2)
    y, grains = h.process_tuned(x, FM.SAMPLE_RATE, warp=1.25, rate=0.5, strength=0.0)
    recs = FM.track(x[0], 1024, 256, 32, 1024)
    nrec = recs.shape[0]
    ratios = PM.tune_ratios(recs, FM.SAMPLE_RATE, strength=0.0)
    want, want_len = FoM.formant_plan(recs, 256, 1024, n, 256.0, 32, 1024, ratios=ratios, rates=np.full(nrec, 0.5), warps=np.full(nrec, 1.25))
    wr = FoM.warped(want)
    print(f"{nrec} records, {int(np.sum(recs[:, 0] > 0))} voiced; {want.shape[0]} grains, {int(wr.sum())} warped; output {want_len} of {n}")
    assert np.array_equal(grains, want) and y.shape == (2, want_len) and wr.all() and np.all(FoM.steps(want) == 320) and abs(want_len - 2 * n) <= 2048
    assert np.array_equal(y, h.process(x, grains, 0, want_len))
    model, tol, poisoned = FoM.process(x, want, 0, want_len, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
    err = np.abs(y.astype(np.float64) - model)
    print(f"worst |err| / bound = {float(np.max(err[tol > 0] / tol[tol > 0])):.3f}")
    assert not poisoned.any() and np.all(err <= tol) and np.all(y[tol == 0] == 0.0)
    f, a, res = PM.harmonic_amplitudes(y[0], p, want_len // 4, 3 * want_len // 4)
    hz = f * FM.SAMPLE_RATE
    peak, f0 = float(hz[np.argmax(a)]), FM.SAMPLE_RATE / p
    print(f"strongest harmonic {peak:.0f} Hz, {abs(peak - 1500.0) / f0:.2f} f0 from 1500 Hz; residual {res:.1e}")
    assert res < 0.01 and abs(peak - 1200.0 * 1.25) < f0 and peak != float(hz[np.argmin(np.abs(hz - 1200.0))])
    y_one, g_one = h.process_tuned(x, FM.SAMPLE_RATE, warp=1.0, rate=0.5, strength=0.0)
    ts = phaze_amd.Tsm(1024, 2, max_channels=2)
    y_ts, g_ts = ts.process_tuned(x, FM.SAMPLE_RATE, rate=0.5, strength=0.0)
    ts.close()
    assert np.array_equal(g_one, g_ts) and np.array_equal(y_one, y_ts) and not FoM.warped(g_one).any()
    with pytest.raises(ValueError):
        h.process_tuned(x, FM.SAMPLE_RATE, warp=np.full(nrec - 1, 1.25))
    with pytest.raises(ValueError):
        h.process_tuned(x, FM.SAMPLE_RATE, warp=2.5)
    h.close()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_formant_example_moves_the_formant_and_its_pieces_equal_the_whole(tmp_path):
    exe = TFA.build_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    print(j)
    assert j["one_call_equals_pieces"] is True and j["up"]["warped"] == j["up"]["grains"] > 50 and j["down"]["warped"] == j["down"]["grains"] > 50
    for side, warp in (("up", 1.25), ("down", 0.8)):
        assert abs(j[side]["note"] - 69.0) < 0.1 and j[side]["samples"] == j["samples"]                  # on A4, whatever the warp
        assert abs(j[side]["strongest_harmonic"] - 1200.0 * warp) < 440.0, j[side]                        # the first formant moved with it
    assert abs(j["strongest_harmonic_in"] - 1200.0) < 452.0
