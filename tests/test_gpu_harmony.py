"""The harmony kernel (Harmony / pv_harmony_*) on the GPU: bit equality with the numpy float32 fold of the per-voice Tsm.process outputs, the derived bound
against the numpy model (tests/harmony_model.py), partition invariance, the hull, muting, every refusal and process_tuned.

Tolerance against the model: the kernel's y_v is pv_tsm_kernel's arithmetic operation for operation, so it is within tol_v, the derived bound of
tests/test_gpu_tsm.py's docstring, of the model's y_v.  The fold rounds one product and one add per voice, each within 2^-24 relative of a partial sum of
at most sum |g_v| (|y_v| + tol_v), so
    |out_gpu - sum g_v y_v| <= sum |g_v| tol_v + (V + 1) 2^-24 sum |g_v| (|y_v| + tol_v) + V 2^-149,
the sums over the voices that are not skipped; the last term is for products in the subnormal range (tol_v carries the subnormal slack of the tsm bound).
harmony_model.process(bound=True) restates it.  No sample is left out; an output no voice covers must be exactly 0.  Everything else is bit for bit.
Worst observed |err| / bound over all cases: 0.18 (small2, three channels; one MI355X)."""
import ctypes as C
import json
import shutil
import subprocess

import numpy as np
import pytest

import f0_model as FM
import harmony_model as HM
import psola_model as PM
import test_gpu_tsm as TGT
import tsm_model as TM

pytestmark = pytest.mark.gpu

FP, IP, LP = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
TILE = 1024
NOUT = 3 * TILE + 37
NCH = 3
C_MAJOR = sum(1 << k for k in (0, 2, 4, 5, 7, 9, 11))


def _voices(name):
    """(max_period, max_rate, nin, [far grains int32[., 4] per voice]).  Every table spans three tiles and 37 outputs; the voices have different densities,
    one is empty and one has a gap (outputs 990 .. 2209 and the whole second tile) in the cases of eight."""
    rng = np.random.default_rng(len(name) * 211 + ord(name[-1]))
    n = NOUT
    nv = int(name[-1])
    if name.startswith("small"):       # max_period 64 at max_rate 4: the voices read at four times the output position
        mp, R, nin = 64, 4, 4 * n
        strides, jitter = [19, 7, 5, 11, 13, 23, 29, 40][:nv], 60
        lengths = lambda m: rng.integers(2, 65, m)
    else:                              # max_period 1024 at max_rate 4
        mp, R, nin = 1024, 4, 4 * n
        strides, jitter = [211, 97, 61, 150, 333, 41, 500, 120][:nv], 900
        lengths = lambda m: rng.choice([2, 300, 700, 1024], m)
    tables = []
    for v, stride in enumerate(strides):
        t = np.arange(v, n + mp - 4, stride)
        if nv == 8 and v == 5:
            t = np.concatenate([np.arange(3, 951, stride), np.arange(2250, n, stride)])
        g = TGT._far_table(rng, t, 40 if (nv == 8 and v == 5) else lengths(t.size), 3.0, jitter)
        if nv == 8 and v == 3:
            g = g[:0]
        tables.append(np.ascontiguousarray(g, np.int32).reshape(-1, 4))
    assert HM.check_voices(tables, mp) is None, HM.check_voices(tables, mp)
    assert HM.check_span(tables, mp, R, 0, NOUT) is None, (HM.check_span(tables, mp, R, 0, NOUT), TM.span(mp, R))
    return mp, R, nin, tables


CASES = ["small2", "small8", "mid2", "mid8"]
_CACHE = {}


def case(name):
    """Shared per case, computed once and never written: the input, the voices, the gains, the model's output on the library's tables and its bound, and which
    outputs each voice covers."""
    if name not in _CACHE:
        import phaze_amd
        mp, R, nin, tables = _voices(name)
        nv = len(tables)
        x = TGT._signals(nin, 11 + len(name))
        rng = np.random.default_rng(99 + nv)
        gains = rng.uniform(-1.5, 1.5, (nv, NCH)).astype(np.float32)
        gains[nv - 1, 2] = 0.0                                               # the last voice is muted on channel 2
        P, H = phaze_amd.vari_prototype(), phaze_amd.psola_window()
        outs = [TM.process(x, t, 0, NOUT, P, H, bound=True) for t in tables]
        y, tol, poisoned = HM.process(x, tables, gains, 0, NOUT, bound=True, outs=outs)
        covered = np.stack([o[1][0] > 0 for o in outs])
        assert not poisoned.any()
        for a in [x, gains, y, tol, covered] + tables:
            a.setflags(write=False)
        _CACHE[name] = dict(mp=mp, R=R, n=nin, tables=tables, x=x, gains=gains, y=y, tol=tol, covered=covered)
    return _CACHE[name]


def _flat(tables):
    first = np.zeros(len(tables) + 1, np.int64)
    first[1:] = np.cumsum([t.shape[0] for t in tables])
    g = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int32).reshape(-1, 4) for t in tables]), np.int32)
    return g, first


def _raw(h, x, tables, gains, out_first, nout, pad_in=0, pad_out=0, lead=0, fn="pv_harmony_process", first=None, nvoices=None, null_gains=False):
    """One host call through the raw C entry point: rows `lead` floats into their buffers (lead = 1: four bytes off any alignment) and strides longer than the
    rows.  Returns (rc, out rows, whether everything around the rows still holds the fill)."""
    nch, nin = x.shape
    xin = np.full(lead + nch * (nin + pad_in), np.nan, np.float32)
    rows = xin[lead:].reshape(nch, nin + pad_in)
    rows[:, :nin] = x
    out = np.full(lead + nch * (nout + pad_out) + 3, -77.0, np.float32)
    orow = out[lead:lead + nch * (nout + pad_out)].reshape(nch, nout + pad_out)
    g, vf = _flat(tables)
    vf = vf if first is None else np.asarray(first, np.int64)
    w = np.ascontiguousarray(gains, np.float32)
    rc = getattr(h._L, fn)(h._h, rows.ctypes.data_as(FP), nin, nin + pad_in, nch, g.ctypes.data_as(IP) if g.size else None, None if vf.size == 0 else vf.ctypes.data_as(LP),
                           len(tables) if nvoices is None else nvoices, None if null_gains else w.ctypes.data_as(FP), orow.ctypes.data_as(FP), out_first, nout,
                           nout + pad_out)
    clean = bool(np.all(orow[:, nout:] == -77.0) and np.all(out[:lead] == -77.0) and np.all(out[lead + nch * (nout + pad_out):] == -77.0))
    return rc, orow[:, :nout].copy(), clean


def _device(h, x, tables, gains, cuts, stream=None):
    """The device form in the calls `cuts`, padded strides, rows four bytes off their alignment; checks that nothing around the rows was written."""
    import torch
    nch, n = x.shape
    if stream is not None:
        h.set_stream(stream.cuda_stream)
    d_in = torch.full((nch * (n + 7) + 1,), float("nan"), dtype=torch.float32, device="cuda")
    d_in[1:].view(nch, n + 7)[:, :n] = torch.from_numpy(x.copy()).cuda()
    d_out = torch.full((nch * (NOUT + 5) + 1,), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for a, b in zip(cuts[:-1], cuts[1:]):
        h.process_device(d_in.data_ptr() + 4, n, n + 7, nch, tables, gains, d_out.data_ptr() + 4 + 4 * a, a, b - a, NOUT + 5)
    h.synchronize()
    if stream is not None:
        h.set_stream(None)
    got = d_out.cpu().numpy()
    assert got[0] == -77.0 and np.all(got[1:].reshape(nch, NOUT + 5)[:, NOUT:] == -77.0)
    return got[1:].reshape(nch, NOUT + 5)[:, :NOUT].copy()


def _per_voice(mp, R, x, tables, nout=NOUT):
    """float32[V, nch, nout]: Tsm.process of every voice alone."""
    import phaze_amd
    ts = phaze_amd.Tsm(mp, R, max_channels=x.shape[0], max_outputs=nout)
    ys = np.stack([ts.process(x, t, 0, nout) for t in tables])
    ts.close()
    return ys


def test_one_voice_at_gain_one_is_tsm_process():
    """The values of Tsm.process, -0 and +0 equal (the fold starts from +0), from the host form and the device form, on a synthetic and a planned table."""
    import phaze_amd
    for name in ("small", "slow", "gap"):
        mp, R, nin, g = TGT._grains(name)
        k = dict(mp=mp, R=R, g=g, x=TGT._signals(nin, 7 + len(name)))
        ts = phaze_amd.Tsm(k["mp"], k["R"], max_channels=NCH, max_outputs=NOUT)
        want = ts.process(k["x"], k["g"], 0, NOUT)
        ts.close()
        h = phaze_amd.Harmony(k["mp"], k["R"], max_voices=1, max_channels=NCH, max_outputs=NOUT)
        got = h.process(k["x"], [k["g"]], [1.0], 0, NOUT)
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want), (name, int(np.sum(got != want)))
        assert np.array_equal(_device(h, k["x"], [k["g"]], [1.0], [0, NOUT]), want)
        assert np.array_equal(h.process(k["x"][1], [k["g"]], [1.0], 1001, 1500), want[1, 1001:2501])
        h.close()


@pytest.mark.parametrize("name", CASES)
def test_the_mix_is_the_float32_fold_of_tsm_process_and_within_the_bound_of_the_model(name):
    import phaze_amd
    k = case(name)
    nv = len(k["tables"])
    ys = _per_voice(k["mp"], k["R"], k["x"], k["tables"])
    any_voice = k["covered"].any(axis=0)
    if nv == 8:
        assert k["tables"][3].shape[0] == 0 and not k["covered"][3].any() and not k["covered"][5][TILE:2 * TILE].any() and k["covered"][5][:900].all()
    for nch, pads, lead in ((1, (0, 0), 0), (3, (5, 129), 1)):
        gains = k["gains"][:, :nch]
        h = phaze_amd.Harmony(k["mp"], k["R"], max_voices=nv, max_channels=nch, max_outputs=NOUT)
        rc, y, clean = _raw(h, k["x"][:nch], k["tables"], gains, 0, NOUT, *pads, lead=lead)
        assert rc == 0 and clean, h._L.pv_harmony_last_error(h._h)
        want = HM.mix(ys[:, :nch], k["covered"], gains)
        assert np.array_equal(y, want), (nch, int(np.sum(y != want)))
        if nch == 1:
            assert np.array_equal(h.process(k["x"][0], k["tables"], gains[:, 0], 0, NOUT), want[0])          # gains of shape [V]
        ym, tol = k["y"][:nch], k["tol"][:nch]                                                              # channels are independent
        err = np.abs(y.astype(np.float64) - ym)
        live = tol > 0
        worst = float(np.max(err[live] / tol[live])) if live.any() else 0.0
        print(f"{name} nch {nch}: worst |err| / bound = {worst:.3f}, max |err| = {err.max():.3e}")
        assert np.all(err <= tol), (nch, int(np.sum(err > tol)), worst)
        assert np.all(y[:, ~any_voice] == 0.0)                                                               # no voice: exact zeros
        h.close()


@pytest.mark.parametrize("name", ["small8", "mid2"])
def test_any_partition_and_every_form_give_the_same_bits(name):
    import phaze_amd
    import torch
    k = case(name)
    x, tables, gains, mp, R = k["x"], k["tables"], k["gains"], k["mp"], k["R"]
    nv = len(tables)
    h = phaze_amd.Harmony(mp, R, max_voices=nv, max_channels=NCH, max_outputs=NOUT)
    rc, want, clean = _raw(h, x, tables, gains, 0, NOUT)
    assert rc == 0 and clean
    assert np.array_equal(h.process(x, tables, gains, 0, NOUT), want)                        # the binding, and a repeated call
    # splits at positions that are no multiple of the tile, with an empty call: the tiles of a call start at its first output
    cuts = [0, 0, 700, 701, 1900, 2947, NOUT]
    assert all(HM.check_span(tables, mp, R, a, b - a) is None for a, b in zip(cuts[:-1], cuts[1:]) if b > a)
    parts = [h.process(x, tables, gains, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts, axis=1), want)
    for c in range(NCH):                                                                     # a channel alone against the same channel among others
        assert np.array_equal(h.process(x[c], tables, gains[:, c], 0, NOUT), want[c])
    assert np.array_equal(_device(h, x, tables, gains, [0, NOUT]), want)                      # the device form in one call
    h.close()
    small = phaze_amd.Harmony(mp, R, max_voices=nv, max_channels=NCH, max_outputs=1)         # host pieces of one tile
    rc, y, clean = _raw(small, x, tables, gains, 0, NOUT, 3, 2, lead=1)
    assert rc == 0 and clean and np.array_equal(y, want)
    small.close()
    h = phaze_amd.Harmony(mp, R, max_channels=NCH)                                           # the defaults, the device form on a user stream, in pieces
    assert np.array_equal(h.process(x, tables, gains, 0, NOUT), want)
    assert np.array_equal(_device(h, x, tables, gains, cuts, stream=torch.cuda.Stream()), want)
    h.close()


def _hull_voices(distance):
    """Two voices at max_period 4096 whose displacements spread over 16000 samples each and lie `distance` samples apart."""
    rng = np.random.default_rng(404)
    t = np.arange(0, NOUT + 4000, 509)
    a = TGT._far_table(rng, t, rng.choice([2, 1000, 4096], t.size), 0.0, 0)
    b = TGT._far_table(rng, t + 100, rng.choice([2, 1000, 4096], t.size), 0.0, 0)
    swing = np.where(np.arange(t.size) % 2 == 0, 0, 16000)                   # every other grain reads 16000 samples further on
    a[:, 2] = -swing
    b[:, 2] = -swing - distance
    return [np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)]


def test_the_hull_near_the_span_runs_and_past_the_span_is_refused():
    """max_period 4096 at max_rate 1, span 25664: each voice alone reads about 17100 samples per tile; 8000 samples apart their hull is about 25100, and
    9000 apart it is past the span while each voice alone still fits."""
    import phaze_amd
    from phaze_amd import capi
    mp, R = 4096, 1
    nin = NOUT + 26000
    x = TGT._signals(nin, 5)[:2]
    gains = np.array([[0.75, -0.5], [0.5, 1.25]], np.float32)
    near = _hull_voices(8000)
    hull, _ = HM.tiles(near, mp, 0, NOUT)
    assert HM.check_voices(near, mp) is None and HM.check_span(near, mp, R, 0, NOUT) is None and 0.95 * TM.span(mp, R) < hull[:, 1].max() <= TM.span(mp, R)
    assert max(TM.tiles(v, mp, 0, NOUT)[:, 3].max() for v in near) < 0.7 * TM.span(mp, R)
    h = phaze_amd.Harmony(mp, R, max_voices=2, max_channels=2, max_outputs=NOUT)
    rc, y, clean = _raw(h, x, near, gains, 0, NOUT, 3, 2, lead=1)
    assert rc == 0 and clean, h._L.pv_harmony_last_error(h._h)
    P, H = phaze_amd.vari_prototype(), phaze_amd.psola_window()
    outs = [TM.process(x, t, 0, NOUT, P, H, bound=True) for t in near]
    assert np.array_equal(y, HM.mix(_per_voice(mp, R, x, near), [o[1][0] > 0 for o in outs], gains))
    ym, tol, poisoned = HM.process(x, near, gains, 0, NOUT, bound=True, outs=outs)
    assert not poisoned.any() and np.all(np.abs(y - ym) <= tol) and np.any(y != 0.0)
    far = _hull_voices(9000)
    tile, voice, grain, extent = HM.check_span(far, mp, R, 0, NOUT)
    assert extent > TM.span(mp, R) and all(TM.check_span(v, mp, R, 0, NOUT) is None for v in far)
    for fn in ("pv_harmony_process", "pv_harmony_process_device"):
        rc, y, clean = _raw(h, x, far, gains, 0, NOUT, fn=fn)
        msg = h._L.pv_harmony_last_error(h._h).decode()
        assert rc == capi.PV_ERR_ARGUMENT and f"tile {tile}:" in msg and f"voice {voice} grain {grain}:" in msg and str(extent) in msg and str(TM.span(mp, R)) in msg, msg
        assert clean and np.all(y == -77.0)                                  # every output byte still holds the fill
    for v in range(2):                                                       # each voice alone is accepted
        rc, y, clean = _raw(h, x, [far[v]], gains[v:v + 1], 0, NOUT)
        cov = TM.process(x[:1], far[v], 0, NOUT, P, H, bound=True)[1][0] > 0
        assert rc == 0 and clean and np.array_equal(y, HM.mix(_per_voice(mp, R, x, [far[v]]), [cov], gains[v:v + 1]))
    h.close()


def test_a_muted_voice_keeps_its_non_finite_samples_out_and_uncovered_outputs_are_zero():
    """Three voices on three channels at max_period 64, max_rate 4.  Voice 1 reads 3000 samples ahead of the others and is muted on channel 1 only; a NaN and
    an infinity lie where only voice 1 reads, in every channel.  Channel 1 stays finite everywhere, channels 0 and 2 are non-finite exactly where the model
    says.  No voice has a grain between outputs 1200 and 1500: exact zeros there."""
    import phaze_amd
    rng = np.random.default_rng(61)
    mp, R = 64, 4
    nin = NOUT + 3200
    keep = lambda t: t[(t < 1150) | (t > 1550)]
    tables = [np.ascontiguousarray(TGT._far_table(rng, keep(np.arange(v, NOUT + 40, stride)), 40, 0.0, 50), np.int32) for v, stride in enumerate((17, 23, 29))]
    tables[1][:, 2] -= 3000
    assert HM.check_voices(tables, mp) is None and HM.check_span(tables, mp, R, 0, NOUT) is None
    x = np.array(TGT._signals(nin, 13))
    x[:, 3700] = np.nan
    x[:, 5205] = np.inf
    x[0, 800] = -np.inf                                                      # and one under voices 0 and 2, in channel 0 only
    gains = np.array([[1.0, 0.5, -0.25], [0.5, 0.0, 0.75], [-1.0, 1.0, 0.5]], np.float32)
    y, tol, poisoned = HM.process(x, tables, gains, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
    assert poisoned[0].any() and poisoned[2].any() and not poisoned[1].any() and not poisoned.all()
    h = phaze_amd.Harmony(mp, R, max_voices=3, max_channels=3, max_outputs=1024)
    got = h.process(x, tables, gains, 0, NOUT)
    assert np.all(np.isfinite(got[1]))
    assert np.array_equal(~np.isfinite(got), poisoned), int(np.sum(~np.isfinite(got) != poisoned))
    ok = ~poisoned
    assert np.all(np.abs(got[ok] - y[ok]) <= tol[ok])
    assert np.all(got[:, 1200:1500] == 0.0) and not np.any(np.signbit(got[:, 1200:1500])) and np.all(tol[:, 1200:1500] == 3 * 2.0 ** -149)
    dev = _device(h, x, tables, gains, [0, 1300, NOUT])
    assert np.array_equal(np.isfinite(dev), ok) and np.array_equal(dev[ok], got[ok])
    # all gains zero: nothing is read, everything is zero
    assert not np.any(h.process(x, tables, np.zeros((3, 3), np.float32), 0, NOUT))
    h.close()


def test_refused_calls_leave_the_output_untouched_and_name_voice_and_grain():
    import phaze_amd
    from phaze_amd import capi
    k = case("small2")
    x, tables, mp, R = k["x"][:2], k["tables"], k["mp"], k["R"]
    gains = np.array(k["gains"][:, :2])
    h = phaze_amd.Harmony(mp, R, max_voices=2, max_channels=2, max_outputs=1024)

    def refused(tabs, word, xx=x, w=gains, rc=capi.PV_ERR_ARGUMENT, out_first=0, **kw):
        for fn in ("pv_harmony_process", "pv_harmony_process_device"):     # both forms check before any device work: host rows never reach the device
            got, y, clean = _raw(h, xx, tabs, w, out_first, NOUT, fn=fn, **kw)
            msg = h._L.pv_harmony_last_error(h._h).decode()
            assert got == rc and word in msg, (fn, got, msg)
            assert clean and np.all(y == -77.0)

    for voice in (0, 1):
        g = tables[voice]
        last = g.shape[0] - 1
        for idx, col, val in [(7, 3, 1), (7, 3, mp + 1), (0, 0, -1), (5, 0, 1 << 30), (9, 1, 65536), (9, 1, -1), (11, 2, 1 << 30), (11, 2, -(1 << 30)), (last, 0, 5),
                              (20, 0, int(g[19, 0]) - 1)]:
            bad = [np.array(t) for t in tables]
            bad[voice][idx, col] = val
            assert HM.check_voices(bad, mp)[:2] == (voice, idx)
            refused(bad, f"voice {voice} grain {idx}:")
        swapped = [np.array(t) for t in tables]
        swapped[voice][[30, 31]] = swapped[voice][[31, 30]]
        refused(swapped, f"voice {voice} grain 31:")
    # centres restart at a voice boundary: the second voice begins before the first one ends, and that is no error
    assert tables[1][0, 0] < tables[0][-1, 0]
    # a well-formed pair with a tile whose hull exceeds the span
    wide = [np.array(t) for t in tables]
    wide[1][:, 2] -= 3000
    assert HM.check_voices(wide, mp) is None and all(TM.check_span(t, mp, R, 0, NOUT) is None for t in wide)
    tile, voice, grain, extent = HM.check_span(wide, mp, R, 0, NOUT)
    refused(wide, f"tile {tile}: voice {voice} grain {grain}:")
    assert str(extent) in h._L.pv_harmony_last_error(h._h).decode() and "span" in h._L.pv_harmony_last_error(h._h).decode()
    # voice_first, the voice count and the gains
    n0, n1 = tables[0].shape[0], tables[1].shape[0]
    refused(tables, "voice_first[0]", first=[1, n0, n0 + n1])
    refused(tables, "voice_first[2]", first=[0, n0, n0 - 1])
    refused(tables, "voice_first[1]", first=[0, -1, n0 + n1])
    refused(tables, "null", first=[])
    refused(tables, "2^27", first=[0, n0, (1 << 27) + 1])
    refused(tables, "nvoices", nvoices=0)
    refused(tables, "nvoices", nvoices=-1)
    refused(tables, "max_voices", nvoices=3, first=[0, n0, n0 + n1, n0 + n1], w=np.ones((3, 2), np.float32), rc=capi.PV_ERR_CAPACITY)
    refused(tables, "max_channels", xx=k["x"], w=np.ones((2, 3), np.float32), rc=capi.PV_ERR_CAPACITY)
    refused(tables, "null", null_gains=True)
    for value in (np.nan, np.inf, -np.inf):
        w = np.array(gains)
        w[1, 0] = value
        refused(tables, "voice 1: its gain on channel 0", w=w)
    refused(tables, "2^30", out_first=(1 << 30) - 5)
    out = np.full(8, -77.0, np.float32)
    g, vf = _flat(tables)
    w1 = np.ones(2, np.float32)
    xp, gp, fp_, wp, op = x[0].ctypes.data_as(FP), g.ctypes.data_as(IP), vf.ctypes.data_as(LP), w1.ctypes.data_as(FP), out.ctypes.data_as(FP)
    for args in ((None, 100, 100, 1, gp, fp_, 2, wp, op, 0, 8, 8), (xp, 100, 100, 1, None, fp_, 2, wp, op, 0, 8, 8), (xp, 100, 100, 1, gp, fp_, 2, wp, None, 0, 8, 8),
                 (xp, -1, 100, 1, gp, fp_, 2, wp, op, 0, 8, 8), (xp, 100, 100, -1, gp, fp_, 2, wp, op, 0, 8, 8), (xp, 100, 100, 1, gp, fp_, 2, wp, op, -1, 8, 8),
                 (xp, 100, 100, 1, gp, fp_, 2, wp, op, 0, -8, 8), (x.ctypes.data_as(FP), 100, 99, 2, gp, fp_, 2, gains.ctypes.data_as(FP), op, 0, 4, 4),
                 (x.ctypes.data_as(FP), 100, 100, 2, gp, fp_, 2, gains.ctypes.data_as(FP), op, 0, 4, 3)):
        assert h._L.pv_harmony_process(h._h, *args) == capi.PV_ERR_ARGUMENT and np.all(out == -77.0), args[1:4]
    # the handle still works; a call without channels or outputs does nothing; an empty voice is legal
    none = np.zeros(3, np.int64)
    assert h._L.pv_harmony_process(h._h, None, 0, 0, 0, None, none.ctypes.data_as(LP), 2, None, None, 0, 0, 0) == 0
    assert np.array_equal(h.process(x, tables, gains, 5, 0), np.zeros((2, 0), np.float32))
    whole = h.process(x, tables, gains, 0, NOUT)
    assert np.all(np.abs(whole - k["y"][:2]) <= k["tol"][:2])
    lone = h.process(x, [tables[0], tables[1][:0]], gains, 0, NOUT)
    assert np.array_equal(lone, h.process(x, [tables[0][:0], tables[0]], gains[::-1], 0, NOUT))
    h.close()
    assert h._L.pv_harmony_destroy(None) == capi.PV_ERR_ARGUMENT


def test_process_tuned_is_the_hand_made_pipeline():
    """The two-formant voice of period 217.3 (221 Hz, a little sharp of A3) in C major at degrees (0, 2, 4), at rate 1 and at half speed: one f0 track,
    harmony_ratios, one tsm_plan per voice on the same row of rates, one call.  The tables, the length (voice 0's output_len) and the bits are the hand-made
    pipeline's, with the default gains 1 / V and with given ones."""
    import phaze_amd
    n = FM.PLAN_LEN
    x = np.stack([PM.voice(217.3, n), PM.voice(217.3, n, phase=0.3)])
    h = phaze_amd.Harmony(1024, 2, max_voices=3, max_channels=2)
    tracker = phaze_amd.F0Tracker(1024, 256, 32, 1024)
    recs = tracker.track(x[0], 2458)[0]
    tracker.close()
    nrec = recs.shape[0]
    assert np.all(recs[:, 0] > 0)
    ratios = phaze_amd.harmony_ratios(recs, FM.SAMPLE_RATE, (0, 2, 4), scale_mask=C_MAJOR)
    assert np.array_equal(ratios, HM.harmony_ratios(recs, FM.SAMPLE_RATE, (0, 2, 4), C_MAJOR))
    assert np.allclose(ratios[1] / ratios[0], 2.0 ** (3 / 12), rtol=1e-12) and np.allclose(ratios[2] / ratios[0], 2.0 ** (7 / 12), rtol=1e-12)
    for rate in (1.0, 0.5):
        plans = [phaze_amd.tsm_plan(recs, 256, 1024, n, 256.0, 32, 1024, ratios=ratios[v], rates=np.full(nrec, rate)) for v in range(3)]
        tables = [g for g, _ in plans]
        y, got_tables = h.process_tuned(x, FM.SAMPLE_RATE, scale_mask=C_MAJOR, rate=rate)
        assert len(got_tables) == 3 and all(np.array_equal(a, b) for a, b in zip(got_tables, tables))
        assert y.shape == (2, plans[0][1]) and abs(plans[0][1] - n / rate) <= 2 * 1024 - 3
        assert np.array_equal(y, h.process(x, tables, np.full(3, 1.0 / 3.0, np.float32), 0, plans[0][1]))
        w = np.array([[1.0, 0.5], [0.25, 0.0], [0.0, 0.75]], np.float32)
        y2, _ = h.process_tuned(x, FM.SAMPLE_RATE, degrees=(0, 2, 4), gains=w, scale_mask=C_MAJOR, rate=np.full(nrec, rate))
        assert np.array_equal(y2, h.process(x, tables, w, 0, plans[0][1])) and np.any(y2 != y)
    y1, t1 = h.process_tuned(x[0], FM.SAMPLE_RATE, degrees=(0,), gains=[1.0], scale_mask=C_MAJOR)          # one voice at gain 1: Tsm.process_tuned
    ts = phaze_amd.Tsm(1024, 2)
    yt, gt = ts.process_tuned(x[0], FM.SAMPLE_RATE, scale_mask=C_MAJOR)
    ts.close()
    assert np.array_equal(t1[0], gt) and np.array_equal(y1, yt)
    with pytest.raises(ValueError):
        h.process_tuned(x, FM.SAMPLE_RATE, rate=np.full(nrec - 1, 0.5))
    h.close()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_harmony_example_adds_a_third_and_a_fifth(tmp_path):
    import test_harmony_abi as THA
    exe = THA.build_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    print(j)
    assert abs(j["output_samples"] - j["samples"]) <= 2 * 1024 - 3 and all(g > 50 for g in j["grains"])
    assert abs(j["note_hz"][0] - 220.0) < 0.5 and abs(j["ratios"][1] / j["ratios"][0] - 2.0 ** (3 / 12)) < 1e-5 and abs(j["ratios"][2] / j["ratios"][0] - 2.0 ** (7 / 12)) < 1e-5
    assert j["level"][1] > 3.0 * j["level_in_at_third"]                      # the third is in the output and was not in the input
