"""Per-take plans on the overlap-add path (Takes / pv_takes_*) on the GPU: one call plays K independently planned takes of different lengths, and take k's
output is exactly Tsm.process on take k alone.

Expected values come from Tsm.process per take on a Tsm of the same (max_period, max_rate): an independent kernel that tests/test_gpu_tsm.py holds to
the numpy model.  The contract is one line, so every comparison here is ==: no tolerance anywhere, except that one case is also held within
tsm_model.process(bound=True)'s derived bound (tests/test_gpu_tsm.py's docstring, unchanged: the arithmetic per (output, grain, tap) is pv_tsm_kernel's
operation for operation), with no sample left out."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import f0_model as FM
import psola_model as PM
import takes_model as KM
import test_gpu_tsm as TGT
import test_takes_model as TKM
import tsm_model as TM

pytestmark = pytest.mark.gpu

TILE = KM.TILE
NOUT = TGT.NOUT
NCH = 3
FILL = -77.0
RAGGED = ("small", "tiny", "gap", "empty", "slow", "fast")
RAGGED_FIRSTS = [0, 517, 0, 1001, 517, 0]

_CACHE = {}


def ragged():
    """The six ragged takes on a (512, 4) configuration, computed once and never written: inputs of three channels, tables, first outputs, counts, and what
    Tsm(512, 4).process gives for each take alone."""
    if "ragged" not in _CACHE:
        tables = [TGT._grains(name)[3] for name in RAGGED]
        xs = [TGT._signals(TGT._grains(name)[2], 11 + k) for k, name in enumerate(RAGGED)]
        _CACHE["ragged"] = _expected(512, 4, xs, tables, list(RAGGED_FIRSTS), list(TKM.RAGGED_NOUTS))
    return _CACHE["ragged"]


def classes():
    """The fixture call of tests/test_takes_model.py on (4096, 1): tiles in all four occupancy classes."""
    if "classes" not in _CACHE:
        mp, R, nins, tables, firsts, nouts = TKM.class_fixture()
        xs = [TGT._signals(n, 23 + k) for k, n in enumerate(nins)]
        _CACHE["classes"] = _expected(mp, R, xs, tables, firsts, nouts)
    return _CACHE["classes"]


def _expected(mp, R, xs, tables, firsts, nouts):
    import phaze_amd
    assert KM.check_span(tables, mp, R, firsts, nouts) is None
    h = phaze_amd.Tsm(mp, R, max_channels=NCH)
    want = [h.process(x, g, f, n) for x, g, f, n in zip(xs, tables, firsts, nouts)]
    h.close()
    for a in xs + tables + want:
        a.setflags(write=False)
    return dict(mp=mp, R=R, xs=xs, tables=tables, firsts=firsts, nouts=nouts, want=want)


def layout(xs, tables, firsts, nouts, nch, pad_in=0, pad_out=0, lead=0):
    """(input buffers, output buffers, takes) of a call with one input and one output buffer per take: rows `lead` floats into their buffers (lead = 1: four
    bytes off any alignment), strides pad_in / pad_out longer than the rows, NaN around the input rows and the fill around the output rows.  A take is
    [input buffer, offset, nin, in_stride, grains, output buffer, offset, out_first, nout, out_stride], offsets in floats."""
    ins, outs, takes = [], [], []
    for k, (x, g, f, n) in enumerate(zip(xs, tables, firsts, nouts)):
        nin = x.shape[1]
        b = np.full(lead + nch * (nin + pad_in), np.nan, np.float32)
        b[lead:].reshape(nch, nin + pad_in)[:, :nin] = x[:nch]
        ins.append(b)
        outs.append(np.full(lead + nch * (n + pad_out) + 3, FILL, np.float32))
        takes.append([k, lead, nin, nin + pad_in, g, k, lead, f, n, n + pad_out])
    return ins, outs, takes


def _array(takes, in_ptrs, out_ptrs):
    from phaze_amd import capi
    arr = (capi._Take * max(len(takes), 1))()
    for k, (ib, io, nin, istride, g, ob, oo, f, n, ostride) in enumerate(takes):
        if isinstance(g, int):                                              # a count without a table
            gp, ng = None, g
        elif isinstance(g, tuple):                                          # a table and a count of its own (refused before the table is read)
            gp, ng = g[0].ctypes.data_as(C.POINTER(C.c_int32)), g[1]
        else:
            gp, ng = (g.ctypes.data_as(C.POINTER(C.c_int32)) if g.size else None), g.shape[0]
        arr[k] = capi._Take(in_ptrs[ib] + 4 * io if ib is not None else None, nin, istride, gp, ng, out_ptrs[ob] + 4 * oo if ob is not None else None, f, n, ostride)
    return arr


def call(h, ins, outs, takes, nch, device=False, ntakes=None):
    """One call through the raw C entry point: rc.  The device form works on copies of the buffers and brings the outputs back into `outs`."""
    if not device:
        arr = _array(takes, [b.ctypes.data for b in ins], [b.ctypes.data for b in outs])
        return h._L.pv_takes_process(h._h, arr, len(takes) if ntakes is None else ntakes, nch)
    import torch
    d_ins = [torch.from_numpy(b.copy()).cuda() for b in ins]
    d_outs = [torch.from_numpy(b.copy()).cuda() for b in outs]
    torch.cuda.synchronize()
    arr = _array(takes, [t.data_ptr() for t in d_ins], [t.data_ptr() for t in d_outs])
    rc = h._L.pv_takes_process_device(h._h, arr, len(takes) if ntakes is None else ntakes, nch)
    h.synchronize()
    for b, t in zip(outs, d_outs):
        b[:] = t.cpu().numpy()
    return rc


def rows(outs, takes, nch):
    """(the output rows of every take, whether everything around the rows still holds the fill)."""
    got, seen = [], [np.zeros(b.shape, bool) for b in outs]
    for ib, io, nin, istride, g, ob, oo, f, n, ostride in takes:
        idx = oo + (np.arange(nch)[:, None] * ostride + np.arange(n)[None, :] if n > 0 else np.zeros((nch, 0), np.int64))
        got.append(outs[ob][idx])
        seen[ob][idx] = True
    return got, all(bool(np.all(b[~s] == FILL)) for b, s in zip(outs, seen))


def same(got, want, nch):
    return all(a.dtype == np.float32 and a.shape == w[:nch].shape and np.array_equal(a, w[:nch]) and not np.any(np.signbit(a) & (a == 0) & ~np.signbit(w[:nch]))
               for a, w in zip(got, want))


def run(h, k, nch, device=False, pads=(0, 0), lead=0, pick=None):
    """The case k (all its takes, or the takes `pick` in that order) through one call: (rc, rows, clean, what Tsm.process gave for them)."""
    pick = list(range(len(k["xs"]))) if pick is None else pick
    sel = {key: [k[key][i] for i in pick] for key in ("xs", "tables", "firsts", "nouts", "want")}
    ins, outs, takes = layout(sel["xs"], sel["tables"], sel["firsts"], sel["nouts"], nch, *pads, lead=lead)
    rc = call(h, ins, outs, takes, nch, device)
    got, clean = rows(outs, takes, nch)
    return rc, got, clean, sel["want"]


# ---- bits --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nch,pads,lead", [(1, (0, 0), 0), (3, (5, 129), 1)])
def test_every_take_of_a_ragged_call_has_the_bits_of_tsm_process(nch, pads, lead):
    import phaze_amd
    k = ragged()
    assert [w.shape for w in k["want"]] == [(NCH, n) for n in TKM.RAGGED_NOUTS] and any(np.any(w != 0) for w in k["want"])
    h = phaze_amd.Takes(512, 4, max_channels=nch)
    rc, got, clean, want = run(h, k, nch, pads=pads, lead=lead)
    assert rc == 0, h._L.pv_takes_last_error(h._h)
    assert clean and same(got, want, nch), [int(np.sum(a != w[:nch])) for a, w in zip(got, want)]
    # the binding
    ys = h.process([x[:nch] for x in k["xs"]], k["tables"], k["firsts"], k["nouts"])
    assert same(ys, want, nch)
    ys = h.process([x[0] for x in k["xs"]], k["tables"], k["firsts"], k["nouts"])
    assert all(y.ndim == 1 and np.array_equal(y, w[0]) for y, w in zip(ys, want))
    h.close()


@pytest.mark.parametrize("nch,pads,lead", [(1, (0, 0), 0), (3, (5, 129), 1)])
def test_a_call_with_tiles_in_every_occupancy_class_has_the_bits_of_tsm_process(nch, pads, lead):
    """Four launches, one per class: the widest tile reads more than 11072 samples, the narrowest fewer than 960."""
    import phaze_amd
    k = classes()
    t = phaze_amd.takes_tiles(k["mp"], k["R"], k["tables"], k["firsts"], k["nouts"])
    assert set(t[:, 6].tolist()) == {1, 2, 3, 4}
    for device in (False, True):
        h = phaze_amd.Takes(4096, 1, max_channels=nch)
        rc, got, clean, want = run(h, k, nch, device=device, pads=pads, lead=lead)
        assert rc == 0, h._L.pv_takes_last_error(h._h)
        assert clean and same(got, want, nch), (device, [int(np.sum(a != w[:nch])) for a, w in zip(got, want)])
        h.close()


@pytest.mark.parametrize("slack", [4, 0])
def test_the_widest_tile_of_the_largest_configuration_runs_beside_narrow_ones(slack):
    """(3641, 2) has the span 31240, no multiple of 64 and within 63 samples of the largest count that fits the LDS: a tile that reads 31236 (31240) samples
    cannot be staged rounded up to 64, so its launch stages the count itself (tests/takes_model.py launch_span).  Its two grains cover disjoint outputs, so
    the take is the sum of two Tsm.process calls with one grain each, whose tiles are narrow; also held to the model's bound.  A ragged take beside it."""
    import phaze_amd
    mp, R = 3641, 2
    g, cap = TKM.widest_tile_table(mp, R, slack)
    assert cap == 31240 - slack and KM.cls(cap) == 1 and KM.launch_span(cap) == cap and KM.lds_bytes((cap + 63) & ~63) > TM.LDS_BYTES
    k = ragged()
    xs = [TGT._signals(32000, 41), k["xs"][0]]
    tables, firsts, nouts = [g, k["tables"][0]], [0, 0], [1024, NOUT]
    t = phaze_amd.takes_tiles(mp, R, tables, firsts, nouts)
    assert t[0].tolist() == [0, 0, 0, 2, 65, cap, 1, 0] and set(t[1:, 6].tolist()) == {3, 4}
    tsm = phaze_amd.Tsm(mp, R, max_channels=NCH)
    parts = [tsm.process(xs[0], g[j:j + 1], 0, 1024) for j in range(2)]
    want = [parts[0] + parts[1], tsm.process(xs[1], tables[1], 0, NOUT)]
    tsm.close()
    assert np.all(parts[0][:, 200:] == 0) and np.all(parts[1][:, :800] == 0) and np.any(parts[0] != 0) and np.any(parts[1] != 0)
    model, tol, poisoned = TM.process(xs[0], g, 0, 1024, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
    for device in (False, True):
        h = phaze_amd.Takes(mp, R, max_channels=NCH)
        ins, outs, takes = layout(xs, tables, firsts, nouts, NCH, 3, 2, lead=1)
        rc = call(h, ins, outs, takes, NCH, device)
        assert rc == 0, h._L.pv_takes_last_error(h._h)
        got, clean = rows(outs, takes, NCH)
        h.close()
        assert clean and same(got, want, NCH), (device, [int(np.sum(a != w)) for a, w in zip(got, want)])
        assert np.all(np.abs(got[0].astype(np.float64) - model) <= tol) and np.all(got[0][tol == 0] == 0)


def test_a_ragged_call_is_within_the_derived_bound_of_the_model():
    """tests/test_gpu_tsm.py's bound, every sample of every take and channel; an output no grain covers is exactly +0."""
    import phaze_amd
    k = ragged()
    h = phaze_amd.Takes(512, 4, max_channels=NCH)
    rc, got, clean, _ = run(h, k, NCH, pads=(5, 129), lead=1)
    h.close()
    assert rc == 0 and clean
    P, Hn = phaze_amd.vari_prototype(), phaze_amd.psola_window()
    worst = 0.0
    for name, x, g, f, n, y in zip(RAGGED, k["xs"], k["tables"], k["firsts"], k["nouts"], got):
        want, tol, poisoned = TM.process(x, g, f, n, P, Hn, bound=True)
        assert not poisoned.any()
        err = np.abs(y.astype(np.float64) - want)
        live = tol > 0
        if live.any():
            worst = max(worst, float(np.max(err[live] / tol[live])))
        assert np.all(err <= tol), (name, int(np.sum(err > tol)))
        assert np.all(y[~live] == 0.0) and not np.any(np.signbit(y[~live]))
    print(f"worst |err| / bound = {worst:.3f}")


# ---- forms -------------------------------------------------------------------------------------------------------------------------------------

def test_every_form_gives_the_same_bits():
    import phaze_amd
    import torch
    k = ragged()
    # the device form on the handle's stream, then on a user stream, then a repeated call
    h = phaze_amd.Takes(512, 4, max_channels=NCH)
    rc, got, clean, want = run(h, k, NCH, device=True, pads=(7, 5), lead=1)
    assert rc == 0 and clean and same(got, want, NCH)
    stream = torch.cuda.Stream()
    h.set_stream(stream.cuda_stream)
    rc, got, clean, want = run(h, k, NCH, device=True, pads=(7, 5), lead=1)
    assert rc == 0 and clean and same(got, want, NCH)
    h.set_stream(None)
    for _ in range(2):
        rc, got, clean, want = run(h, k, NCH, pads=(3, 2))
        assert rc == 0 and clean and same(got, want, NCH)
    # the takes in reversed order, and every take alone
    pick = list(range(6))[::-1]
    rc, got, clean, want = run(h, k, NCH, pick=pick)
    assert rc == 0 and clean and same(got, want, NCH)
    rc, got, clean, want = run(h, k, NCH, device=True, pick=pick)
    assert rc == 0 and clean and same(got, want, NCH)
    for i in range(6):
        rc, got, clean, want = run(h, k, NCH, pick=[i])
        assert rc == 0 and clean and same(got, want, NCH), i
    h.close()
    # host pieces of one tile, on both configurations
    for case, cfg in ((k, (512, 4)), (classes(), (4096, 1))):
        small = phaze_amd.Takes(*cfg, max_channels=NCH, max_outputs=1024)
        rc, got, clean, want = run(small, case, NCH, pads=(3, 2), lead=1)
        assert rc == 0 and clean and same(got, want, NCH)
        small.close()
    # pieces of three tiles: a piece ends inside a take and the next begins there
    three = phaze_amd.Takes(512, 4, max_channels=NCH, max_outputs=3 * TILE)
    rc, got, clean, want = run(three, k, NCH)
    assert rc == 0 and clean and same(got, want, NCH)
    three.close()


@pytest.mark.parametrize("cut", [700, 2048])
def test_a_take_split_into_two_takes_gives_the_bits_of_one(cut):
    """[0, cut) and [cut, n) share the input and write adjacent outputs of the same rows: the tiles differ unless the cut is a multiple of 1024, the bits do
    not."""
    import phaze_amd
    k = ragged()
    x, g, want = k["xs"][0], k["tables"][0], k["want"][0]
    n = want.shape[1]
    ins, outs, takes = layout([x], [g], [0], [n], NCH, 4, 9, lead=1)
    ib, io, nin, istride, _, ob, oo, _, _, ostride = takes[0]
    two = [[ib, io, nin, istride, g, ob, oo, 0, cut, ostride], [ib, io, nin, istride, g, ob, oo + cut, cut, n - cut, ostride]]
    for device in (False, True):
        h = phaze_amd.Takes(512, 4, max_channels=NCH)
        outs[0][:] = FILL
        assert call(h, ins, outs, two, NCH, device) == 0, h._L.pv_takes_last_error(h._h)
        got, clean = rows(outs, takes, NCH)
        assert clean and np.array_equal(got[0], want), (device, int(np.sum(got[0] != want)))
        h.close()


def test_two_takes_may_share_an_input():
    """Two plans on one recording: a double-track."""
    import phaze_amd
    k = ragged()
    x = k["xs"][0]                                                          # small's input, 4 n samples: gap's table reads the same range
    tables = [k["tables"][0], k["tables"][2]]
    tsm = phaze_amd.Tsm(512, 4, max_channels=NCH)
    want = [tsm.process(x, g, 0, NOUT) for g in tables]
    tsm.close()
    assert not np.array_equal(want[0], want[1])
    ins, outs, takes = layout([x, x], tables, [0, 0], [NOUT, NOUT], NCH, 2, 3)
    takes[1][0] = 0                                                         # the second take reads the first take's buffer
    ins[1][:] = np.nan
    for device in (False, True):
        h = phaze_amd.Takes(512, 4, max_channels=NCH)
        for b in outs:
            b[:] = FILL
        assert call(h, ins, outs, takes, NCH, device) == 0
        got, clean = rows(outs, takes, NCH)
        assert clean and same(got, want, NCH)
        h.close()


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_non_finite_sample_changes_its_own_take_only(value):
    """A non-finite sample in take 1's input reaches exactly the outputs of take 1 the model says, and no output of any other take changes a bit."""
    import phaze_amd
    k = ragged()
    pick = [0, 4, 2]                                                        # small, slow, gap, each from its own first output
    xs = [np.array(k["xs"][i]) for i in pick]
    tables, firsts = [k["tables"][i] for i in pick], [k["firsts"][i] for i in pick]
    nouts = [NOUT, 1500, NOUT]
    g = tables[1]
    for j, c in ((g.shape[0] // 2, 0), (g.shape[0] // 3, 1), (5, 2)):
        t, w, D, L = (int(v) for v in g[j])
        xs[1][c, min(max(t - L + 1 - D - 32, 0), xs[1].shape[1] - 1)] = value
        xs[1][c, min(max(t - D, 0), xs[1].shape[1] - 1)] = -value if value == value else value
    _, _, poisoned = TM.process(xs[1], g, firsts[1], nouts[1], phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
    assert poisoned.any() and not poisoned.all()
    tsm = phaze_amd.Tsm(512, 4, max_channels=NCH)
    want = [tsm.process(x, t, f, n) for x, t, f, n in zip(xs, tables, firsts, nouts)]
    clean_want = tsm.process(k["xs"][4], g, firsts[1], nouts[1])
    tsm.close()
    for device in (False, True):
        h = phaze_amd.Takes(512, 4, max_channels=NCH)
        ins, outs, takes = layout(xs, tables, firsts, nouts, NCH, 1, 1)
        assert call(h, ins, outs, takes, NCH, device) == 0
        got, clean = rows(outs, takes, NCH)
        h.close()
        assert clean and np.array_equal(~np.isfinite(got[1]), poisoned)
        assert np.array_equal(got[1][~poisoned], clean_want[~poisoned])      # take 1 changes exactly where the model says
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[2]))
        assert np.array_equal(got[1], want[1], equal_nan=True)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_leave_every_output_untouched_and_name_the_take():
    import phaze_amd
    from phaze_amd import capi
    k = ragged()
    h = phaze_amd.Takes(512, 4, max_channels=2, max_outputs=1024)
    bad = capi.PV_ERR_ARGUMENT

    def refused(word, nch=2, rc_want=bad, ntakes=None, **change):
        """Both forms, with `change`: take index -> {position in the take: value}, applied to the takes of the ragged call."""
        for device in (False, True):
            ins, outs, takes = layout(k["xs"], k["tables"], k["firsts"], k["nouts"], max(nch, 1), 2, 3)
            for i, fields in change.items():
                for pos, val in fields.items():
                    takes[int(i[1:])][pos] = val
            rc = call(h, ins, outs, takes, nch, device, ntakes=ntakes)
            msg = h._L.pv_takes_last_error(h._h).decode()
            assert rc == rc_want and word in msg, (device, rc, msg)
            assert all(np.all(b == FILL) for b in outs), (word, device)       # every output byte of every take still holds the fill

    small, fast = k["tables"][0], k["tables"][5]
    # a bad grain in the first, a middle and the last take (the last take has no outputs: its table is validated all the same)
    for i, g in ((0, small), (2, k["tables"][2]), (5, fast)):
        for idx, col, val in [(7, 3, 1), (7, 3, 513), (0, 0, -1), (9, 1, 65536), (11, 2, 1 << 30), (g.shape[0] - 1, 0, 5)]:
            b = np.array(g)
            b[idx, col] = val
            refused(f"take {i}: grain {idx}:", **{f"t{i}": {4: b}})
    wide = np.array(k["tables"][2])
    wide[3, 2] = -((1 << 30) - 1)
    tile, first, extent = TM.check_span(wide, 512, 4, 0, 1023)
    refused(f"take 2: grain {first}:", t2={4: wide})
    assert "span" in h._L.pv_takes_last_error(h._h).decode() and str(extent) in h._L.pv_takes_last_error(h._h).decode()
    # counts, ranges, buffers, strides
    refused("take 3", t3={2: -1})
    refused("take 4", t4={8: -1})
    refused("take 1", t1={7: -1})
    refused("2^30", t0={7: (1 << 30) - 5})
    # the sums over the takes, refused on the counts before any buffer or table is read
    refused("take 1: the takes' outputs together reach 2^30", t0={8: 1 << 29}, t1={8: 1 << 29})
    refused("take 5: the takes' outputs together reach 2^30", t0={8: 1 << 29}, t5={8: (1 << 29) - sum(k["nouts"][1:])})     # exactly 2^30
    refused("take 2: more than 2^27 grains in one call", t0={4: (small, (1 << 26) + 1)}, t2={4: (small, (1 << 26) + 1)})
    refused("take 3: more than 2^27 grains", t3={4: (small, (1 << 27) + 1)})
    refused("take 1: null buffer", t1={0: None})
    refused("take 4: null buffer", t4={5: None})
    refused("take 0: null grains", t0={4: 3})
    refused("take 0: channel strides", t0={3: 100})
    refused("take 2: channel strides", t2={9: 1022})
    refused("negative channel", nch=-1)
    refused("max_channels", nch=3, rc_want=capi.PV_ERR_CAPACITY)
    refused("takes", ntakes=-1)
    refused("65536", ntakes=65537)
    # overlapping output rows: take 4 writes into take 0's rows, at the very end of them and across two channels
    n0 = k["nouts"][0]
    refused("take 0 and take 4: their output rows overlap", t4={5: 0, 6: n0 - 1})
    refused("take 0 and take 4: their output rows overlap", t4={5: 0, 6: n0 + 3 - 500})
    refused("take 2 and take 5: their output rows overlap", t5={5: 2, 6: 100, 8: 10, 9: 10})
    for fn in ("pv_takes_process", "pv_takes_process_device"):
        assert getattr(h._L, fn)(h._h, None, 3, 1) == bad and "null takes" in h._L.pv_takes_last_error(h._h).decode()
    # adjacent rows are no overlap; the handle still works; calls without takes, channels or outputs do nothing
    ins, outs, takes = layout(k["xs"], k["tables"], k["firsts"], k["nouts"], 2, 2, 3)
    takes[4][5], takes[4][6] = 0, 2 * (n0 + 3)                              # right behind take 0's second row
    outs[0] = np.concatenate([outs[0][:2 * (n0 + 3)], np.full(2 * (k["nouts"][4] + 3), FILL, np.float32)])
    assert call(h, ins, outs, takes, 2) == 0, h._L.pv_takes_last_error(h._h)
    got, clean = rows(outs, takes, 2)
    assert clean and same(got, k["want"], 2)
    assert h._L.pv_takes_process(h._h, None, 0, 1) == 0 and h._L.pv_takes_process_device(h._h, None, 0, 2) == 0
    ins, outs, takes = layout(k["xs"], k["tables"], k["firsts"], [0] * 6, 2)
    assert call(h, ins, outs, takes, 2) == 0 and call(h, ins, outs, takes, 0) == 0 and all(np.all(b == FILL) for b in outs)
    assert h.process([], []) == []
    h.close()
    assert h._L.pv_takes_destroy(None) == bad


# ---- process_tuned and the example -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("epochs", [False, True])
def test_process_tuned_is_tsm_process_tuned_per_take(epochs):
    """Three voice-like takes of different lengths and pitches at the rates 1, 1/2 and 2, tracked in one call of three channels: the tables and the outputs
    are those of Tsm.process_tuned on each take alone."""
    import phaze_amd
    spec = ((452.0, 12000, 1.0), (223.0, 9000, 0.5), (331.0, 15000, 2.0))
    xs = [np.stack([PM.voice(FM.SAMPLE_RATE / f, n), PM.voice(FM.SAMPLE_RATE / f, n, phase=0.3)]) for f, n, _ in spec]
    rates = [r for _, _, r in spec]
    h = phaze_amd.Takes(1024, 2, max_channels=2)
    ys, tables = h.process_tuned(xs, FM.SAMPLE_RATE, rate=rates, epochs=epochs)
    tsm = phaze_amd.Tsm(1024, 2, max_channels=2)
    for k, (x, r) in enumerate(zip(xs, rates)):
        y, g = tsm.process_tuned(x, FM.SAMPLE_RATE, rate=r, epochs=epochs)
        assert g.shape[0] > 20 and np.array_equal(tables[k], g), k
        assert ys[k].shape == y.shape and np.array_equal(ys[k], y), (k, int(np.sum(ys[k] != y)))
        assert abs(y.shape[1] - x.shape[1] / r) <= 2 * 1024 - 3
    # one number for all takes, a row per record for one of them, one-dimensional takes
    ys1, t1 = h.process_tuned([x[0] for x in xs], FM.SAMPLE_RATE, rate=0.5, epochs=epochs)
    y, g = tsm.process_tuned(xs[2][0], FM.SAMPLE_RATE, rate=0.5, epochs=epochs)
    assert ys1[2].ndim == 1 and np.array_equal(ys1[2], y) and np.array_equal(t1[2], g)
    nrec = (xs[1].shape[1] - 2048) // 256 + 1
    ys2, t2 = h.process_tuned(xs, FM.SAMPLE_RATE, rate=[1.0, np.full(nrec, 0.5), 2.0], epochs=epochs)
    assert all(np.array_equal(a, b) for a, b in zip(ys2, ys)) and all(np.array_equal(a, b) for a, b in zip(t2, tables))
    # a take with no whole f0 frame (shorter than window + max_lag = 2048) beside the others: no records, the unvoiced grains, as alone
    short = np.ascontiguousarray(xs[0][:, :1500])
    ys3, t3 = h.process_tuned([xs[1], short, xs[2]], FM.SAMPLE_RATE, rate=[0.5, 0.5, 2.0], epochs=epochs)
    y, g = tsm.process_tuned(short, FM.SAMPLE_RATE, rate=0.5, epochs=epochs)
    assert g.shape[0] > 3 and np.array_equal(t3[1], g) and ys3[1].shape == y.shape and np.array_equal(ys3[1], y) and np.any(y != 0)
    assert np.array_equal(ys3[0], ys[1]) and np.array_equal(ys3[2], ys[2])
    with pytest.raises(ValueError):
        h.process_tuned(xs, FM.SAMPLE_RATE, rate=[1.0, 2.0])
    with pytest.raises(ValueError):
        h.process_tuned(xs, FM.SAMPLE_RATE, rate=[1.0, np.full(nrec - 1, 0.5), 2.0])
    assert h.process_tuned([], FM.SAMPLE_RATE) == ([], [])
    tsm.close()
    h.close()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_takes_example_plays_three_takes_in_one_call(tmp_path):
    import test_takes_abi as TTA
    exe = TTA.build_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert lines[-1] == "one_call_equals_three_tsm_calls 1" and len(lines) == 4
    for k, (line, hz, speed, target) in enumerate(zip(lines, (452.0, 223.0, 331.0), (1.0, 0.5, 2.0), (69, 57, 64))):
        w = line.split()
        f = dict(zip(w[0::2], w[1::2]))
        assert int(f["take"]) == k and float(f["frequency"]) == hz and float(f["rate"]) == speed and float(f["target"]) == target
        assert abs(int(f["output"]) - int(f["samples"]) / speed) <= 2 * 1024 - 3
        assert abs(float(f["note"]) - target) < 0.01, line
