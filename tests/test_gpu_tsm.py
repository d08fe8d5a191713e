"""The time-scale modification kernel (Tsm / pv_tsm_*) on the GPU against the numpy model (tests/tsm_model.py), bit equality with Psola.process on tables
that read near where they write, and partition invariance.

Tolerance against the model: the DERIVED bound of tests/test_gpu_psola.py's docstring, unchanged.  The kernel's arithmetic per (output, grain, tap) is
pv_psola_kernel's operation for operation; the displacement D of a far grain enters the addresses only, never a rounded value.  So with u = 2^-24, per
grain with a fractional displacement |xt^ - xt| <= e_g = u [64 (a_g + |xt| s_g) / |d_g| + |xt|] (64 fused multiply-adds, 64 additions, one division; 0
for a whole-sample displacement), the window weight is within 3 u m of h with m = |h| + |f d|, and with G grains covering an output
    |y_gpu - y| <= [ (G + 3) u (A + |y| S) + E ] / D + u |y|,   A = sum m_g |xt_g|, S = sum m_g, D = sum h_g, E = sum |h_g| e_g,
times 1 + 2^-10 for the second order, plus 2^-149 (1 + (G + 67) / D) for an intermediate in the subnormal range: tsm_model.process(bound=True)
restates it for the same arithmetic.  No sample is left out; an output no grain covers must be exactly 0.  Everything else is bit for bit.
Worst observed |err| / bound over all cases: 0.23 (the plan at half speed, three channels; one MI355X)."""
import ctypes as C
import json
import shutil
import subprocess

import numpy as np
import pytest

import f0_model as FM
import psola_model as PM
import tsm_model as TM

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int32)
TILE = 1024
NOUT = 3 * TILE + 37
NCH = 3


def _far_table(rng, t, L, slope, jitter):
    """Grains at the centres t (random fractions of either kind, a fifth of them whole-sample) that read the input at about (1 + slope) n."""
    t = np.asarray(t, np.int64)
    tf, phi = rng.integers(0, 256, t.size), rng.integers(0, 256, t.size)
    phi[::5] = 0
    phi[1::7] = 1
    phi[2::7] = 255
    tf[3::11] = 0
    tf[4::11] = 255
    D = -np.floor(slope * t).astype(np.int64) + rng.integers(-jitter, jitter + 1, t.size)
    return np.stack([t, tf + 256 * phi, D, np.broadcast_to(L, t.shape)], axis=1)


def _grains(name):
    """(max_period, max_rate, nin, far grains int32[., 4]).  A tile holds 1024 outputs: every table spans three tiles and 37 outputs."""
    rng = np.random.default_rng(len(name) * 137 + ord(name[0]))
    n = NOUT
    if name == "small":                # max_period 64 at max_rate 4: a grain every 19 outputs reading at four times the output position
        mp, R, nin = 64, 4, 4 * n
        t = np.arange(0, n + 60, 19)
        g = _far_table(rng, t, rng.integers(2, 65, t.size), 3.0, 60)
        g[:3, 3] = [64, 2, 64]
    elif name == "mid":                # max_period 1024 at max_rate 4: about 105 KB of LDS were it sized by the capacity
        mp, R, nin = 1024, 4, 4 * n
        t = np.arange(0, n + 1000, 211)
        g = _far_table(rng, t, rng.choice([2, 300, 1024], t.size), 3.0, 1000)
    elif name == "big":                # max_period 4096 at max_rate 1, the largest span: displacements spread over 16000 samples
        mp, R, nin = 4096, 1, n + 9000
        t = np.arange(0, n + 4000, 509)
        g = _far_table(rng, t, rng.choice([2, 1000, 4096], t.size), 0.0, 8000)
        g[:, 2] -= 8000
    elif name == "tiny":               # L = 2 .. 8, a grain every two or three samples: hundreds per tile, two thousand samples from where they write
        mp, R, nin = 8, 1, n + 2100
        t = np.cumsum(rng.integers(1, 4, 1400)) - 5
        t = t[(t >= 0) & (t < n + 6)]
        g = _far_table(rng, t, rng.integers(2, 9, t.size), 0.0, 7)
        g[:, 2] -= 2000
    elif name == "huge":               # L = max_period = 4096: every grain spans every tile and hangs over both ends of the input
        mp, R, nin = 4096, 1, n
        g = np.array([[0, 0, 0, 4096], [700, 255 + 256 * 255, -4096, 4096], [1500, 0, 4096, 4096], [1500, 256 * 255, 4095, 4096], [1600, 255 + 256, -8000, 4096],
                      [2900, 17 + 256 * 128, 7000, 4096], [n - 1, 128 + 256 * 253, -1, 4096], [n + 4000, 0, 4000, 4096]])
    elif name == "sweep":              # D runs from +3 tiles to -3 tiles: the first outputs read before the input, the last ones past its end: exact zeros
        mp, R, nin = 64, 4, n
        t = np.arange(0, n + 40, 31)
        g = _far_table(rng, t, 40, 0.0, 0)
        g[:, 2] = 3 * TILE - (6 * TILE * t) // n
    elif name == "gap":                # nothing between 950 and 2250: outputs 990 .. 2209 and the whole second tile are uncovered
        mp, R, nin = 64, 4, 4 * n
        t = np.concatenate([np.arange(3, 951, 19), np.arange(2250, n, 23)])
        g = _far_table(rng, t, 40, 3.0, 60)
        g[t == 3 + 19 * 49, 1] &= ~255                                        # the last grain before the gap ends at a whole sample
    elif name == "empty":
        mp, R, nin, g = 512, 2, n, np.zeros((0, 4), np.int64)
    elif name == "slow":               # a planned table at half speed: every analysis mark serves two grains; period 217.3 moved by 1.25, then unvoiced
        mp, R, nin = 512, 2, 1600
        recs = PM.records_of([217.3] * 15 + [-60.0] * 10)
        g, nout = TM.tsm_plan(recs, 64, 32, nin, 128.0, 32, mp, ratios=np.full(25, 1.25), rates=np.full(25, 0.5))
        assert nout >= n and np.all(np.bincount((g[:, 0] - g[:, 2])[g[:, 1] < 256] // 128)[14:24] == 2)
    elif name == "fast":               # a planned table at four times the speed
        mp, R, nin = 512, 4, 4 * n + 64
        recs = PM.records_of([217.3] * 120 + [-60.0] * 76)
        g, nout = TM.tsm_plan(recs, 64, 32, nin, 128.0, 32, mp, ratios=np.full(196, 0.8), rates=np.full(196, 4.0))
        assert nout >= n
    else:
        raise KeyError(name)
    g = np.ascontiguousarray(g, np.int32).reshape(-1, 4)
    assert TM.check_grains(g, mp) is None, TM.check_grains(g, mp)
    assert TM.check_span(g, mp, R, 0, NOUT) is None, (TM.check_span(g, mp, R, 0, NOUT), TM.span(mp, R))
    assert name in ("empty",) or not TM.is_near(g, mp)
    return mp, R, nin, g


CASES = ["small", "mid", "big", "tiny", "huge", "sweep", "gap", "empty", "slow", "fast"]


def _signals(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = np.zeros((NCH, n))
    x[0] = rng.standard_normal(n)
    x[1] = 0.5 * np.cos(0.05 * t + 1.0) + 0.3 * np.cos(1.3 * t) + 0.2 * np.cos(2.9 * t + 2.0)
    x[2] = np.where((t // 37) % 2 == 0, 1.0, -1.0)
    return x.astype(np.float32)


_CACHE = {}


def case(name):
    """Shared per table, computed once and never written: the input, the grains, the model's output on the library's tables and its bound."""
    if name not in _CACHE:
        import phaze_amd
        mp, R, nin, g = _grains(name)
        x = _signals(nin, 7 + len(name))
        y, tol, poisoned = TM.process(x, g, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
        assert not poisoned.any()
        for a in (x, g, y, tol):
            a.setflags(write=False)
        _CACHE[name] = dict(mp=mp, R=R, n=nin, g=g, x=x, y=y, tol=tol)
    return _CACHE[name]


def _raw(h, x, g, out_first, nout, pad_in=0, pad_out=0, lead=0, fn="pv_tsm_process"):
    """One host call through the raw C entry point: rows `lead` floats into their buffers (lead = 1: four bytes off any alignment) and strides longer than the
    rows.  Returns (rc, out rows, whether everything around the rows still holds the fill)."""
    nch, nin = x.shape
    xin = np.full(lead + nch * (nin + pad_in), np.nan, np.float32)
    rows = xin[lead:].reshape(nch, nin + pad_in)
    rows[:, :nin] = x
    out = np.full(lead + nch * (nout + pad_out) + 3, -77.0, np.float32)
    orow = out[lead:lead + nch * (nout + pad_out)].reshape(nch, nout + pad_out)
    gp = g.ctypes.data_as(IP) if g.size else None
    rc = getattr(h._L, fn)(h._h, rows.ctypes.data_as(FP), nin, nin + pad_in, nch, gp, g.shape[0], orow.ctypes.data_as(FP), out_first, nout, nout + pad_out)
    clean = bool(np.all(orow[:, nout:] == -77.0) and np.all(out[:lead] == -77.0) and np.all(out[lead + nch * (nout + pad_out):] == -77.0))
    return rc, orow[:, :nout].copy(), clean


def _device(h, x, g, cuts, stream=None):
    """The device form in the calls `cuts`, padded strides, rows four bytes off their alignment; checks that nothing around the rows was written."""
    import torch
    nch, n = x.shape
    if stream is not None:
        h.set_stream(stream.cuda_stream)
    d_in = torch.full((nch * (n + 7) + 1,), float("nan"), dtype=torch.float32, device="cuda")
    d_in[1:].view(nch, n + 7)[:, :n] = torch.from_numpy(x.copy()).cuda()
    d_out = torch.full((nch * (NOUT + 5) + 1,), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert (d_in.data_ptr() + 4) % 16 == 4
    for a, b in zip(cuts[:-1], cuts[1:]):
        h.process_device(d_in.data_ptr() + 4, n, n + 7, nch, g, d_out.data_ptr() + 4 + 4 * a, a, b - a, NOUT + 5)
    h.synchronize()
    if stream is not None:
        h.set_stream(None)
    got = d_out.cpu().numpy()
    assert got[0] == -77.0 and np.all(got[1:].reshape(nch, NOUT + 5)[:, NOUT:] == -77.0)
    return got[1:].reshape(nch, NOUT + 5)[:, :NOUT].copy()


@pytest.mark.parametrize("name", CASES)
def test_every_sample_is_within_the_derived_bound_of_the_model(name):
    import phaze_amd
    k = case(name)
    covered = k["tol"][0] > 0
    if name == "gap":
        assert not covered[975:2210].any() and covered[:974].all() and covered[2212:].all() and not covered[TILE:2 * TILE].any()
    if name == "empty":
        assert not covered.any()
    if name == "sweep":                # the first and the last outputs read outside the input: covered, and exactly zero in the model too
        assert covered[:900].all() and covered[-900:].all() and np.all(k["y"][:, :900] == 0.0) and np.all(k["y"][:, -900:] == 0.0) and np.any(k["y"][:, 1200:1900] != 0.0)
    for nch, pads, lead in ((1, (0, 0), 0), (3, (5, 129), 1)):
        h = phaze_amd.Tsm(k["mp"], k["R"], max_channels=nch, max_outputs=NOUT)
        rc, y, clean = _raw(h, k["x"][:nch], k["g"], 0, NOUT, *pads, lead=lead)
        assert rc == 0 and clean, h._L.pv_tsm_last_error(h._h)
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


def _near_tables():
    """(name, max_period, nin, psola grains) that read near where they write: the synthetic and the planned tables of tests/test_gpu_psola.py, and a plan of
    pv_tsm_plan at rate 1."""
    import test_gpu_psola as TGP
    out = [(name,) + TGP._grains(name) for name in ("tiny", "huge", "alternate", "gap", "voice")]
    recs = PM.records_of([217.3] * 30 + [-60.0] * 19)
    g, nout = TM.tsm_plan(recs, 64, 32, NOUT, 128.0, 32, 512, ratios=np.full(49, 0.8), rates=np.ones(49))
    assert nout == NOUT and TM.is_near(g, 512)
    out.append(("planned", 512, NOUT, TM.to_psola(g)))
    return out


def test_near_tables_give_the_bits_of_psola_process():
    """A table with |256 D + phi| <= 256 max_period is pv_psola_process's table in another notation: the same bits, at every max_rate the pair allows, from the
    host form, the device form and a range in the middle."""
    import phaze_amd
    import test_gpu_psola as TGP
    for name, mp, n, g in _near_tables():
        x = TGP._signals(n, 7 + len(name))
        ps = phaze_amd.Psola(mp, max_channels=NCH, max_outputs=NOUT)
        want = ps.process(x, g, 0, NOUT)
        ps.close()
        f = TM.from_psola(g)
        assert TM.is_near(f, mp) and np.array_equal(TM.to_psola(f), g)
        for R in ((1,) if mp == 4096 else (1, 4)):
            h = phaze_amd.Tsm(mp, R, max_channels=NCH, max_outputs=NOUT)
            got = h.process(x, f, 0, NOUT)
            assert got.dtype == np.float32 and np.array_equal(got, want), (name, R, int(np.sum(got != want)))
            assert np.array_equal(h.process(x, f, 1001, 1500), want[:, 1001:2501])
            assert np.array_equal(_device(h, x, f, [0, 1500, NOUT]), want)
            h.close()


def _partition(rng, total):
    """Cuts of [0, total) into calls of random length, empty ones among them."""
    cuts = [0, 0]
    while cuts[-1] < total:
        cuts.append(min(total, cuts[-1] + int(rng.choice([0, 1, 63, 64, 300, 1023, 1024, 1025, int(rng.integers(1, 700))]))))
    return cuts + [total]


def _fitting(rng, k):
    """A random partition none of whose calls has a tile beyond the span (the tiles of a call start at its first output, so the budget is per call)."""
    for _ in range(50):
        cuts = _partition(rng, NOUT)
        if 0 in np.diff(cuts) and len(cuts) > 4 and all(TM.check_span(k["g"], k["mp"], k["R"], a, b - a) is None for a, b in zip(cuts[:-1], cuts[1:]) if b > a):
            return cuts
    raise AssertionError("no partition fits")


@pytest.mark.parametrize("name", CASES)
def test_any_partition_and_every_form_give_the_same_bits(name):
    import phaze_amd
    import torch
    k = case(name)
    x, g, mp, R = k["x"], k["g"], k["mp"], k["R"]
    rng = np.random.default_rng(5 + len(name))
    h = phaze_amd.Tsm(mp, R, max_channels=NCH, max_outputs=NOUT)
    rc, want, clean = _raw(h, x, g, 0, NOUT)
    assert rc == 0 and clean
    assert np.array_equal(h.process(x, g, 0, NOUT), want)                                    # the binding, and a repeated call
    # a random partition of the output range, with empty calls, each call on its own rows
    cuts = _fitting(rng, k)
    parts = [h.process(x, g, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert all(p.shape == (NCH, b - a) for p, a, b in zip(parts, cuts[:-1], cuts[1:]))
    assert np.array_equal(np.concatenate(parts, axis=1), want)
    # a range in the middle, from an odd output on
    assert np.array_equal(h.process(x, g, 1001, 1500), want[:, 1001:2501])
    # a channel alone against the same channel among others
    for c in range(NCH):
        assert np.array_equal(h.process(x[c], g, 0, NOUT), want[c])
    # the device form on the handle's stream in one call
    assert np.array_equal(_device(h, x, g, [0, NOUT]), want)
    h.close()
    # host pieces: a staging buffer of one tile
    small = phaze_amd.Tsm(mp, R, max_channels=NCH, max_outputs=1)
    rc, y, clean = _raw(small, x, g, 0, NOUT, 3, 2, lead=1)
    assert rc == 0 and clean and np.array_equal(y, want)
    small.close()
    # the device form on a user stream, in pieces
    h = phaze_amd.Tsm(mp, R, max_channels=NCH)
    assert np.array_equal(_device(h, x, g, cuts, stream=torch.cuda.Stream()), want)
    h.close()


def test_the_host_form_falls_back_to_one_tile_per_piece_when_the_tiles_read_far_apart():
    """Three tiles whose source ranges lie a million samples apart: together they do not fit the staging buffer of a four-tile piece, so each goes alone."""
    import phaze_amd
    rng = np.random.default_rng(77)
    nin = 2_100_000
    x = rng.standard_normal(nin).astype(np.float32)
    t = np.arange(20, NOUT, 41)
    t = t[(t % TILE > 61) & (t % TILE < TILE - 61)]                          # no grain reaches two tiles
    g = _far_table(rng, t, 60, 0.0, 10)
    g[:, 2] -= (t // TILE) * 1_000_000 + 5000
    g = np.ascontiguousarray(g, np.int32)
    assert TM.check_span(g, 64, 1, 0, NOUT) is None
    y, tol, _ = TM.process(x, g, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
    h = phaze_amd.Tsm(64, 1, max_outputs=4096)
    got = h.process(x, g, 0, NOUT)
    assert np.all(np.abs(got - y[0]) <= tol[0]) and all(np.any(got[j * TILE + 100:(j + 1) * TILE - 100] != 0.0) for j in range(3))
    assert np.array_equal(_device(h, x[None, :], g, [0, NOUT])[0], got)
    h.close()


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_outputs_are_exactly_the_models(value):
    """A non-finite sample reaches exactly the outputs that have it under a tap of a grain with a non-zero weight, wherever in the input the grain reads: on a
    grain's edge, inside the 64-tap reach of a fractional displacement, and under a whole-sample one, which reads one sample only.  The finite outputs keep
    their bits in every form."""
    import phaze_amd
    for name in ("small", "tiny", "slow"):
        k = case(name)
        g, mp = k["g"], k["mp"]
        x = np.array(k["x"])
        n = x.shape[1]
        for j, c in ((g.shape[0] // 2, 0), (g.shape[0] // 3, 1), (g.shape[0] // 5, 2), (5, 0)):
            t, w, D, L = (int(v) for v in g[j])
            first = t - L + 1                                               # the grain's first output; its first tap reads first - D - 32
            x[c, min(max(first - D - 32, 0), n - 1)] = value
            x[c, min(max(t - D, 0), n - 1)] = -value if value == value else value
        y, tol, poisoned = TM.process(x, g, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
        h = phaze_amd.Tsm(mp, k["R"], max_channels=NCH, max_outputs=1024)
        got = h.process(x, g, 0, NOUT)
        assert np.array_equal(~np.isfinite(got), poisoned), (name, int(np.sum(~np.isfinite(got) != poisoned)))
        assert poisoned.any() and not poisoned.all()
        ok = ~poisoned
        assert np.all(np.abs(got[ok] - y[ok]) <= tol[ok])
        cuts = _fitting(np.random.default_rng(17), k)
        parts = np.concatenate([h.process(x, g, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
        assert np.array_equal(np.isfinite(parts), ok) and np.array_equal(parts[ok], got[ok])
        dev = _device(h, x, g, [0, NOUT])
        assert np.array_equal(np.isfinite(dev), ok) and np.array_equal(dev[ok], got[ok])
        h.close()


def test_refused_calls_leave_the_output_untouched_and_name_the_grain():
    import phaze_amd
    from phaze_amd import capi
    k = case("small")
    x, g, mp, R = k["x"], k["g"], k["mp"], k["R"]
    h = phaze_amd.Tsm(mp, R, max_channels=2, max_outputs=1024)

    def refused(grains, word, xx=x[:2], **kw):
        args = dict(out_first=0, nout=NOUT)
        args.update(kw)
        for fn in ("pv_tsm_process", "pv_tsm_process_device"):             # both forms check before any device work: host rows never reach the device
            rc, y, clean = _raw(h, xx, grains, args["out_first"], args["nout"], fn=fn)
            msg = h._L.pv_tsm_last_error(h._h).decode()
            assert rc == args.get("rc", capi.PV_ERR_ARGUMENT) and word in msg, (fn, rc, msg)
            assert clean and np.all(y == -77.0)

    last = g.shape[0] - 1
    for idx, col, val, word in [(7, 3, 1, "grain 7"), (7, 3, mp + 1, "grain 7"), (0, 0, -1, "grain 0"), (5, 0, 1 << 30, "grain 5"), (9, 1, 65536, "grain 9"),
                                (9, 1, -1, "grain 9"), (11, 2, 1 << 30, "grain 11"), (11, 2, -(1 << 30), "grain 11"), (last, 0, 5, f"grain {last}"),
                                (20, 0, int(g[19, 0]) - 1, "grain 20")]:
        bad = np.array(g)
        bad[idx, col] = val
        assert TM.check_grains(bad, mp)[0] == idx
        refused(bad, word)
    swapped = np.array(g)
    swapped[[30, 31]] = swapped[[31, 30]]
    refused(swapped, "grain 31")
    # a well-formed table with a tile that reads more than the span: the message names the tile's first grain
    for idx, val in ((60, 100000), (100, (1 << 30) - 1), (3, -((1 << 30) - 1))):
        wide = np.array(g)
        wide[idx, 2] = val
        assert TM.check_grains(wide, mp) is None
        tile, first, extent = TM.check_span(wide, mp, R, 0, NOUT)
        assert extent > TM.span(mp, R) and tile == int(g[idx, 0]) // TILE
        refused(wide, f"grain {first}:")
        msg = h._L.pv_tsm_last_error(h._h).decode()
        assert "span" in msg and str(extent) in msg and str(TM.span(mp, R)) in msg, msg
        # the tiles before it are fine: a call that ends before the tile is accepted
        if tile > 0:
            rc, y, clean = _raw(h, x[:2], wide, 0, tile * TILE - 200)
            assert rc == 0 and clean and np.all(np.abs(y - k["y"][:2, :tile * TILE - 200]) <= k["tol"][:2, :tile * TILE - 200])
    refused(g, "max_channels", xx=x[:3], rc=capi.PV_ERR_CAPACITY)
    refused(g, "2^30", out_first=(1 << 30) - 5)
    rc = h._L.pv_tsm_process(h._h, None, 100, 100, 1, g.ctypes.data_as(IP), g.shape[0], np.zeros(8, np.float32).ctypes.data_as(FP), 0, 8, 8)
    assert rc == capi.PV_ERR_ARGUMENT and "null" in h._L.pv_tsm_last_error(h._h).decode()
    out = np.full(8, -77.0, np.float32)
    xp, gp, op = x[0].ctypes.data_as(FP), g.ctypes.data_as(IP), out.ctypes.data_as(FP)
    for args in ((xp, 100, 100, 1, None, 3, op, 0, 8, 8), (xp, 100, 100, 1, gp, 3, None, 0, 8, 8), (xp, -1, 100, 1, gp, 3, op, 0, 8, 8), (xp, 100, 100, -1, gp, 3, op, 0, 8, 8),
                 (xp, 100, 100, 1, gp, -3, op, 0, 8, 8), (xp, 100, 100, 1, gp, 3, op, -1, 8, 8), (xp, 100, 100, 1, gp, 3, op, 0, -8, 8),
                 (x.ctypes.data_as(FP), 100, 99, 2, gp, 3, op, 0, 4, 4), (x.ctypes.data_as(FP), 100, 100, 2, gp, 3, op, 0, 4, 3)):
        assert h._L.pv_tsm_process(h._h, *args) == capi.PV_ERR_ARGUMENT and np.all(out == -77.0), args[1:6]
    # the handle still works, and a call without channels or outputs does nothing
    assert h._L.pv_tsm_process(h._h, None, 0, 0, 0, None, 0, None, 0, 0, 0) == 0
    assert np.array_equal(h.process(x[:2], g, 5, 0), np.zeros((2, 0), np.float32))
    assert np.all(np.abs(h.process(x[:2], g, 0, NOUT) - k["y"][:2]) <= k["tol"][:2])
    h.close()
    assert h._L.pv_tsm_destroy(None) == capi.PV_ERR_ARGUMENT


def test_process_tuned_at_half_speed_lands_on_the_note_and_keeps_the_formant():
    """The two-formant voice-like tone at 452 Hz (period 106.19), twelve thousand samples, at half speed.  process_tuned returns the model's grains (the device's
    records are the model's, tests/test_gpu_f0.py), an output of the model's output_len, about twice the input, and the bits of process(x, grains); the
    output's tracked note is 69 within the tolerance of tests/test_gpu_psola.py, twice the tracker's bound of 1.5e-3 relative on the period; and the
    strongest harmonic, the third, stays the third.  A per-record rate row gives the same as the number; rate 1 gives Psola.process_tuned's bits."""
    import phaze_amd
    n = FM.PLAN_LEN
    x = np.stack([PM.voice(FM.SAMPLE_RATE / 452.0, n), PM.voice(FM.SAMPLE_RATE / 452.0, n, phase=0.3)])
    h = phaze_amd.Tsm(1024, 2, max_channels=2)
    y, grains = h.process_tuned(x, FM.SAMPLE_RATE, rate=0.5)
    recs = FM.track(x[0], 1024, 256, 32, 1024)
    nrec = recs.shape[0]
    ratios = PM.tune_ratios(recs, FM.SAMPLE_RATE)
    want, want_len = TM.tsm_plan(recs, 256, 1024, n, 256.0, 32, 1024, ratios=ratios, rates=np.full(nrec, 0.5))
    assert np.all(recs[:, 0] > 0) and np.array_equal(grains, want) and y.shape == (2, want_len) and abs(want_len - 2 * n) <= 2 * 1024 - 3
    assert np.array_equal(y, h.process(x, grains, 0, want_len))
    y_row, g_row = h.process_tuned(x, FM.SAMPLE_RATE, rate=np.full(nrec, 0.5))
    assert np.array_equal(g_row, grains) and np.array_equal(y_row, y)
    y_one, g_one = h.process_tuned(x, FM.SAMPLE_RATE)
    ps = phaze_amd.Psola(1024, max_channels=2)
    y_ps, g_ps = ps.process_tuned(x, FM.SAMPLE_RATE)
    ps.close()
    assert np.array_equal(g_one, TM.from_psola(g_ps)) and np.array_equal(y_one, y_ps)
    with pytest.raises(ValueError):
        h.process_tuned(x, FM.SAMPLE_RATE, rate=np.full(nrec - 1, 0.5))
    h.close()
    out = FM.track(y[0, 2048:want_len - 1024], 1024, 256, 32, 1024)
    notes = [69.0 + 12.0 * np.log2(FM.SAMPLE_RATE / FM.period(r) / 440.0) for r in out]
    print("tracked notes of the output:", min(notes), max(notes), "output", want_len, "of", n)
    assert np.all(out[:, 0] > 0) and max(abs(v - 69.0) for v in notes) <= 12.0 * np.log2(1.0 + 2 * 1.5e-3)
    f_in, a_in, _ = PM.harmonic_amplitudes(x[0], FM.SAMPLE_RATE / 452.0, 3000, 9000)
    f_out, a_out, res = PM.harmonic_amplitudes(y[0], FM.SAMPLE_RATE / 440.0, 6000, 18000)
    k_in, k_out = int(np.argmax(a_in)) + 1, int(np.argmax(a_out)) + 1
    print(f"strongest harmonic: {f_in[k_in - 1] * FM.SAMPLE_RATE:.0f} Hz in, {f_out[k_out - 1] * FM.SAMPLE_RATE:.0f} Hz out, residual {res:.2e}")
    assert k_in == k_out == 3


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_tsm_example_plays_at_half_and_double_speed(tmp_path):
    import test_tsm_abi as TTA
    exe = TTA.build_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    print(j)
    assert abs(j["detected_note"] - (69.0 + 12.0 * np.log2(452.0 / 440.0))) < 0.03 and abs(j["strongest_harmonic_in"] - 3 * 452.0) < 1.0
    for key, speed in (("half_speed", 0.5), ("double_speed", 2.0)):
        assert abs(j[key]["samples"] - j["samples"] / speed) <= 2 * 1024 - 3, key
        assert abs(j[key]["note"] - 69.0) <= 12.0 * np.log2(1.0 + 2 * 1.5e-3) and abs(j[key]["strongest_harmonic"] - 3 * 440.0) < 1.0, key
