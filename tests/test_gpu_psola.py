"""The pitch-synchronous overlap-add kernel (Psola / pv_psola_*) on the GPU against the numpy model (tests/psola_model.py), and partition invariance.

Tolerance against the model, DERIVED the way tests/test_gpu_vari.py derives its own, u = 2^-24.  The model forms weights and sums in fp64 from the
library's own tables P and Hn and the same f32 input.  Per grain g with a fractional shift the kernel runs 64 fused multiply-adds into one f32
accumulator with the table's weights as they are, 64 additions into another, and one division:
    |xt^_g - xt_g| <= e_g = u [ 64 (a_g + |xt_g| s_g) / |d_g| + |xt_g| ],   a_g = sum |w_i x_i|, s_g = sum |w_i|, d_g = sum w_i,
and e_g = 0 for a whole-sample shift, which reads the sample itself.  The window weight is h^ = fl(fma(f^, d^, Hn[q])) with f^ = fl(rem * fl(1 / L)) and
d^ = fl(Hn[q + 1] - Hn[q]): three roundings on the product f d and one on the result, |h^ - h| <= 3 u m with m = |h| + |f d|.  With G grains covering
an output the numerator, G fused multiply-adds into one f32 accumulator, is within (G + 3) u A + E of sum h xt, A = sum m_g |xt_g|, E = sum |h_g| e_g,
and the weight sum within (G + 3) u S of D = sum h, S = sum m_g.  The quotient adds the relative errors and the division rounds once:
    |y_gpu - y| <= [ (G + 3) u (A + |y| S) + E ] / D + u |y|
to first order; the factor 1 + 2^-10 covers the second order, and 2^-149 (1 + (G + 67) / D) an intermediate in the subnormal range.  A, S, D, E and G
come from the model for that very sample.  No sample is left out; an output no grain covers must be exactly 0.  Everything else is bit for bit."""
import ctypes as C
import json
import shutil
import subprocess

import numpy as np
import pytest

import f0_model as FM
import psola_model as PM

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int32)
TILE = 1024
NOUT = 3 * TILE + 37
NCH = 3


def _grains(name):
    """(max_period, nin, grains int32[., 4]).  A tile holds 1024 outputs: every table spans three tiles and 37 outputs."""
    rng = np.random.default_rng(len(name) * 131 + ord(name[0]))
    n = NOUT
    if name == "tiny":                 # L = 2 .. 8, a grain every two or three samples: hundreds per tile; every kind of shift
        mp = 8
        t = np.cumsum(rng.integers(1, 4, 1400)) - 5
        t = t[(t >= 0) & (t < n + 6)]
        g = np.stack([t, rng.integers(0, 256, t.size), rng.integers(-256 * mp, 256 * mp + 1, t.size), rng.integers(2, 9, t.size)], axis=1)
        g[::5, 2] = (g[::5, 2] >> 8) << 8                                   # phi = 0
        g[1::7, 2] = ((g[1::7, 2] >> 8) << 8) + 1                            # phi = 1
        g[2::7, 2] = np.minimum(((g[2::7, 2] >> 8) << 8) + 255, 256 * mp - 1)  # phi = 255
        g[3::11, 1] = 0
        g[4::11, 1] = 255
        g[:2, 2] = [256 * mp, -256 * mp]
    elif name == "huge":               # L = max_period = 4096: every grain spans every tile and hangs over both ends; the largest shifts
        mp = 4096
        g = np.array([[0, 0, 0, 4096], [700, 255, -256 * 4096, 4096], [1500, 0, 256 * 4096, 4096], [1500, 0, 256 * 4095 + 255, 4096],
                      [1600, 255, -256 * 4096 + 1, 4096], [2900, 17, 256 * 2000 + 128, 4096], [n - 1, 128, -3, 4096], [n + 4000, 0, 256 * 4000, 4096]])
    elif name == "alternate":          # L alternating 32 / 300
        mp = 300
        t = np.arange(0, n + 250, 47)
        g = np.stack([t, rng.integers(0, 256, t.size), rng.integers(-256 * mp, 256 * mp + 1, t.size), np.where(np.arange(t.size) % 2, 300, 32)], axis=1)
        g[0, 2], g[1, 2], g[2, 2] = 256 * mp, -256 * mp, 0
    elif name == "gap":                # nothing between 950 and 2250: outputs 990 .. 2209 and the whole second tile are uncovered
        mp = 64
        t = np.concatenate([np.arange(3, 951, 19), np.arange(2250, n, 23)])
        g = np.stack([t, rng.integers(0, 256, t.size), rng.integers(-256 * mp, 256 * mp + 1, t.size), np.full(t.size, 40)], axis=1)
        g[t == 3 + 19 * 49, 1] = 0                                            # the last grain before the gap ends at a whole sample
    elif name == "empty":
        mp, g = 512, np.zeros((0, 4), np.int64)
    elif name == "voice":              # a planned table: period 217.3 moved by 1.25, then an unvoiced stretch
        mp = 512
        recs = PM.records_of([217.3] * 30 + [-60.0] * 19)
        g = PM.psola_plan(recs, 64, 32, n, 128.0, 32, mp, ratios=np.full(49, 1.25))
    else:
        raise KeyError(name)
    g = np.ascontiguousarray(g, np.int32).reshape(-1, 4)
    assert PM.check_grains(g, mp) is None, PM.check_grains(g, mp)
    return mp, n, g


CASES = ["tiny", "huge", "alternate", "gap", "empty", "voice"]


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
        mp, n, g = _grains(name)
        x = _signals(n, 7 + len(name))
        y, tol, poisoned = PM.process(x, g, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
        assert not poisoned.any()
        for a in (x, g, y, tol):
            a.setflags(write=False)
        _CACHE[name] = dict(mp=mp, n=n, g=g, x=x, y=y, tol=tol)
    return _CACHE[name]


def _raw(ps, x, g, out_first, nout, pad_in=0, pad_out=0, lead=0, fn="pv_psola_process"):
    """One host call through the raw C entry point: rows `lead` floats into their buffers (lead = 1: four bytes off any alignment) and strides longer than the rows.
    Returns (rc, out rows, whether everything around the rows still holds the fill)."""
    nch, nin = x.shape
    xin = np.full(lead + nch * (nin + pad_in), np.nan, np.float32)
    rows = xin[lead:].reshape(nch, nin + pad_in)
    rows[:, :nin] = x
    out = np.full(lead + nch * (nout + pad_out) + 3, -77.0, np.float32)
    orow = out[lead:lead + nch * (nout + pad_out)].reshape(nch, nout + pad_out)
    gp = g.ctypes.data_as(IP) if g.size else None
    rc = getattr(ps._L, fn)(ps._h, rows.ctypes.data_as(FP), nin, nin + pad_in, nch, gp, g.shape[0], orow.ctypes.data_as(FP), out_first, nout, nout + pad_out)
    clean = bool(np.all(orow[:, nout:] == -77.0) and np.all(out[:lead] == -77.0) and np.all(out[lead + nch * (nout + pad_out):] == -77.0))
    return rc, orow[:, :nout].copy(), clean


@pytest.mark.parametrize("name", CASES)
def test_every_sample_is_within_the_derived_bound_of_the_model(name):
    import phaze_amd
    k = case(name)
    covered = k["tol"][0] > 0
    if name == "gap":
        assert not covered[975:2210].any() and covered[:974].all() and covered[2212:].all() and not covered[TILE:2 * TILE].any()
    if name == "empty":
        assert not covered.any()
    for nch, pads, lead in ((1, (0, 0), 0), (3, (5, 129), 1)):
        ps = phaze_amd.Psola(k["mp"], max_channels=nch, max_outputs=NOUT)
        rc, y, clean = _raw(ps, k["x"][:nch], k["g"], 0, NOUT, *pads, lead=lead)
        assert rc == 0 and clean, ps._L.pv_psola_last_error(ps._h)
        err = np.abs(y.astype(np.float64) - k["y"][:nch])
        tol = k["tol"][:nch]
        worst = float(np.max(err[:, covered] / tol[:, covered])) if covered.any() else 0.0
        print(f"{name} nch {nch}: worst |err| / bound = {worst:.3f}, max |err| = {err.max():.3e}")
        assert np.all(err <= tol), (nch, int(np.sum(err > tol)), worst)
        assert np.all(y[:, ~covered] == 0.0) and not np.any(np.signbit(y[:, ~covered]))          # no grain: exact zeros
        ps.close()


def _partition(rng, total):
    """Cuts of [0, total) into calls of random length, empty ones among them."""
    cuts = [0, 0]
    while cuts[-1] < total:
        cuts.append(min(total, cuts[-1] + int(rng.choice([0, 1, 63, 64, 300, 1023, 1024, 1025, int(rng.integers(1, 700))]))))
    return cuts + [total]


@pytest.mark.parametrize("name", CASES)
def test_any_partition_and_every_form_give_the_same_bits(name):
    import phaze_amd
    import torch
    k = case(name)
    x, g, mp = k["x"], k["g"], k["mp"]
    rng = np.random.default_rng(5 + len(name))
    ps = phaze_amd.Psola(mp, max_channels=NCH, max_outputs=NOUT)
    rc, want, clean = _raw(ps, x, g, 0, NOUT)
    assert rc == 0 and clean
    assert np.array_equal(ps.process(x, g), want)                                           # the binding, and a repeated call
    # a random partition of the output range, with empty calls, each call on its own rows
    cuts = _partition(rng, NOUT)
    assert 0 in np.diff(cuts) and len(cuts) > 4
    parts = [ps.process(x, g, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert all(p.shape == (NCH, b - a) for p, a, b in zip(parts, cuts[:-1], cuts[1:]))
    assert np.array_equal(np.concatenate(parts, axis=1), want)
    # a range in the middle, from an odd output on
    assert np.array_equal(ps.process(x, g, 1001, 1500), want[:, 1001:2501])
    # a channel alone against the same channel among others
    for c in range(NCH):
        assert np.array_equal(ps.process(x[c], g), want[c])
    ps.close()
    # host pieces: a staging buffer of one tile
    small = phaze_amd.Psola(mp, max_channels=NCH, max_outputs=1)
    rc, y, clean = _raw(small, x, g, 0, NOUT, 3, 2, lead=1)
    assert rc == 0 and clean and np.array_equal(y, want)
    small.close()
    # the device form on a user stream, in pieces, padded strides, rows four bytes off their alignment
    ps = phaze_amd.Psola(mp, max_channels=NCH)
    stream = torch.cuda.Stream()
    ps.set_stream(stream.cuda_stream)
    n = x.shape[1]
    d_in = torch.full((NCH * (n + 7) + 1,), float("nan"), dtype=torch.float32, device="cuda")
    d_in[1:].view(NCH, n + 7)[:, :n] = torch.from_numpy(x.copy()).cuda()
    d_out = torch.full((NCH * (NOUT + 5) + 1,), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for a, b in zip(cuts[:-1], cuts[1:]):
        ps.process_device(d_in.data_ptr() + 4, n, n + 7, NCH, g, d_out.data_ptr() + 4 + 4 * a, a, b - a, NOUT + 5)
    ps.synchronize()
    got = d_out.cpu().numpy()
    assert got[0] == -77.0 and np.all(got[1:].reshape(NCH, NOUT + 5)[:, NOUT:] == -77.0)
    assert np.array_equal(got[1:].reshape(NCH, NOUT + 5)[:, :NOUT], want)
    ps.set_stream(None)
    ps.close()


def test_outputs_past_the_input_and_a_short_input():
    """The output range need not lie inside the input: samples outside [0, nin) read as zero, whatever the partition."""
    import phaze_amd
    k = case("alternate")
    x, g = k["x"][:, :2000], k["g"]
    want = PM.process(x, g, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
    ps = phaze_amd.Psola(k["mp"], max_channels=NCH, max_outputs=1024)
    y = ps.process(x, g, 0, NOUT)
    assert np.all(np.abs(y - want[0]) <= want[1])
    assert np.array_equal(np.concatenate([ps.process(x, g, 0, 1999), ps.process(x, g, 1999, NOUT - 1999)], axis=1), y)
    ps.close()


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_outputs_are_exactly_the_models(value):
    """A non-finite sample reaches exactly the outputs that have it under a tap of a grain with a non-zero weight: on a grain's edge, inside the 64-tap
    reach of a fractional shift, and under a whole-sample shift, which reads one sample only.  The finite outputs keep their bits in every form."""
    import phaze_amd
    import torch
    for name in ("alternate", "tiny", "voice"):
        k = case(name)
        g, mp = k["g"], k["mp"]
        x = np.array(k["x"])
        t, tf, dq, L = (int(v) for v in g[g.shape[0] // 2])
        first = t - L + 1                                                   # the grain's first output; its first tap reads first - D - 32
        x[0, min(max(first - (dq >> 8) - 32, 0), x.shape[1] - 1)] = value
        x[0, 1500] = value
        x[1, 1024] = value
        x[2, 3] = value
        x[2, NOUT - 2] = -value if value == value else value
        y, tol, poisoned = PM.process(x, g, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
        ps = phaze_amd.Psola(mp, max_channels=NCH, max_outputs=1024)
        got = ps.process(x, g)
        assert np.array_equal(~np.isfinite(got), poisoned), (name, int(np.sum(~np.isfinite(got) != poisoned)))
        assert poisoned.any() and not poisoned.all()
        ok = ~poisoned
        assert np.all(np.abs(got[ok] - y[ok]) <= tol[ok])
        rng = np.random.default_rng(17)
        cuts = _partition(rng, NOUT)
        parts = np.concatenate([ps.process(x, g, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
        assert np.array_equal(np.isfinite(parts), ok) and np.array_equal(parts[ok], got[ok])
        d_in = torch.from_numpy(x.copy()).cuda()
        d_out = torch.zeros((NCH, NOUT), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ps.process_device(d_in.data_ptr(), x.shape[1], x.shape[1], NCH, g, d_out.data_ptr(), 0, NOUT, NOUT)
        ps.synchronize()
        dev = d_out.cpu().numpy()
        assert np.array_equal(np.isfinite(dev), ok) and np.array_equal(dev[ok], got[ok])
        ps.close()


def test_refused_calls_leave_the_output_untouched_and_name_the_grain():
    import phaze_amd
    from phaze_amd import capi
    k = case("alternate")
    x, g, mp = k["x"], k["g"], k["mp"]
    ps = phaze_amd.Psola(mp, max_channels=2, max_outputs=1024)

    def refused(grains, word, xx=x[:2], **kw):
        args = dict(out_first=0, nout=NOUT)
        args.update(kw)
        for fn in ("pv_psola_process", "pv_psola_process_device"):         # both forms check before any device work: host rows never reach the device
            rc, y, clean = _raw(ps, xx, grains, args["out_first"], args["nout"], fn=fn)
            msg = ps._L.pv_psola_last_error(ps._h).decode()
            assert rc == args.get("rc", capi.PV_ERR_ARGUMENT) and word in msg, (fn, rc, msg)
            assert clean and np.all(y == -77.0)

    for idx, col, val, word in [(7, 3, 1, "grain 7"), (7, 3, mp + 1, "grain 7"), (0, 0, -1, "grain 0"), (5, 0, 1 << 30, "grain 5"), (9, 1, 256, "grain 9"),
                                (9, 1, -1, "grain 9"), (11, 2, 256 * mp + 1, "grain 11"), (11, 2, -256 * mp - 1, "grain 11"), (g.shape[0] - 1, 0, 5, f"grain {g.shape[0] - 1}"),
                                (20, 0, int(g[19, 0]) - 1, "grain 20")]:
        bad = np.array(g)
        bad[idx, col] = val
        assert PM.check_grains(bad, mp)[0] == idx
        refused(bad, word)
    swapped = np.array(g)
    swapped[[30, 31]] = swapped[[31, 30]]
    refused(swapped, "grain 31")
    refused(g, "max_channels", xx=x[:3], rc=capi.PV_ERR_CAPACITY)
    refused(g, "2^30", out_first=(1 << 30) - 5)
    rc = ps._L.pv_psola_process(ps._h, None, 100, 100, 1, g.ctypes.data_as(IP), g.shape[0], np.zeros(8, np.float32).ctypes.data_as(FP), 0, 8, 8)
    assert rc == capi.PV_ERR_ARGUMENT and "null" in ps._L.pv_psola_last_error(ps._h).decode()
    out = np.full(8, -77.0, np.float32)
    for args in ((x[0].ctypes.data_as(FP), 100, 100, 1, None, 3, out.ctypes.data_as(FP), 0, 8, 8), (x[0].ctypes.data_as(FP), 100, 100, 1, g.ctypes.data_as(IP), 3, None, 0, 8, 8),
                 (x[0].ctypes.data_as(FP), -1, 100, 1, g.ctypes.data_as(IP), 3, out.ctypes.data_as(FP), 0, 8, 8), (x[0].ctypes.data_as(FP), 100, 100, -1, g.ctypes.data_as(IP), 3, out.ctypes.data_as(FP), 0, 8, 8),
                 (x[0].ctypes.data_as(FP), 100, 100, 1, g.ctypes.data_as(IP), -3, out.ctypes.data_as(FP), 0, 8, 8), (x[0].ctypes.data_as(FP), 100, 100, 1, g.ctypes.data_as(IP), 3, out.ctypes.data_as(FP), -1, 8, 8),
                 (x[0].ctypes.data_as(FP), 100, 100, 1, g.ctypes.data_as(IP), 3, out.ctypes.data_as(FP), 0, -8, 8), (x.ctypes.data_as(FP), 100, 99, 2, g.ctypes.data_as(IP), 3, out.ctypes.data_as(FP), 0, 4, 4),
                 (x.ctypes.data_as(FP), 100, 100, 2, g.ctypes.data_as(IP), 3, out.ctypes.data_as(FP), 0, 4, 3)):
        assert ps._L.pv_psola_process(ps._h, *args) == capi.PV_ERR_ARGUMENT and np.all(out == -77.0), args[1:6]
    # the handle still works, and a call without channels or outputs does nothing
    assert ps._L.pv_psola_process(ps._h, None, 0, 0, 0, None, 0, None, 0, 0, 0) == 0
    assert np.array_equal(ps.process(x[:2], g, 5, 0), np.zeros((2, 0), np.float32))
    assert np.all(np.abs(ps.process(x[:2], g) - k["y"][:2]) <= k["tol"][:2])
    ps.close()
    assert ps._L.pv_psola_destroy(None) == capi.PV_ERR_ARGUMENT


def test_process_tuned_keeps_the_formant_and_lands_on_the_note():
    """A two-formant voice-like tone at 452 Hz (period 106.19), twelve thousand samples.  process_tuned returns the model's grains (the device's records
    are the model's, tests/test_gpu_f0.py) and the bits of process(x, grains); the output's tracked note is 69 within twice the tracker's bound of 1.5e-3
    relative on the period, 0.052 semitones; and the strongest harmonic, the third, stays the third: 1356 Hz becomes 1320 Hz, under the first formant
    at 1200 Hz either way, where the glide's resampler would have moved the formant itself."""
    import phaze_amd
    n = FM.PLAN_LEN
    x = np.stack([PM.voice(FM.SAMPLE_RATE / 452.0, n), PM.voice(FM.SAMPLE_RATE / 452.0, n, phase=0.3)])
    ps = phaze_amd.Psola(1024, max_channels=2)
    y, grains = ps.process_tuned(x, FM.SAMPLE_RATE)
    recs = FM.track(x[0], 1024, 256, 32, 1024)
    ratios = PM.tune_ratios(recs, FM.SAMPLE_RATE)
    want = PM.psola_plan(recs, 256, 1024, n, 256.0, 32, 1024, ratios=ratios)
    assert np.all(recs[:, 0] > 0) and np.array_equal(grains, want) and y.shape == x.shape
    assert np.array_equal(y, ps.process(x, grains))
    ps.close()
    out = FM.track(y[0, 2048:n - 1024], 1024, 256, 32, 1024)
    notes = [69.0 + 12.0 * np.log2(FM.SAMPLE_RATE / FM.period(r) / 440.0) for r in out]
    print("tracked notes of the output:", min(notes), max(notes))
    assert np.all(out[:, 0] > 0) and max(abs(v - 69.0) for v in notes) <= 12.0 * np.log2(1.0 + 2 * 1.5e-3)
    f_in, a_in, _ = PM.harmonic_amplitudes(x[0], FM.SAMPLE_RATE / 452.0, 3000, 9000)
    f_out, a_out, res = PM.harmonic_amplitudes(y[0], FM.SAMPLE_RATE / 440.0, 3000, 9000)
    k_in, k_out = int(np.argmax(a_in)) + 1, int(np.argmax(a_out)) + 1
    print(f"strongest harmonic: {f_in[k_in - 1] * FM.SAMPLE_RATE:.0f} Hz in, {f_out[k_out - 1] * FM.SAMPLE_RATE:.0f} Hz out, residual {res:.2e}")
    assert k_in == k_out == 3


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_psola_example_corrects_and_pieces_give_the_same_bits(tmp_path):
    import test_psola_abi as TPA
    exe = TPA.build_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    print(j)
    assert j["one_call_equals_pieces"] is True
    assert abs(j["detected_note"] - (69.0 + 12.0 * np.log2(452.0 / 440.0))) < 0.03 and abs(j["corrected_note"] - 69.0) <= 12.0 * np.log2(1.0 + 2 * 1.5e-3)
    assert abs(j["strongest_harmonic_in"] - 3 * 452.0) < 1.0 and abs(j["strongest_harmonic_out"] - 3 * 440.0) < 1.0
