"""The full-grain harmony kernel (Choir / pv_choir_*) on the GPU: bit equality with Harmony.process on plain tables, the values of Mirror.process and
Formant.process for one voice at gain 1, the derived bound against the numpy model (tests/choir_model.py) on tables of all four kinds of grain, bit equality
with the numpy float32 fold of the per-voice outputs, partition invariance, the span, non-finite samples, every refusal and process_tuned.

Tolerance against the model, DERIVED (tests/test_gpu_formant.py's docstring states it in full): for one voice the kernel's arithmetic on a grain is
pv_tsm_kernel's, pv_mirror_kernel's or pv_formant_kernel's operation for operation, and the mirrored warped grain runs pv_formant_kernel's operations on
another (m, r): the direction enters the addresses and the fraction only, never the way a value is rounded, so the bound per grain,
e_g = u [(Tloc + 3) (a_g + |xt| s_g) / |d_g| + |xt|] for a warped grain of Tloc non-zero taps and u [64 (a_g + |xt| s_g) / |d_g| + |xt|] for a fractional
unwarped one, and the window and fold terms are unchanged: choir_model.voice(bound=True) returns formant_model's bound per sample.  The mix adds
harmony_model's fold bound.  No sample is left out; an output no voice covers must be exactly 0.  Everything else is bit for bit.
Worst observed |err| / bound: 0.136 (`small` with every third grain of each kind, three channels); 0.087 and below on the other mixed one-voice tables,
0.047 on the mixes of three and eight voices, 0.033 on the planned voices.  One MI355X."""
import ctypes as C
import json
import shutil
import subprocess

import numpy as np
import pytest

import choir_model as CM
import f0_model as FM
import harmony_model as HM
import psola_model as PM
import test_choir_model as TCM
import test_formant_abi as TFA
import test_gpu_harmony as TGH
import test_gpu_tsm as TGT
import test_psola_model as TPM

pytestmark = pytest.mark.gpu

FP, IP, LP = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
TILE = TGT.TILE
NOUT = TGT.NOUT
NCH = TGT.NCH
STEP, BIT = CM.STEP, CM.MIRROR
MIXED = [("small", "thirds"), ("tiny", "thirds"), ("mid", "thirds"), ("sweep", "thirds"), ("gap", "thirds"), ("small", "all"), ("tiny", "all"), ("mid", "all")]


def _raw(h, x, tables, gains, out_first, nout, pad_in=0, pad_out=0, lead=0, fn="pv_choir_process", **kw):
    return TGH._raw(h, x, tables, gains, out_first, nout, pad_in, pad_out, lead, fn, **kw)


def _error(h):
    return h._L.pv_choir_last_error(h._h).decode()


_CACHE = {}


def one(name, mode):
    """Shared per mixed one-voice table, computed once and never written: the far table `name` of tests/test_gpu_tsm.py with the full grain word
    (test_choir_model.full_table), the input, the model's output on the library's tables and its bound."""
    if (name, mode) not in _CACHE:
        import phaze_amd
        mp, R, nin, g = TGT._grains(name)
        m = TCM.full_table(g, mode)
        assert CM.check_grains(m, mp) is None and CM.check_span([m], mp, R, 0, NOUT) is None, (CM.check_grains(m, mp), CM.check_span([m], mp, R, 0, NOUT), CM.span(mp, R))
        both = CM.mirrored(m) & CM.warped(m)
        s, phi, tf = CM.steps(m)[both], (m[both, 1] >> 8) & 255, m[both, 1] & 255
        assert both.sum() < 16 or (set(s.tolist()) == set(TCM.STEPS) and {0, 1, 255} <= set(phi.tolist()) and {0, 255} <= set(tf.tolist()))
        x = TGT._signals(nin, 7 + len(name))
        y, tol, poisoned = CM.voice(x, m, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
        assert not poisoned.any()
        for a in (x, m, y, tol):
            a.setflags(write=False)
        _CACHE[(name, mode)] = dict(mp=mp, R=R, n=nin, g=m, x=x, y=y, tol=tol)
    return _CACHE[(name, mode)]


def _voices(nv):
    """(max_period, max_rate, nin, tables): nv = 8: the eight voices of tests/test_gpu_harmony.py's small8 (voice 3 is empty, voice 5 has nothing between outputs
    950 and 2250: the whole second tile), at max_period 64; nv = 3: voices 5, 3 and 0 of its mid8, at max_period 1024.  The voices take the full grain word
    in turn: every third grain of each kind, all grains mirrored and warped, plain."""
    mp, R, nin, tables = TGH._voices("small8" if nv == 8 else "mid8")
    if nv == 3:
        tables = [tables[5], tables[3], tables[0]]
    out = []
    for v, t in enumerate(tables):
        out.append(np.ascontiguousarray(t if v % 3 == 2 or t.shape[0] == 0 else TCM.full_table(t, ("thirds", "all")[v % 3])))
    assert CM.check_voices(out, mp) is None and CM.check_span(out, mp, R, 0, NOUT) is None, (CM.check_voices(out, mp), CM.check_span(out, mp, R, 0, NOUT), CM.span(mp, R))
    return mp, R, nin, out


def many(nv):
    """Shared per case of several voices, computed once and never written: input, tables, gains (the last voice muted on channel 2), the model's per-voice
    outputs with their bounds, and which outputs each voice covers."""
    if nv not in _CACHE:
        import phaze_amd
        mp, R, nin, tables = _voices(nv)
        x = TGT._signals(nin, 11 + nv)
        gains = np.random.default_rng(99 + nv).uniform(-1.5, 1.5, (nv, NCH)).astype(np.float32)
        gains[nv - 1, 2] = 0.0
        P, H = phaze_amd.vari_prototype(), phaze_amd.psola_window()
        outs = [CM.voice(x, t, 0, NOUT, P, H, bound=True) for t in tables]
        y, tol, poisoned = CM.process(x, tables, gains, 0, NOUT, bound=True, outs=outs)
        covered = np.stack([o[1][0] > 0 for o in outs])
        assert not poisoned.any()
        for a in [x, gains, y, tol, covered] + tables:
            a.setflags(write=False)
        _CACHE[nv] = dict(mp=mp, R=R, n=nin, tables=tables, x=x, gains=gains, y=y, tol=tol, covered=covered)
    return _CACHE[nv]


# ---- against the siblings ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["small2", "small8", "mid2"])
def test_plain_tables_give_the_bits_of_harmony_process(name):
    """The voices of tests/test_gpu_harmony.py, 2 and 8 of them, and the first of them alone: Harmony.process's output with ==, from the host form on padded
    rows, a range in the middle and the device form."""
    import phaze_amd
    k = TGH.case(name)
    x, tables, gains, mp, R = k["x"], k["tables"], k["gains"], k["mp"], k["R"]
    for tabs, w in ((tables, gains), (tables[:1], gains[:1])):
        nv = len(tabs)
        hv = phaze_amd.Harmony(mp, R, max_voices=nv, max_channels=NCH, max_outputs=NOUT)
        want = hv.process(x, tabs, w, 0, NOUT)
        hv.close()
        h = phaze_amd.Choir(mp, R, max_voices=nv, max_channels=NCH, max_outputs=NOUT)
        rc, got, clean = _raw(h, x, tabs, w, 0, NOUT, 5, 129, lead=1)
        assert rc == 0 and clean, _error(h)
        assert got.dtype == np.float32 and np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want)), (name, nv, int(np.sum(got != want)))
        assert np.array_equal(h.process(x, tabs, w, 1001, 1500), want[:, 1001:2501])
        assert np.array_equal(TGH._device(h, x, tabs, w, [0, 1500, NOUT]), want)
        h.close()


@pytest.mark.parametrize("name", ["small", "tiny", "mid", "sweep", "slow"])
def test_one_voice_at_gain_one_gives_the_values_of_mirror_process_and_formant_process(name):
    """Mirror-only tables (every second grain, and every grain, mirrored) against Mirror.process and warp-only tables (every third grain, and every grain,
    warped) against Formant.process: the same values, -0 and +0 equal (the fold starts from +0)."""
    import phaze_amd
    mp, R, nin, g = TGT._grains(name)
    x = TGT._signals(nin, 7 + len(name))
    h = phaze_amd.Choir(mp, R, max_voices=1, max_channels=NCH, max_outputs=NOUT)
    for cls, tabs in ((phaze_amd.Mirror, (TCM.mirror_table(g), TCM.mirror_table(g, 1, 0))), (phaze_amd.Formant, (TFA.warp_table(g), TFA.warp_table(g, 1, 0)))):
        sib = cls(mp, R, max_channels=NCH, max_outputs=NOUT)
        for table in tabs:
            want = sib.process(x, table, 0, NOUT)
            got = h.process(x, [table], [1.0], 0, NOUT)
            assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want), (name, cls.__name__, int(np.sum(got != want)))
            assert np.array_equal(TGH._device(h, x, [table], [1.0], [0, NOUT]), want)
            assert np.array_equal(h.process(x[1], [table], [1.0], 1001, 1500), want[1, 1001:2501])
        sib.close()
    h.close()


# ---- mixed tables -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,mode", MIXED)
def test_every_sample_of_a_mixed_voice_is_within_the_derived_bound_of_the_model(name, mode):
    import phaze_amd
    k = one(name, mode)
    covered = k["tol"][0] > 0
    both = CM.mirrored(k["g"]) & CM.warped(k["g"])
    assert both.all() if mode == "all" else (both.sum() >= k["g"].shape[0] // 4 and not both.all())
    if name == "gap":
        assert not covered[975:2210].any() and not covered[TILE:2 * TILE].any()
    for nch, pads, lead in ((1, (0, 0), 0), (3, (5, 129), 1)):
        h = phaze_amd.Choir(k["mp"], k["R"], max_voices=1, max_channels=nch, max_outputs=NOUT)
        rc, y, clean = _raw(h, k["x"][:nch], [k["g"]], np.ones((1, nch), np.float32), 0, NOUT, *pads, lead=lead)
        assert rc == 0 and clean, _error(h)
        err = np.abs(y.astype(np.float64) - k["y"][:nch])
        tol = k["tol"][:nch]
        live = covered[None, :] & (tol > 0)
        worst = float(np.max(err[live] / tol[live])) if live.any() else 0.0
        print(f"{name} {mode} nch {nch}: worst |err| / bound = {worst:.3f}, max |err| = {err.max():.3e}")
        assert np.all(err <= tol), (nch, int(np.sum(err > tol)), worst)
        assert np.all(y[:, ~covered] == 0.0) and not np.any(np.signbit(y[:, ~covered]))          # no grain: exact zeros
        h.close()


def _per_voice(h, x, tables, nout=NOUT, first=0):
    """float32[V, nch, nout]: every voice alone at gain 1 through the same handle."""
    return np.stack([h.process(x, [t], [1.0], first, nout) for t in tables])


@pytest.mark.parametrize("nv", [3, 8])
def test_the_mix_is_the_float32_fold_of_the_per_voice_outputs(nv):
    """Three voices at max_period 1024 and eight at 64, among them an empty voice, a voice with a whole-tile gap and a voice muted on one channel, the voices
    in turn with every third grain of each kind, all grains mirrored and warped, and plain: the output == the numpy float32 fold of the per-voice Choir outputs,
    and lies within the model's bound."""
    import phaze_amd
    k = many(nv)
    empty, gap = (1, 0) if nv == 3 else (3, 5)
    assert k["tables"][empty].shape[0] == 0 and not k["covered"][empty].any() and not k["covered"][gap][TILE:2 * TILE].any() and k["covered"][gap][:900].all()
    assert k["gains"][nv - 1, 2] == 0.0 and sum(int((CM.mirrored(t) & CM.warped(t)).sum()) for t in k["tables"]) > 10
    any_voice = k["covered"].any(axis=0)
    for nch, pads, lead in ((1, (0, 0), 0), (3, (5, 129), 1)):
        gains = k["gains"][:, :nch]
        h = phaze_amd.Choir(k["mp"], k["R"], max_voices=nv, max_channels=nch, max_outputs=NOUT)
        rc, y, clean = _raw(h, k["x"][:nch], k["tables"], gains, 0, NOUT, *pads, lead=lead)
        assert rc == 0 and clean, _error(h)
        want = HM.mix(_per_voice(h, k["x"][:nch], k["tables"]), k["covered"], gains)
        assert np.array_equal(y, want), (nch, int(np.sum(y != want)))
        err = np.abs(y.astype(np.float64) - k["y"][:nch])
        tol = k["tol"][:nch]
        live = tol > 0
        print(f"V = {nv} nch {nch}: worst |err| / bound = {float(np.max(err[live] / tol[live])):.3f}, max |err| = {err.max():.3e}")
        assert np.all(err <= tol), (nch, int(np.sum(err > tol)))
        assert np.all(y[:, ~any_voice] == 0.0)
        h.close()


@pytest.mark.parametrize("nv", [3, 8])
def test_any_partition_and_every_form_give_the_same_bits(nv):
    """One call, a repeated call, calls split at odd outputs with an empty one among them, a range in the middle, a channel alone, host pieces of one tile, and
    the device form on the handle's stream and on a user stream."""
    import phaze_amd
    import torch
    k = many(nv)
    x, tables, gains, mp, R = k["x"], k["tables"], k["gains"], k["mp"], k["R"]
    h = phaze_amd.Choir(mp, R, max_voices=nv, max_channels=NCH, max_outputs=NOUT)
    rc, want, clean = _raw(h, x, tables, gains, 0, NOUT)
    assert rc == 0 and clean
    assert np.array_equal(h.process(x, tables, gains, 0, NOUT), want)                        # the binding, and a repeated call
    cuts = [0, 0, 700, 701, 1900, 2947, NOUT]                                                # the tiles of a call start at its first output
    assert all(CM.check_span(tables, mp, R, a, b - a) is None for a, b in zip(cuts[:-1], cuts[1:]) if b > a)
    parts = [h.process(x, tables, gains, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts, axis=1), want)
    assert np.array_equal(h.process(x, tables, gains, 1001, 1500), want[:, 1001:2501])
    for c in range(NCH):
        assert np.array_equal(h.process(x[c], tables, gains[:, c], 0, NOUT), want[c])
    assert np.array_equal(TGH._device(h, x, tables, gains, [0, NOUT]), want)
    h.close()
    small = phaze_amd.Choir(mp, R, max_voices=nv, max_channels=NCH, max_outputs=1)           # host pieces of one tile
    rc, y, clean = _raw(small, x, tables, gains, 0, NOUT, 3, 2, lead=1)
    assert rc == 0 and clean and np.array_equal(y, want)
    small.close()
    h = phaze_amd.Choir(mp, R, max_channels=NCH)                                             # the defaults, the device form on a user stream, in pieces
    assert np.array_equal(h.process(x, tables, gains, 0, NOUT), want)
    assert np.array_equal(TGH._device(h, x, tables, gains, cuts, stream=torch.cuda.Stream()), want)
    h.close()


# ---- the span ---------------------------------------------------------------------------------------------------------------------------------------

def _device_tile(h, x, tables, gains):
    """The device form on one tile of outputs."""
    import torch
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((x.shape[0], TILE), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    h.process_device(d_in.data_ptr(), x.shape[1], x.shape[1], x.shape[0], tables, gains, d_out.data_ptr(), 0, TILE, TILE)
    h.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("mp,R", [(64, 1), (1024, 4)])
def test_a_mirrored_grain_of_step_512_may_bring_a_hull_to_exactly_the_span_and_no_further(mp, R):
    """Voice 0 holds a plain grain that reads from position 3 on; voice 1 a mirrored grain of step 512 whose range on tile 0 ends at D + c: with
    D = 3 + span - c the hull of the tile is exactly span(max_period, max_rate) and the call is accepted and within the bound; one sample more is refused
    with PV_ERR_ARGUMENT, the message names the tile, the first grain of its lowest voice and the extent, and the output keeps its fill."""
    import phaze_amd
    from phaze_amd import capi
    cap = CM.span(mp, R)
    nin = cap + 700
    x = TGT._signals(nin, 3)[:2]
    gains = np.array([[0.75, -0.5], [0.5, 1.25]], np.float32)
    word = BIT + 512 * STEP + 256 * 77 + 200
    c = int(CM.tiles(np.array([[600, word, 0, 64]]), mp, 0, TILE)[0, 2:].sum())                # where the grain's range ends at D = 0
    voices = lambda D: [np.array([[100, 7, 0, 64]], np.int32), np.array([[600, word, D, 64]], np.int32)]
    fit = voices(3 + cap - c)
    assert CM.check_voices(fit, mp) is None and CM.hull(fit, mp, 0, TILE)[0].tolist() == [[3, cap]] and CM.check_span(fit, mp, R, 0, TILE) is None
    h = phaze_amd.Choir(mp, R, max_voices=2, max_channels=2, max_outputs=TILE)
    y, tol, _ = CM.process(x, fit, gains, 0, TILE, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
    wide = voices(4 + cap - c)
    assert CM.check_voices(wide, mp) is None and CM.check_span(wide, mp, R, 0, TILE) == (0, 0, 0, cap + 1)
    for fn in ("pv_choir_process", "pv_choir_process_device"):
        rc, out, clean = _raw(h, x, wide, gains, 0, TILE, fn=fn)                  # host rows never reach the device: refused before any device work
        msg = _error(h)
        assert rc == capi.PV_ERR_ARGUMENT and "tile 0: voice 0 grain 0:" in msg and "span" in msg and str(cap + 1) in msg and str(cap) in msg, msg
        assert clean and np.all(out == -77.0)
    rc, out, clean = _raw(h, x, fit, gains, 0, TILE)
    assert rc == 0 and clean, _error(h)
    assert np.all(np.abs(out - y) <= tol) and np.any(out[:, 540:660] != 0.0) and np.any(out[:, 40:160] != 0.0)
    assert np.array_equal(_device_tile(h, x, fit, gains), out)
    h.close()


# ---- non-finite samples -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_samples_reach_exactly_the_models_outputs_and_a_muted_voice_keeps_them_out(value):
    """Three voices of mixed grains at max_period 64: voice 1 reads 3000 samples ahead of the others and is muted on channel 1 only.  Non-finite samples lie
    under the outermost taps and the centre of mirrored warped grains of voice 0 (channel 0) and of voice 1 (channels 1 and 2), and where only voice 1 reads,
    in every channel: the output is non-finite exactly where the model says (the zero-weight rule included), channel 1 stays finite everywhere, and the
    finite outputs keep their bits in every form."""
    import phaze_amd
    rng = np.random.default_rng(61)
    mp, R = 64, 4
    nin = NOUT + 3400
    far = [TGT._far_table(rng, np.arange(v, NOUT + 40, stride), 40, 0.0, 50) for v, stride in enumerate((17, 23, 29))]
    far[1][:, 2] -= 3000
    tables = [TCM.full_table(far[0], "thirds"), TCM.full_table(far[1], "all"), np.ascontiguousarray(far[2], np.int32)]
    assert CM.check_voices(tables, mp) is None and CM.check_span(tables, mp, R, 0, NOUT) is None
    x = np.array(TGT._signals(nin, 13))
    for v, c in ((0, 0), (1, 2), (1, 1)):
        g = tables[v]
        both = np.flatnonzero(CM.mirrored(g) & CM.warped(g))
        for j in (both[both.size // 3], both[both.size // 2]):
            t, w, D, L = (int(q) for q in g[j])
            s = w >> 17
            W = 32 if s < 256 else 64
            m0 = int(CM._m(t, w & 255, (w >> 8) & 255, D, s, True, t - L + 1)[0])
            x[c, min(max(m0 - W + 1, 0), nin - 1)] = value                   # tap 0 of the grain's first output: weight 0 unless r is 0
            x[c, min(max(m0 + W, 0), nin - 1)] = value                       # its last tap
            x[c, min(max(D - t, 0), nin - 1)] = -value if value == value else value
    x[:, 4500] = value                                                       # where only voice 1 reads (outputs near 1500)
    gains = np.array([[1.0, 0.5, -0.25], [0.5, 0.0, 0.75], [-1.0, 1.0, 0.5]], np.float32)
    y, tol, poisoned = CM.process(x, tables, gains, 0, NOUT, phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
    assert poisoned[0].any() and poisoned[2].any() and not poisoned[1].any() and not poisoned.all() and poisoned[0, 1400:1600].any()
    h = phaze_amd.Choir(mp, R, max_voices=3, max_channels=3, max_outputs=1024)
    got = h.process(x, tables, gains, 0, NOUT)
    assert np.all(np.isfinite(got[1]))
    assert np.array_equal(~np.isfinite(got), poisoned), int(np.sum(~np.isfinite(got) != poisoned))
    ok = ~poisoned
    assert np.all(np.abs(got[ok] - y[ok]) <= tol[ok])
    parts = np.concatenate([h.process(x, tables, gains, a, b - a) for a, b in ((0, 1001), (1001, 2333), (2333, NOUT))], axis=1)
    assert np.array_equal(np.isfinite(parts), ok) and np.array_equal(parts[ok], got[ok])
    dev = TGH._device(h, x, tables, gains, [0, 1300, NOUT])
    assert np.array_equal(np.isfinite(dev), ok) and np.array_equal(dev[ok], got[ok])
    assert not np.any(h.process(x, tables, np.zeros((3, 3), np.float32), 0, NOUT))           # all gains zero: nothing is read, everything is zero
    h.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_leave_the_output_untouched_and_name_voice_and_grain():
    import phaze_amd
    from phaze_amd import capi
    k = TGH.case("small2")
    x, mp, R = k["x"][:2], k["mp"], k["R"]
    tables = [TCM.full_table(k["tables"][0], "thirds"), TCM.full_table(k["tables"][1], "thirds")]
    gains = np.array(k["gains"][:, :2])
    assert CM.check_voices(tables, mp) is None and CM.check_span(tables, mp, R, 0, NOUT) is None
    h = phaze_amd.Choir(mp, R, max_voices=2, max_channels=2, max_outputs=1024)

    def refused(tabs, word, xx=x, w=gains, rc=capi.PV_ERR_ARGUMENT, out_first=0, **kw):
        for fn in ("pv_choir_process", "pv_choir_process_device"):         # both forms check before any device work: host rows never reach the device
            got, y, clean = _raw(h, xx, tabs, w, out_first, NOUT, fn=fn, **kw)
            msg = _error(h)
            assert got == rc and word in msg, (fn, got, msg)
            assert clean and np.all(y == -77.0)

    for voice in (0, 1):
        g = tables[voice]
        last = g.shape[0] - 1
        fwd = [int(i) for i in np.flatnonzero(~CM.mirrored(g))[2:4]]          # a warped forward grain (i % 3 == 1) and a plain one (i % 10 == 9) are among them
        mir = [int(i) for i in np.flatnonzero(CM.mirrored(g))[2:4]]           # a mirrored and a mirrored warped grain
        assert CM.warped(g)[mir].any() and not CM.warped(g)[mir].all()
        cases = [(9, 1, 1 << 27), (10, 1, (1 << 27) + int(g[10, 1])), (9, 1, -1),                                    # w >= 2^27, w < 0
                 (9, 1, 127 * STEP + 5), (10, 1, BIT + 513 * STEP), (9, 1, STEP), (10, 1, BIT + 127 * STEP),           # z = 127, 513 and 1, either direction
                 (fwd[0], 2, 1 << 30), (fwd[1], 2, 1 << 30), (fwd[0], 2, -(1 << 30)),                                # a forward grain with D >= 2^30 or D <= -2^30
                 (mir[0], 2, -(1 << 30)), (mir[1], 2, -(1 << 30)),                                                   # a mirrored grain with D <= -2^30
                 (7, 3, 1), (7, 3, mp + 1), (10, 3, 0),                                                              # L
                 (0, 0, -1), (5, 0, 1 << 30), (last, 0, 5), (20, 0, int(g[19, 0]) - 1)]                              # centre and order
        for idx, col, val in cases:
            bad = [np.array(t) for t in tables]
            bad[voice][idx, col] = val
            assert CM.check_voices(bad, mp)[:2] == (voice, idx), (idx, col, val)
            refused(bad, f"voice {voice} grain {idx}:")
        swapped = [np.array(t) for t in tables]
        swapped[voice][[30, 31]] = swapped[voice][[31, 30]]
        refused(swapped, f"voice {voice} grain 31:")
        # a mirrored D of 2^30 and more passes validation; then the span refuses the tile
        wide = [np.array(t) for t in tables]
        wide[voice][mir[1], 2] = (1 << 31) - 1
        assert CM.check_voices(wide, mp) is None
        tile, v, grain, extent = CM.check_span(wide, mp, R, 0, NOUT)
        refused(wide, f"tile {tile}: voice {v} grain {grain}:")
        assert str(extent) in _error(h) and "span" in _error(h)
    assert tables[1][0, 0] < tables[0][-1, 0]                                # centres restart at a voice boundary, and that is no error
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
    g, vf = TGH._flat(tables)
    w1 = np.ones(2, np.float32)
    xp, gp, fp_, wp, op = x[0].ctypes.data_as(FP), g.ctypes.data_as(IP), vf.ctypes.data_as(LP), w1.ctypes.data_as(FP), out.ctypes.data_as(FP)
    for args in ((None, 100, 100, 1, gp, fp_, 2, wp, op, 0, 8, 8), (xp, 100, 100, 1, None, fp_, 2, wp, op, 0, 8, 8), (xp, 100, 100, 1, gp, fp_, 2, wp, None, 0, 8, 8),
                 (xp, -1, 100, 1, gp, fp_, 2, wp, op, 0, 8, 8), (xp, 100, 100, -1, gp, fp_, 2, wp, op, 0, 8, 8), (xp, 100, 100, 1, gp, fp_, 2, wp, op, -1, 8, 8),
                 (xp, 100, 100, 1, gp, fp_, 2, wp, op, 0, -8, 8), (x.ctypes.data_as(FP), 100, 99, 2, gp, fp_, 2, gains.ctypes.data_as(FP), op, 0, 4, 4),
                 (x.ctypes.data_as(FP), 100, 100, 2, gp, fp_, 2, gains.ctypes.data_as(FP), op, 0, 4, 3)):
        for fn in (h._L.pv_choir_process, h._L.pv_choir_process_device):
            assert fn(h._h, *args) == capi.PV_ERR_ARGUMENT and np.all(out == -77.0), args[1:4]
    # the handle still works; a call without channels or outputs does nothing; an empty voice is legal
    none = np.zeros(3, np.int64)
    assert h._L.pv_choir_process(h._h, None, 0, 0, 0, None, none.ctypes.data_as(LP), 2, None, None, 0, 0, 0) == 0
    assert np.array_equal(h.process(x, tables, gains, 5, 0), np.zeros((2, 0), np.float32))
    lone = h.process(x, [tables[0], tables[1][:0]], gains, 0, NOUT)
    assert np.array_equal(lone, h.process(x, [tables[0][:0], tables[0]], gains[::-1], 0, NOUT)) and np.any(lone != 0.0)
    h.close()
    assert h._L.pv_choir_destroy(None) == capi.PV_ERR_ARGUMENT


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------------

def test_process_tuned_is_the_hand_made_pipeline_and_the_models_tables():
    """The voice of tests/test_psola_model.py (period 217.3, resonators at 1200 and 2600 Hz), twelve thousand samples: the lead, a major second below with the
    formants lowered to 0.85 and a major third above with them raised to 1.15, at half tempo with mirror on.  process_tuned returns the model's grain tables
    (the device's f0 records are the model's, tests/test_gpu_f0.py) and about 24 000 samples, voice 0's output_len, and the bits of the hand-made pipeline
    (harmony_ratios, three choir_plans, one process); with warps=None and mirror=False it gives Harmony.process_tuned's tables and bits."""
    import phaze_amd
    n = FM.PLAN_LEN
    p = FM.period(PM.records_of([TPM.PERIOD])[0])
    x = np.stack([PM.voice(p, n), PM.voice(p, n, phase=0.3)]).astype(np.float32)
    degrees, warps = (0, -2, 4), (1.0, 0.85, 1.15)
    h = phaze_amd.Choir(1024, 2, 3, max_channels=2)
    y, tables = h.process_tuned(x, FM.SAMPLE_RATE, degrees=degrees, warps=warps, rate=0.5, mirror=True)
    recs = FM.track(x[0], 1024, 256, 32, 1024)
    nrec = recs.shape[0]
    ratios = HM.harmony_ratios(recs, FM.SAMPLE_RATE, degrees)
    model = [CM.choir_plan(recs, 256, 1024, n, 256.0, 32, 1024, ratios=ratios[v], rates=np.full(nrec, 0.5), warps=np.full(nrec, warps[v]), mirror=True) for v in range(3)]
    assert len(tables) == 3 and all(np.array_equal(a, b[0]) for a, b in zip(tables, model))
    assert y.shape == (2, model[0][1]) and abs(model[0][1] - 2 * n) <= 2 * 1024 - 3
    assert not CM.warped(tables[0]).any() and np.all(CM.steps(tables[1]) == 218) and np.all(CM.steps(tables[2]) == 294)
    tracker = phaze_amd.F0Tracker(1024, 256, 32, 1024)
    dev_recs = tracker.track(x[0], 2458)[0]
    tracker.close()
    rows = phaze_amd.harmony_ratios(dev_recs, FM.SAMPLE_RATE, degrees)
    plans = [phaze_amd.choir_plan(dev_recs, 256, 1024, n, 256.0, 32, 1024, ratios=rows[v], rates=np.full(nrec, 0.5), warps=np.full(nrec, warps[v]), mirror=True)
             for v in range(3)]
    assert all(np.array_equal(a, b[0]) for a, b in zip(tables, plans))
    assert np.array_equal(y, h.process(x, tables, np.full(3, 1.0 / 3.0, np.float32), 0, plans[0][1])) and np.any(y != 0.0)
    ym, tol, poisoned = CM.process(x, tables, np.full(3, 1.0 / 3.0, np.float32), 0, plans[0][1], phaze_amd.vari_prototype(), phaze_amd.psola_window(), bound=True)
    err = np.abs(y.astype(np.float64) - ym)
    print(f"{nrec} records; grains {[t.shape[0] for t in tables]}; output {plans[0][1]} of {n}; worst |err| / bound = {float(np.max(err[tol > 0] / tol[tol > 0])):.3f}")
    assert not poisoned.any() and np.all(err <= tol)
    y0, t0 = h.process_tuned(x, FM.SAMPLE_RATE, degrees=degrees, warps=None, rate=0.5, mirror=False)
    hv = phaze_amd.Harmony(1024, 2, 3, max_channels=2)
    yh, th = hv.process_tuned(x, FM.SAMPLE_RATE, degrees=degrees, rate=0.5)
    hv.close()
    assert all(np.array_equal(a, b) for a, b in zip(t0, th)) and np.array_equal(y0, yh) and np.array_equal(np.signbit(y0), np.signbit(yh))
    with pytest.raises(ValueError):
        h.process_tuned(x, FM.SAMPLE_RATE, degrees=degrees, warps=(1.0, 0.85))
    with pytest.raises(ValueError):
        h.process_tuned(x, FM.SAMPLE_RATE, degrees=degrees, warps=(1.0, 0.85, 2.5))
    h.close()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_choir_example_plays_a_third_below_at_half_tempo_and_its_pieces_equal_the_whole(tmp_path):
    import test_choir_abi as TCA
    exe = TCA.build_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    print(j)
    assert j["one_call_equals_three_pieces"] is True and abs(j["output_samples"] - 2 * j["samples"]) <= 2 * 1024 - 3 and all(g > 50 for g in j["grains"])
    assert j["mirrored"] > 10 and j["mirrored_and_warped"] > 5
    assert abs(j["note_hz"][0] - 220.0) < 0.5 and abs(j["ratios"][1] / j["ratios"][0] - 2.0 ** (-4 / 12)) < 1e-5          # A3 and, two degrees of C major below, F3
    assert j["level"][1] > 3.0 * j["level_in_at_third_below"]                # the third below is in the output and was not in the input
