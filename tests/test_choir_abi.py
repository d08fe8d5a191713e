"""The pv_choir_* surface without a GPU: what the header declares is what the library exports and the binding types; calls without a handle and bad
configs are refused before any device; pv_choir_plan equals tests/choir_model.py, pv_mirror_plan and pv_formant_plan exactly; the host code of
psola/pv_choir.h and the planner run under AddressSanitizer and UBSan in a stand-alone program and print the model's tables; the kernel's resources; and
the example builds as pedantic C99."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import choir_model as CM
import psola_model as PM
import resource_usage as RU
import test_choir_model as TCM
import test_epoch_model as TEM
import test_formant_abi as TFA
import test_gpu_harmony as TGH
import test_gpu_tsm as TGT
import test_mirror_model as TMM
import test_psola_abi as TPA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
CSRC = os.path.join(ROOT, "phaze_amd", "csrc")
SURFACE = {"pv_choir_create": 2, "pv_choir_destroy": 1, "pv_choir_last_error": 1, "pv_choir_set_stream": 2, "pv_choir_synchronize": 1, "pv_choir_process": 13,
           "pv_choir_process_device": 13, "pv_choir_plan": 12}
DEVICE_POINTERS = {"pv_choir_process_device": (1, 9)}                        # void * in the binding
IP, DP, FP, LP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64)
STEP, BIT = CM.STEP, CM.MIRROR

_lib = TPA._lib
_has_gpu = TPA._has_gpu
_declaration = TPA._declaration


def test_header_declares_library_exports_and_binding_types_the_surface():
    import phaze_amd
    from phaze_amd import capi
    text = open(HEADER).read()
    declared = set(re.findall(r"PV_API\s+[\w ]+?\*?\s*\b(pv_choir_\w+)\s*\(", text))
    assert declared == set(SURFACE)
    assert set(SURFACE) <= set(capi.EXPORTS) and {n for n in capi.EXPORTS if n.startswith("pv_choir_")} == set(SURFACE)
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pv_\w+)", out))
    assert {n for n in exported if n.startswith("pv_choir_")} == set(SURFACE)
    assert exported == set(capi.EXPORTS)
    vp = C.c_void_p
    types = {"pv_choir *": vp, "const pv_choir *": vp, "pv_choir **": C.POINTER(vp), "const pv_choir_config *": C.POINTER(capi._ChoirConfig),
             "const pv_epoch_params *": C.POINTER(capi._EpochParams), "const pv_psola_params *": C.POINTER(capi._PsolaParams), "void *": vp, "const float *": FP,
             "float *": FP, "int32_t": C.c_int32, "int64_t": C.c_int64, "const int32_t *": IP, "int32_t *": IP, "const double *": DP, "int64_t *": LP,
             "const int64_t *": LP}
    for name, nargs in SURFACE.items():
        ret, decl = _declaration(name)
        got = getattr(L, name).argtypes
        assert len(got) == len(decl) == nargs, (name, decl)
        for i, (d, g) in enumerate(zip(decl, got)):
            want = vp if i in DEVICE_POINTERS.get(name, ()) else types[d]
            assert g == want, (name, i, d, g)
        assert getattr(L, name).restype == {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p}[ret], (name, ret)
    # the process calls take pv_harmony_process's argument lists
    for form in ("process", "process_device"):
        assert _declaration("pv_choir_" + form)[1][1:] == _declaration("pv_harmony_" + form)[1][1:]
        assert getattr(L, "pv_choir_" + form).argtypes == getattr(L, "pv_harmony_" + form).argtypes
    assert L.pv_abi_version() == capi.ABI_VERSION == 6 == int(re.search(r"#define PV_ABI_VERSION (\d+)", text).group(1))      # the change only adds
    note = text[text.index("#define PV_ABI_VERSION") - 2000:text.index("#define PV_ABI_VERSION")]
    assert "pv_choir_" in note and "pv_formant_" in note and "pv_contour_" in note and "6 = the time-stretch handle" in note
    assert C.sizeof(capi._ChoirConfig) == 32
    body = re.search(r"typedef struct pv_choir_config \{(.*?)\} pv_choir_config;", text, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+);", body, re.M)
    assert [(n, C.c_int32) for t, n in fields] == list(capi._ChoirConfig._fields_) and all(t == "int32_t" for t, _ in fields)
    assert [n for _, n in fields] == ["struct_size", "max_period", "max_rate", "max_voices", "max_channels", "max_outputs", "device_id", "flags"]     # pv_harmony_config's
    assert re.search(r"#define PV_CHOIR_CONFIG_INIT \{ \(int32_t\)sizeof\(pv_choir_config\), 0, 0, 0, 0, 0, 0, 0 \}", text)
    cfg = capi.make_choir_config(512, 2, 3, 4, 5, 6, 0)
    assert [getattr(cfg, n) for n, _ in capi._ChoirConfig._fields_] == [32, 512, 2, 3, 4, 5, 6, 0]
    for name in ("Choir", "choir_plan", "make_choir_config"):
        assert getattr(phaze_amd, name) is getattr(capi, name) and name in phaze_amd.__all__
    for method in ("process", "process_device", "process_tuned"):
        assert hasattr(capi.Choir, method)
    sig = inspect.signature(capi.Choir.process_tuned).parameters
    har = inspect.signature(capi.Harmony.process_tuned).parameters
    assert sig["warps"].default is None and sig["mirror"].default is False and sig["degrees"].default == (0, 2, 4) and sig["epochs"].default is False
    assert [k for k in sig if k not in ("warps", "mirror")] == list(har) and all(sig[k].default == har[k].default for k in har)
    assert list(inspect.signature(capi.Choir.__init__).parameters) == list(inspect.signature(capi.Harmony.__init__).parameters)
    sig = inspect.signature(capi.choir_plan).parameters
    assert sig["warps"].default is None and sig["mirror"].default is True
    assert [k for k in sig if k != "warps"] == list(inspect.signature(capi.mirror_plan).parameters)
    # the limits pv_formant_config states stay, and the new block says that pv_choir_* lifts them
    assert "no mirrored warped grains; pv_harmony_* and pv_takes_* keep unwarped grains" in text
    block = text[text.index("full-grain harmony voices on the overlap-add path"):text.index("typedef struct pv_choir_config")]
    assert "lifts the limits pv_formant_config states" in block


def test_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    x = (C.c_float * 8)()
    g = (C.c_int32 * 4)(4, BIT + 300 * STEP, 0, 2)
    first = (C.c_int64 * 2)(0, 1)
    w = (C.c_float * 1)(1.0)
    bad = capi.PV_ERR_ARGUMENT
    assert L.pv_choir_destroy(None) == bad and L.pv_choir_synchronize(None) == bad and L.pv_choir_set_stream(None, None) == bad
    assert L.pv_choir_process(None, x, 8, 8, 1, g, first, 1, w, x, 0, 8, 8) == bad
    assert L.pv_choir_process_device(None, None, 8, 8, 1, g, first, 1, w, None, 0, 8, 8) == bad
    assert L.pv_choir_create(None, None) == bad
    assert list(x) == [0.0] * 8


def test_config_errors_and_oversized_configs_appear_without_a_device():
    """pv_harmony_config's fields with pv_harmony_create's refusals; the span is pv_formant's, so PV_ERR_UNSUPPORTED begins exactly where the model says."""
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    h = C.c_void_p()

    def create(cfg):
        rc = L.pv_choir_create(C.byref(cfg), C.byref(h))
        return rc, L.pv_choir_last_error(None).decode()

    for (mp, rate), word in [((1, 1), "max_period"), ((0, 1), "max_period"), ((4097, 1), "max_period"), ((-3, 1), "max_period"), ((512, 0), "max_rate"),
                             ((512, 5), "max_rate"), ((512, -1), "max_rate")]:
        rc, msg = create(capi.make_choir_config(mp, rate))
        assert rc == capi.PV_ERR_ARGUMENT and word in msg, (mp, rate, msg)
    cfg = capi.make_choir_config(512, 2)
    cfg.struct_size -= 4
    rc, msg = create(cfg)
    assert rc == capi.PV_ERR_ARGUMENT and "struct_size" in msg
    cfg.struct_size += 8
    assert create(cfg)[0] == capi.PV_ERR_ARGUMENT
    rc, msg = create(capi.make_choir_config(512, 2, flags=1))
    assert rc == capi.PV_ERR_ARGUMENT and "flags" in msg
    for voices in (-1, 9):
        rc, msg = create(capi.make_choir_config(512, 2, max_voices=voices))
        assert rc == capi.PV_ERR_ARGUMENT and "max_voices" in msg
    rc, msg = create(capi.make_choir_config(512, 2, max_channels=-1))
    assert rc == capi.PV_ERR_ARGUMENT and "max_channels" in msg
    assert create(capi.make_choir_config(512, 2, max_channels=65536))[0] == capi.PV_ERR_ARGUMENT
    rc, msg = create(capi.make_choir_config(512, 2, max_outputs=-1))
    assert rc == capi.PV_ERR_ARGUMENT and "max_outputs" in msg
    fits = {(mp, rate): CM.fits(mp, rate) for mp in (2, 64, 1024, 1925, 1926, 2048, 2331, 2332, 2900, 2901, 3753, 3754, 4096) for rate in (1, 2, 3, 4)}
    assert fits[(3753, 1)] and not fits[(3754, 1)] and fits[(2900, 2)] and not fits[(2901, 2)] and fits[(2331, 3)] and not fits[(2332, 3)] and fits[(1925, 4)]
    assert not fits[(1926, 4)] and not fits[(4096, 1)] and not fits[(2048, 4)]
    for (mp, rate), ok in fits.items():
        rc, msg = create(capi.make_choir_config(mp, rate))
        if not ok:
            assert rc == capi.PV_ERR_UNSUPPORTED and "LDS" in msg and str(CM.lds_bytes(mp, rate)) in msg, (mp, rate, msg)
        elif not _has_gpu():
            assert rc == capi.PV_ERR_DEVICE and "HIP device" in msg, (mp, rate, msg)              # gets as far as the device and fails loudly: no CPU fallback
        else:
            assert rc == capi.PV_OK and L.pv_choir_destroy(h) == capi.PV_OK
    with pytest.raises(phaze_amd.PvError) as e:
        phaze_amd.Choir(4096, 1)
    assert e.value.status == capi.PV_ERR_UNSUPPORTED
    with pytest.raises(phaze_amd.PvError):
        phaze_amd.Choir(1)
    if not _has_gpu():
        with pytest.raises(phaze_amd.PvError):
            phaze_amd.Choir(512)


# ---- pure host code: the planner ----------------------------------------------------------------------------------------------------------------

_warps = TCM._warps


@pytest.mark.parametrize("seed", range(24))
def test_plan_equals_the_model_and_both_sibling_planners_exactly(seed):
    """The 24 random tracks of tests/test_mirror_model.py: pv_choir_plan is the model's choir_plan with ==; with warps = NULL it is pv_mirror_plan, with
    mirror = 0 pv_formant_plan; with both it differs from mirror_plan in L and in bits 17 .. 26 of w only."""
    import phaze_amd
    args, kw, mp, R = TMM.track(seed)
    nrec = np.asarray(args[0]).reshape(-1, 4).shape[0]
    ep = kw["epochs"] if kw["epochs"] is not None else TEM.random_epochs(np.random.default_rng(900 + seed), nrec)
    warps = _warps(seed, nrec)
    k = dict(kw, epochs=ep if seed % 2 else kw["epochs"])
    for mirror in (False, True):
        a, na = phaze_amd.choir_plan(*args, mirror=mirror, **k)                # the default is warps=None
        b, nb = phaze_amd.mirror_plan(*args, mirror=mirror, **k)
        assert a.dtype == np.int32 and np.array_equal(a, b) and na == nb
        want, want_len = CM.choir_plan(*args, warps=warps, mirror=mirror, **k)
        got, n = phaze_amd.choir_plan(*args, warps=warps, mirror=mirror, **k)
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want) and n == want_len, (seed, mirror)
        assert CM.check_grains(got, mp) is None and CM.warped(got).sum() > got.shape[0] // 2
    a, na = phaze_amd.choir_plan(*args, warps=warps, mirror=False, **k)
    b, nb = phaze_amd.formant_plan(*args, warps=warps, **k)
    assert np.array_equal(a, b) and na == nb
    full, n = phaze_amd.choir_plan(*args, warps=warps, **k)                    # the default is mirror=True
    mi, _ = phaze_amd.mirror_plan(*args, **k)
    assert np.array_equal(full[:, [0, 2]], mi[:, [0, 2]]) and np.array_equal(full[:, 1] & 0x1FFFF, mi[:, 1]) and np.any(full[:, 3] != mi[:, 3])
    assert np.array_equal(full[:, 3], b[:, 3]) and np.array_equal(full[:, 1] >> 17, b[:, 1] >> 17)


def _raw_plan():
    from phaze_amd import capi
    L = _lib()
    recs = np.ascontiguousarray(PM.records_of([217.3] * 30 + [-60.0] * 70))
    nrec = recs.shape[0]
    ratios = np.full(nrec, 1.25)
    rates = np.full(nrec, 0.5)
    warps = np.full(nrec, 1.25)
    ep = np.ascontiguousarray(TEM.random_epochs(np.random.default_rng(5), nrec))
    return capi, L, recs, nrec, ratios, rates, warps, ep


def test_plan_sizes_in_two_calls_and_writes_no_more_than_the_capacity():
    capi, L, recs, nrec, ratios, rates, warps, ep = _raw_plan()
    want, want_len = CM.choir_plan(recs, 64, 32, 6400, 128.0, 32, 512, ratios=ratios, rates=rates, warps=warps, epochs=ep)
    assert CM.warped(want).all() and (CM.mirrored(want) & CM.warped(want)).sum() > 20
    p = capi.make_psola_params(64, 32, 6400, 128.0, 32, 512)
    e = capi.make_epoch_params()
    rp, qp, sp, wp, ep_ = recs.ctypes.data_as(IP), ratios.ctypes.data_as(DP), rates.ctypes.data_as(DP), warps.ctypes.data_as(DP), ep.ctypes.data_as(IP)
    n_out = C.c_int64(-7)
    n = L.pv_choir_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, wp, ep_, 1, None, 0, C.byref(n_out))
    assert n == want.shape[0] > 50 and n_out.value == want_len
    g = np.full((n + 4, 4), -7, np.int32)
    assert L.pv_choir_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, wp, ep_, 1, g.ctypes.data_as(IP), n - 5, None) == n     # output_len may be NULL
    assert np.array_equal(g[:n - 5], want[:n - 5]) and np.all(g[n - 5:] == -7)
    assert L.pv_choir_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, wp, ep_, 1, g.ctypes.data_as(IP), n + 4, C.byref(n_out)) == n
    assert np.array_equal(g[:n], want) and np.all(g[n:] == -7) and n_out.value == want_len


def test_plan_rejects_every_bad_argument():
    """What either planner refuses: pv_formant_plan's list, and pv_mirror_plan's mirror other than 0 or 1."""
    import phaze_amd
    capi, L, recs, nrec, _, _, _, ep = _raw_plan()
    rp = recs.ctypes.data_as(IP)
    g = np.zeros((2048, 4), np.int32)
    gp = g.ctypes.data_as(IP)
    ones = np.ones(nrec)
    bad = -capi.PV_ERR_ARGUMENT
    n_out = C.c_int64(-7)

    def plan(records=rp, n=nrec, ratios=None, rates=None, warps=None, epochs=ep, mirror=1, out=gp, capacity=2048, struct_delta=0, reserved=0, e_delta=0,
             min_strength=0, lock=0.125, no_e=False, **kw):
        args = dict(f0_hop=64, f0_center=32, input_len=6400, unvoiced_period=128.0, min_period=32, max_period=512)
        args.update(kw)
        p = capi.make_psola_params(**args)
        p.struct_size += struct_delta
        p.reserved = reserved
        e = capi.make_epoch_params(min_strength, lock)
        e.struct_size += e_delta
        return L.pv_choir_plan(C.byref(p), None if no_e else C.byref(e), records, n, None if ratios is None else ratios.ctypes.data_as(DP),
                               None if rates is None else rates.ctypes.data_as(DP), None if warps is None else warps.ctypes.data_as(DP),
                               None if epochs is None else epochs.ctypes.data_as(IP), mirror, out, capacity, C.byref(n_out))

    assert plan() == CM.choir_plan(recs, 64, 32, 6400, 128.0, 32, 512, epochs=ep)[0].shape[0] and n_out.value == 6400
    assert L.pv_choir_plan(None, C.byref(capi.make_epoch_params()), rp, nrec, None, None, None, None, 1, gp, 2048, None) == bad
    g[:] = 0
    n_out.value = -7
    two, nan, zero, inf, low, high = ones.copy(), ones.copy(), ones.copy(), ones.copy(), ones.copy(), ones.copy()
    two[7], nan[0], zero[3], inf[nrec - 1], low[11], high[nrec - 2] = 2.0000001, np.nan, 0.0, np.inf, 0.49, 2.01
    for kw in (dict(struct_delta=8), dict(struct_delta=-8), dict(reserved=1), dict(records=None), dict(n=-1), dict(out=None), dict(capacity=-1), dict(f0_hop=0),
               dict(min_period=1), dict(min_period=0), dict(max_period=4097), dict(min_period=600, max_period=500, unvoiced_period=550.0), dict(unvoiced_period=31.9),
               dict(unvoiced_period=512.5), dict(unvoiced_period=float("nan")), dict(input_len=-1), dict(input_len=1 << 30), dict(ratios=two), dict(ratios=nan),
               dict(ratios=ones * 0.49), dict(ratios=-ones), dict(rates=nan), dict(rates=zero), dict(rates=-ones), dict(rates=inf), dict(no_e=True), dict(e_delta=8),
               dict(e_delta=-8), dict(min_strength=-1), dict(min_strength=16385), dict(lock=0.0), dict(lock=-0.5), dict(lock=1.0000001), dict(lock=float("nan")),
               dict(lock=float("inf")), dict(warps=low), dict(warps=high), dict(warps=nan), dict(warps=two), dict(warps=zero), dict(warps=-ones), dict(warps=inf),
               dict(warps=ones * 0.49), dict(warps=ones * 2.01), dict(mirror=2), dict(mirror=-1), dict(mirror=256)):
        assert plan(**kw) == bad, kw
    assert not g.any() and n_out.value == -7                                # nothing written by a refused call
    assert plan(input_len=(1 << 30) - 1, rates=ones * 0.25, epochs=None, out=None, capacity=0, max_period=4096, unvoiced_period=4096.0, min_period=2048) == bad
    assert plan(records=None, n=0, epochs=None) == CM.choir_plan(np.zeros((0, 4), np.int32), 64, 32, 6400, 128.0, 32, 512)[0].shape[0]
    assert plan(out=None, capacity=0) == plan() == plan(warps=ones) == plan(warps=ones * 0.5) == plan(warps=ones * 2.0, mirror=0)     # the marks depend on neither
    for kw in (dict(warps=ones[:-1]), dict(warps=low), dict(warps=nan)):
        with pytest.raises(ValueError):
            phaze_amd.choir_plan(recs, 64, 32, 6400, 128.0, 32, 512, **kw)


# ---- pure host code under AddressSanitizer and UBSan: the stand-alone driver ---------------------------------------------------------------------------

SAN = TFA.SAN
ENV = TFA.ENV
WHY = TFA.WHY
_driver = {}


def driver(tmp_path_factory):
    """The stand-alone program: tests/sanitize/choir_host.cpp with the planner and the one host function it calls, host code only, under ASan and UBSan.  It
    runs as a plain child process; nothing is loaded into python and nothing is preloaded."""
    if "exe" not in _driver:
        exe = str(tmp_path_factory.mktemp("choir_host") / "choir_host")
        cmd = [RU.HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-x", "hip", "-std=c++17"] + SAN + [
            os.path.join(ROOT, "tests", "sanitize", "choir_host.cpp"), os.path.join(CSRC, "psola", "pv_choir_plan.hip"), os.path.join(CSRC, "stretch", "pv_tune_plan.hip"),
            "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        _driver["exe"] = exe
    return _driver["exe"]


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=ENV, timeout=300)
    txt = r.stdout + r.stderr
    assert "AddressSanitizer" not in txt and "runtime error:" not in txt and "LeakSanitizer" not in txt, txt[-3000:]
    assert r.returncode == 0, (r.returncode, txt[-2000:])
    return r.stdout.split("\n")


def _tiles(exe, path, g, mp, first, nout):
    """What the driver says about one voice's table: ("bad", index, why) or ("tiles", int64[ntiles, 4], the int32 src0 per tile)."""
    g = np.ascontiguousarray(g, np.int32).reshape(-1, 4)
    g.tofile(path)
    lines = [ln for ln in _run(exe, "tiles", path, g.shape[0], mp, first, nout) if ln]
    if lines and lines[0].startswith("bad"):
        _, k, why = lines[0].split()
        return "bad", int(k), WHY[int(why)]
    rows = np.array([[int(v) for v in ln.split()] for ln in lines], np.int64).reshape(-1, 5)
    return "tiles", rows[:, :4], rows[:, 4]


@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_validation_and_tile_walk_equal_the_model_exactly_under_sanitizers(tmp_path_factory, tmp_path):
    """pv_choir.h's check, walk and src0, the text pv_choir_process runs per voice, against choir_model.check_grains and choir_model.tiles with ==: the tables of
    tests/test_gpu_tsm.py plain, with every third grain of each kind and with all grains mirrored and warped; calls from output 0, from an odd output and
    near 2^30; the int32 corners of src0; every refusal with the model's index and reason."""
    exe = driver(tmp_path_factory)
    path = str(tmp_path / "grains.bin")
    checked = 0
    for name in ("small", "mid", "big", "tiny", "huge", "sweep", "gap", "empty", "slow", "fast"):
        mp, R, nin, g = TGT._grains(name)
        for table in (g, TCM.full_table(g, "thirds"), TCM.full_table(g, "all")):
            assert CM.check_grains(table, mp) is None
            for first, nout in ((0, TGT.NOUT), (777, TGT.NOUT - 777), (1024, 1), (5, 0)):
                kind, got, src0 = _tiles(exe, path, table, mp, first, nout)
                want = CM.tiles(table, mp, first, nout)
                assert kind == "tiles" and got.shape == want.shape and np.array_equal(got, want), (name, first)
                assert np.array_equal(src0, want[:, 2])
                checked += want.shape[0]
        full = TCM.full_table(g, "all")
        assert g.shape[0] < 3 or ((CM.mirrored(full) & CM.warped(full)).all() and (CM.mirrored(TCM.full_table(g, "thirds")) & CM.warped(TCM.full_table(g, "thirds"))).any())
    assert checked > 150
    # a planned table with mirrored warped grains
    args, kw, mp, R = TMM.track(5)
    nrec = np.asarray(args[0]).reshape(-1, 4).shape[0]
    g, n = CM.choir_plan(*args, warps=_warps(5, nrec), **kw)
    kind, got, _ = _tiles(exe, path, g, mp, 0, n)
    assert kind == "tiles" and np.array_equal(got, CM.tiles(g, mp, 0, n)) and (CM.mirrored(g) & CM.warped(g)).any()
    # the far ends: outputs near 2^30 with D at either end of its range, all four kinds; src0 comes within a few thousand of +-2^31 and, as uploaded, still is itself
    top = (1 << 30) - 1
    far = np.array([[top - 2000, 512 * STEP + 7, 1 - (1 << 30), 64], [top - 1500, BIT + 128 * STEP + 256 * 200, (1 << 31) - 1, 64], [top - 40, BIT + 300 * STEP, top + 5, 64],
                    [top, BIT + 5, (1 << 31) - 1, 64]])
    assert CM.check_grains(far, 64) is None
    kind, got, src0 = _tiles(exe, path, far, 64, top - 3000, 3001)
    want = CM.tiles(far, 64, top - 3000, 3001)
    assert kind == "tiles" and np.array_equal(got, want)
    assert (1 << 31) - 3000 < want[:, 2].max() < 1 << 31 and np.array_equal(src0, want[:, 2])
    # the corners where src0 leaves int32, and the upload carries its low 32 bits: above, a tile that begins past the centre of a compressed forward grain with
    # D = 1 - 2^30; below, a mirrored grain (plain, and compressed) with D = 1 - 2^30 on outputs near 2^30
    past = np.array([[top - 1000, 512 * STEP, 1 - (1 << 30), 1000]])
    kind, got, src0 = _tiles(exe, path, past, 1024, top - 10, 11)
    want = CM.tiles(past, 1024, top - 10, 11)
    assert kind == "tiles" and np.array_equal(got, want) and want[0, 2] >= 1 << 31 and src0[0] == want[0, 2] - (1 << 32)
    for word in (BIT, BIT + 512 * STEP + 256 * 9 + 3):
        below = np.array([[top - 500, word, 1 - (1 << 30), 1000]])
        kind, got, src0 = _tiles(exe, path, below, 1024, top - 900, 901)
        want = CM.tiles(below, 1024, top - 900, 901)
        assert kind == "tiles" and np.array_equal(got, want) and want[0, 2] < -(1 << 31) and src0[0] == want[0, 2] + (1 << 32)
    # every refusal, with the model's index and reason
    mp, R, nin, g = TGT._grains("small")
    last = g.shape[0] - 1
    for table in (g, TCM.full_table(g, "thirds")):
        fwd, mir = int(np.flatnonzero(~CM.mirrored(table))[3]), int(np.flatnonzero(CM.mirrored(table))[3]) if CM.mirrored(table).any() else 11
        for idx, col, val in [(7, 3, 1), (7, 3, mp + 1), (0, 0, -1), (5, 0, 1 << 30), (9, 1, 1 << 27), (9, 1, -1), (9, 1, 127 * STEP), (9, 1, STEP), (9, 1, 513 * STEP + 3),
                              (9, 1, 1023 * STEP), (9, 1, BIT + 127 * STEP), (9, 1, BIT + 513 * STEP), (fwd, 2, 1 << 30), (fwd, 2, -(1 << 30)), (mir, 2, -(1 << 30)),
                              (last, 0, 5), (20, 0, int(g[19, 0]) - 1)]:
            bad = np.array(table, np.int64)
            bad[idx, col] = val
            want = CM.check_grains(bad, mp)
            assert want is not None and want[0] == idx, (idx, col, val, want)
            assert _tiles(exe, path, bad, mp, 0, TGT.NOUT) == ("bad",) + want, (idx, col, val)
        ok = np.array(table, np.int64)
        if CM.mirrored(table).any():                                           # a mirrored D of 2^30 and of the largest int32 is legal
            ok[mir, 2] = 1 << 30
            assert CM.check_grains(ok, mp) is None and _tiles(exe, path, ok, mp, 0, 1)[0] == "tiles"


@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_the_planner_runs_clean_under_sanitizers_and_gives_the_models_grains(tmp_path_factory, tmp_path):
    """The driver sizes in two calls into a buffer of exactly the capacity, and again into a smaller one; warps and mirror on and off."""
    exe = driver(tmp_path_factory)
    path = str(tmp_path / "track.bin")
    both = 0
    for seed in (3, 5, 10, 17, 23):
        args, kw, mp, R = TMM.track(seed)
        recs = np.ascontiguousarray(args[0], np.int32).reshape(-1, 4)
        nrec = recs.shape[0]
        ep = kw["epochs"] if kw["epochs"] is not None else np.zeros((nrec, 4), np.int32)
        warps = _warps(seed, nrec)
        with open(path, "wb") as f:
            for a in (recs, np.ascontiguousarray(kw["ratios"], np.float64), np.ascontiguousarray(kw["rates"], np.float64), warps, np.ascontiguousarray(ep, np.int32)):
                f.write(a.tobytes())
        for with_warps, mirror in ((0, 0), (0, 1), (1, 0), (1, 1)):
            lines = [ln for ln in _run(exe, "plan", path, nrec, args[1], args[2], args[3], repr(args[4]), args[5], args[6], with_warps, int(kw["epochs"] is not None), 0,
                                       repr(kw["lock"]), mirror) if ln]
            want, want_len = CM.choir_plan(*args, warps=warps if with_warps else None, mirror=bool(mirror), **kw)
            assert lines[0].split() == ["n", str(want.shape[0]), str(want_len)]
            got = np.array([[int(v) for v in ln.split()] for ln in lines[1:]], np.int64).reshape(-1, 4)
            assert np.array_equal(got, want), (seed, with_warps, mirror)
            both += int((CM.mirrored(got) & CM.warped(got)).sum())
    assert both > 10
    # refused plans
    with open(path, "wb") as f:
        f.write(np.zeros(0, np.int32).tobytes())
    assert _run(exe, "plan", path, 0, 64, 32, 1 << 30, "128.0", 32, 512, 1, 0, 0, "0.125", 1)[0] == "refused -2"
    assert _run(exe, "plan", path, 0, 64, 32, 1000, "128.0", 32, 512, 1, 0, 0, "0.125", 2)[0] == "refused -2"


# ---- kernel resources -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_choir_kernel_uses_no_spill_no_scratch_no_agprs():
    """One kernel, pv_choir_kernel: no spill, no scratch, no AGPRs, no static LDS beside the dynamic arrays, at most 128 VGPRs (occupancy here is set by the LDS
    of a launch, not by registers); DESIGN.md "Choir" quotes its figures."""
    kernels = RU.resources("psola/pv_choir_kernels.hip")
    assert len(kernels) == 1 and all("pv_choir_kernel" in n for n in kernels), sorted(kernels)
    for n, v in kernels.items():
        print(n, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs"] <= 128 and v["LDS Size"] == 0, (n, v)


def test_the_new_files_stand_beside_the_existing_overlap_add_kernels():
    """The kernel file restates the sibling arithmetic in its own file: it and its contract include none of the other overlap-add files and name none of their
    kernels or launchers, and use no inline assembly of their own (the mix's rounded product comes from pv_mul_rounded.h, as in the harmony kernel)."""
    src = open(os.path.join(CSRC, "psola", "pv_choir_kernels.hip")).read()
    includes = re.findall(r'#include "([^"]+)"', src)
    assert "pv_choir.h" in includes and "../pv_mul_rounded.h" in includes and not any(i.endswith(".hip") for i in includes)
    assert not {"pv_psola.h", "pv_epoch.h", "pv_harmony.h", "pv_takes.h", "pv_mirror.h", "pv_formant.h"} & set(includes)
    contract = re.findall(r'#include "([^"]+)"', open(os.path.join(CSRC, "psola", "pv_choir.h")).read())
    assert contract == ["pv_tsm.h"]
    for host in ("pv_choir_capi.hip", "pv_choir_plan.hip"):
        inc = re.findall(r'#include "([^"]+)"', open(os.path.join(CSRC, "psola", host)).read())
        assert "pv_choir.h" in inc and not {"pv_harmony.h", "pv_mirror.h", "pv_formant.h", "pv_takes.h"} & set(inc)
    code = re.sub(r"//.*", "", src)
    for name in ("pv_psola_kernel", "pv_epoch_kernel", "pv_tsm_kernel", "pv_harmony_kernel", "pv_takes_kernel", "pv_mirror_kernel", "pv_formant_kernel", "pv_launch_tsm",
                 "pv_launch_psola", "pv_launch_harmony", "pv_launch_takes", "pv_launch_mirror", "pv_launch_formant", "asm"):
        assert name not in code, name
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "pv_choir_kernels.hip" in make.split("stretch-resource-usage:")[1]
    assert all(f"psola/pv_choir_{part}" in make.split("OBJS =")[0] for part in ("kernels.hip", "capi.hip", "plan.hip")) and "psola/pv_choir.h" in make
    lib = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    assert "pv_launch_choir" not in re.findall(r" T (\w+)", lib)              # the launcher is not an export: every new symbol starts with pv_choir_


# ---- the example ------------------------------------------------------------------------------------------------------------------------------

def build_example(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_choir")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_choir.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_choir_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_example(tmp_path)
    if not _has_gpu():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device" in (r.stdout + r.stderr)
