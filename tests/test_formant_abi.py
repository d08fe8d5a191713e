"""CPU checks of the formant-shifting surface: the header declares, the library exports and the ctypes binding gives argument types to every pv_formant_* name,
the ABI stays 6, bad and oversized configs are refused before any device is touched, pv_formant_plan equals the Python model (tests/formant_model.py) bit
for bit, sizes in two calls and refuses every bad argument, the validation and the tile walk of pv_formant.h equal the model's with ==, the kernel file
compiles for gfx950 without spills, scratch or AGPRs, and examples/pv_formant.c builds as pedantic C99 (tests/test_gpu_formant.py runs it, and holds the
refusals of pv_formant_process, which need a handle).  The planner, the validation and the tile walk also run in a stand-alone program
(tests/sanitize/formant_host.cpp) built with AddressSanitizer and UBSan: host code only, nothing of it is loaded into this process."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import formant_model as FoM
import psola_model as PM
import resource_usage as RU
import test_epoch_model as TEM
import test_gpu_tsm as TGT
import test_mirror_model as TMM
import test_psola_abi as TPA
import tsm_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
CSRC = os.path.join(ROOT, "phaze_amd", "csrc")
SURFACE = {"pv_formant_create": 2, "pv_formant_destroy": 1, "pv_formant_last_error": 1, "pv_formant_set_stream": 2, "pv_formant_synchronize": 1, "pv_formant_process": 11,
           "pv_formant_process_device": 11, "pv_formant_plan": 11}
DEVICE_POINTERS = {"pv_formant_process_device": (1, 7)}                      # void * in the binding
IP, DP, FP, LP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64)
STEP = FoM.STEP
STEPS = (128, 129, 200, 255, 257, 300, 511, 512)

_lib = TPA._lib
_has_gpu = TPA._has_gpu
_declaration = TPA._declaration


def warp_table(g, every=3, start=1):
    """The table g with every `every`-th grain warped: steps drawn in turn from STEPS, phi forced through 0, 1, 255 and the table's own value, tf through 0, 255
    and its own value where that keeps the centres in order (a grain whose neighbours sit on other whole positions)."""
    m = np.array(g, np.int64).reshape(-1, 4)
    k = np.arange(start, m.shape[0], every)
    tf, phi = m[:, 1] & 255, (m[:, 1] >> 8) & 255
    for j, i in enumerate(k.tolist()):
        if j % 4 < 3:
            phi[i] = (0, 1, 255)[j % 4]
        alone = (i == 0 or m[i - 1, 0] < m[i, 0]) and (i == m.shape[0] - 1 or m[i + 1, 0] > m[i, 0])
        if alone and (j // 4) % 3 < 2:
            tf[i] = (0, 255)[(j // 4) % 3]
    m[:, 1] = tf + 256 * phi
    m[k, 1] += STEP * np.array(STEPS)[np.arange(k.size) % len(STEPS)]
    return np.ascontiguousarray(m, np.int32)


def test_header_declares_library_exports_and_binding_types_the_surface():
    import phaze_amd
    from phaze_amd import capi
    text = open(HEADER).read()
    declared = set(re.findall(r"PV_API\s+[\w ]+?\*?\s*\b(pv_formant_\w+)\s*\(", text))
    assert declared == set(SURFACE)
    assert set(SURFACE) <= set(capi.EXPORTS)
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pv_\w+)", out))
    assert set(SURFACE) <= exported and {n for n in exported if n.startswith("pv_formant_")} == set(SURFACE)
    assert exported == set(capi.EXPORTS)
    vp = C.c_void_p
    types = {"pv_formant *": vp, "const pv_formant *": vp, "pv_formant **": C.POINTER(vp), "const pv_formant_config *": C.POINTER(capi._FormantConfig),
             "const pv_epoch_params *": C.POINTER(capi._EpochParams), "const pv_psola_params *": C.POINTER(capi._PsolaParams), "void *": vp, "const float *": FP,
             "float *": FP, "int32_t": C.c_int32, "int64_t": C.c_int64, "const int32_t *": IP, "int32_t *": IP, "const double *": DP, "int64_t *": LP}
    for name, nargs in SURFACE.items():
        ret, decl = _declaration(name)
        got = getattr(L, name).argtypes
        assert len(got) == len(decl) == nargs, (name, decl)
        for i, (d, g) in enumerate(zip(decl, got)):
            want = vp if i in DEVICE_POINTERS.get(name, ()) else types[d]
            assert g == want, (name, i, d, g)
        assert getattr(L, name).restype == {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p}[ret], (name, ret)
    assert L.pv_abi_version() == capi.ABI_VERSION == 6 == int(re.search(r"#define PV_ABI_VERSION (\d+)", text).group(1))      # the change only adds
    note = text[text.index("#define PV_ABI_VERSION") - 2000:text.index("#define PV_ABI_VERSION")]
    assert "pv_formant_" in note and "pv_mirror_" in note
    assert C.sizeof(capi._FormantConfig) == 28
    body = re.search(r"typedef struct pv_formant_config \{(.*?)\} pv_formant_config;", text, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+);", body, re.M)
    assert [(n, C.c_int32) for t, n in fields] == list(capi._FormantConfig._fields_) and all(t == "int32_t" for t, _ in fields)
    assert [n for _, n in fields] == ["struct_size", "max_period", "max_rate", "max_channels", "max_outputs", "device_id", "flags"]      # pv_tsm_config's
    assert re.search(r"#define PV_FORMANT_CONFIG_INIT \{ \(int32_t\)sizeof\(pv_formant_config\), 0, 0, 0, 0, 0, 0 \}", text)
    for name in ("Formant", "formant_plan"):
        assert getattr(phaze_amd, name) is getattr(capi, name) and name in phaze_amd.__all__
    for method in ("process", "process_device", "process_tuned"):
        assert hasattr(capi.Formant, method)
    sig = inspect.signature(capi.Formant.process_tuned).parameters
    tsm = inspect.signature(capi.Tsm.process_tuned).parameters
    assert sig["warp"].default == 1.0 and [k for k in sig if k != "warp"] == list(tsm) and all(sig[k].default == tsm[k].default for k in tsm)
    sig = inspect.signature(capi.Formant.__init__).parameters
    assert list(sig)[1:] == ["max_period", "max_rate", "max_channels", "max_outputs", "device_id"] and sig["max_rate"].default == 2
    sig = inspect.signature(capi.formant_plan).parameters
    assert sig["warps"].default is None and [k for k in sig if k != "warps"] == list(inspect.signature(capi.tsm_plan).parameters)


def test_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    x = (C.c_float * 8)()
    g = (C.c_int32 * 4)(4, 300 * STEP, 0, 2)
    bad = capi.PV_ERR_ARGUMENT
    assert L.pv_formant_destroy(None) == bad and L.pv_formant_synchronize(None) == bad and L.pv_formant_set_stream(None, None) == bad
    assert L.pv_formant_process(None, x, 8, 8, 1, g, 1, x, 0, 8, 8) == bad
    assert L.pv_formant_process_device(None, None, 8, 8, 1, g, 1, None, 0, 8, 8) == bad
    assert L.pv_formant_create(None, None) == bad
    assert list(x) == [0.0] * 8


def test_config_errors_and_oversized_configs_appear_without_a_device():
    """pv_tsm_config's fields with pv_tsm_create's refusals; the span is wider than pv_tsm's, so PV_ERR_UNSUPPORTED begins earlier: exactly where the model says."""
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    h = C.c_void_p()

    def create(cfg):
        rc = L.pv_formant_create(C.byref(cfg), C.byref(h))
        return rc, L.pv_formant_last_error(None).decode()

    for (mp, rate), word in [((1, 1), "max_period"), ((0, 1), "max_period"), ((4097, 1), "max_period"), ((-3, 1), "max_period"), ((512, 0), "max_rate"),
                             ((512, 5), "max_rate"), ((512, -1), "max_rate")]:
        rc, msg = create(capi.make_formant_config(mp, rate))
        assert rc == capi.PV_ERR_ARGUMENT and word in msg, (mp, rate, msg)
    cfg = capi.make_formant_config(512, 2)
    cfg.struct_size -= 4
    rc, msg = create(cfg)
    assert rc == capi.PV_ERR_ARGUMENT and "struct_size" in msg
    cfg.struct_size += 8
    assert create(cfg)[0] == capi.PV_ERR_ARGUMENT
    rc, msg = create(capi.make_formant_config(512, 2, flags=1))
    assert rc == capi.PV_ERR_ARGUMENT and "flags" in msg
    rc, msg = create(capi.make_formant_config(512, 2, max_channels=-1))
    assert rc == capi.PV_ERR_ARGUMENT and "max_channels" in msg
    assert create(capi.make_formant_config(512, 2, max_channels=65536))[0] == capi.PV_ERR_ARGUMENT
    rc, msg = create(capi.make_formant_config(512, 2, max_outputs=-1))
    assert rc == capi.PV_ERR_ARGUMENT and "max_outputs" in msg
    fits = {(mp, rate): FoM.fits(mp, rate) for mp in (2, 64, 1024, 1925, 1926, 2048, 2331, 2332, 2900, 2901, 3753, 3754, 4096) for rate in (1, 2, 3, 4)}
    assert fits[(3753, 1)] and not fits[(3754, 1)] and fits[(2900, 2)] and not fits[(2901, 2)] and fits[(2331, 3)] and not fits[(2332, 3)] and fits[(1925, 4)]
    assert not fits[(1926, 4)] and not fits[(4096, 1)] and not fits[(2048, 4)]
    for (mp, rate), ok in fits.items():
        rc, msg = create(capi.make_formant_config(mp, rate))
        if not ok:
            assert rc == capi.PV_ERR_UNSUPPORTED and "LDS" in msg and str(FoM.lds_bytes(mp, rate)) in msg, (mp, rate, msg)
        elif not _has_gpu():
            assert rc == capi.PV_ERR_DEVICE and "HIP device" in msg, (mp, rate, msg)              # gets as far as the device and fails loudly: no CPU fallback
        else:
            assert rc == capi.PV_OK and L.pv_formant_destroy(h) == capi.PV_OK
    with pytest.raises(phaze_amd.PvError) as e:
        phaze_amd.Formant(4096, 1)
    assert e.value.status == capi.PV_ERR_UNSUPPORTED
    with pytest.raises(phaze_amd.PvError):
        phaze_amd.Formant(1)
    if not _has_gpu():
        with pytest.raises(phaze_amd.PvError):
            phaze_amd.Formant(512)


# ---- pure host code: the planner ----------------------------------------------------------------------------------------------------------------

def _warps(seed, nrec):
    w = np.random.default_rng(700 + seed).uniform(0.5, 2.0, nrec)
    w[::7] = 1.0
    w[1::7] = 0.5
    w[2::7] = 2.0
    return w


@pytest.mark.parametrize("seed", [3, 5, 10, 17, 23])
def test_plan_equals_the_model_exactly(seed):
    """Five of the random tracks of tests/test_mirror_model.py, with and without epoch records: warps=None is pv_tsm_plan's and the model's bits, a row the
    model's."""
    import phaze_amd
    args, kw, mp, R = TMM.track(seed)
    nrec = np.asarray(args[0]).reshape(-1, 4).shape[0]
    ep = kw["epochs"] if kw["epochs"] is not None else TEM.random_epochs(np.random.default_rng(900 + seed), nrec)
    warps = _warps(seed, nrec)
    for epochs in (None, ep):
        k = dict(kw, epochs=epochs)
        base, base_len = phaze_amd.tsm_plan(*args, **k)
        got, n = phaze_amd.formant_plan(*args, **k)                            # the default is warps=None
        assert got.dtype == np.int32 and np.array_equal(got, base) and n == base_len
        want, want_len = FoM.formant_plan(*args, warps=warps, **k)
        got, n = phaze_amd.formant_plan(*args, warps=warps, **k)
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want) and n == want_len, (seed, epochs is None)
        assert FoM.check_grains(got, mp) is None and FoM.warped(got).sum() > got.shape[0] // 2


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
    want, want_len = FoM.formant_plan(recs, 64, 32, 6400, 128.0, 32, 512, ratios=ratios, rates=rates, warps=warps, epochs=ep)
    assert FoM.warped(want).all()
    p = capi.make_psola_params(64, 32, 6400, 128.0, 32, 512)
    e = capi.make_epoch_params()
    rp, qp, sp, wp, ep_ = recs.ctypes.data_as(IP), ratios.ctypes.data_as(DP), rates.ctypes.data_as(DP), warps.ctypes.data_as(DP), ep.ctypes.data_as(IP)
    n_out = C.c_int64(-7)
    n = L.pv_formant_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, wp, ep_, None, 0, C.byref(n_out))
    assert n == want.shape[0] > 50 and n_out.value == want_len
    g = np.full((n + 4, 4), -7, np.int32)
    assert L.pv_formant_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, wp, ep_, g.ctypes.data_as(IP), n - 5, None) == n     # output_len may be NULL
    assert np.array_equal(g[:n - 5], want[:n - 5]) and np.all(g[n - 5:] == -7)
    assert L.pv_formant_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, wp, ep_, g.ctypes.data_as(IP), n + 4, C.byref(n_out)) == n
    assert np.array_equal(g[:n], want) and np.all(g[n:] == -7) and n_out.value == want_len


def test_plan_rejects_every_bad_argument():
    import phaze_amd
    capi, L, recs, nrec, _, _, _, ep = _raw_plan()
    rp = recs.ctypes.data_as(IP)
    g = np.zeros((2048, 4), np.int32)
    gp = g.ctypes.data_as(IP)
    ones = np.ones(nrec)
    bad = -capi.PV_ERR_ARGUMENT
    n_out = C.c_int64(-7)

    def plan(records=rp, n=nrec, ratios=None, rates=None, warps=None, epochs=ep, out=gp, capacity=2048, struct_delta=0, reserved=0, e_delta=0, min_strength=0,
             lock=0.125, no_e=False, **kw):
        args = dict(f0_hop=64, f0_center=32, input_len=6400, unvoiced_period=128.0, min_period=32, max_period=512)
        args.update(kw)
        p = capi.make_psola_params(**args)
        p.struct_size += struct_delta
        p.reserved = reserved
        e = capi.make_epoch_params(min_strength, lock)
        e.struct_size += e_delta
        return L.pv_formant_plan(C.byref(p), None if no_e else C.byref(e), records, n, None if ratios is None else ratios.ctypes.data_as(DP),
                                 None if rates is None else rates.ctypes.data_as(DP), None if warps is None else warps.ctypes.data_as(DP),
                                 None if epochs is None else epochs.ctypes.data_as(IP), out, capacity, C.byref(n_out))

    assert plan() == FoM.formant_plan(recs, 64, 32, 6400, 128.0, 32, 512, epochs=ep)[0].shape[0] and n_out.value == 6400
    assert L.pv_formant_plan(None, C.byref(capi.make_epoch_params()), rp, nrec, None, None, None, None, gp, 2048, None) == bad
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
               dict(warps=ones * 0.49), dict(warps=ones * 2.01)):
        assert plan(**kw) == bad, kw
    assert not g.any() and n_out.value == -7                                # nothing written by a refused call
    assert plan(input_len=(1 << 30) - 1, rates=ones * 0.25, epochs=None, out=None, capacity=0, max_period=4096, unvoiced_period=4096.0, min_period=2048) == bad
    assert plan(records=None, n=0, epochs=None) == FoM.formant_plan(np.zeros((0, 4), np.int32), 64, 32, 6400, 128.0, 32, 512)[0].shape[0]
    assert plan(out=None, capacity=0) == plan() == plan(warps=ones) == plan(warps=ones * 0.5) == plan(warps=ones * 2.0)       # the marks do not depend on the warps
    with pytest.raises(ValueError):
        phaze_amd.formant_plan(recs, 64, 32, 6400, 128.0, 32, 512, warps=ones[:-1])
    with pytest.raises(ValueError):
        phaze_amd.formant_plan(recs, 64, 32, 6400, 128.0, 32, 512, warps=low)
    with pytest.raises(ValueError):
        phaze_amd.formant_plan(recs, 64, 32, 6400, 128.0, 32, 512, warps=nan)


# ---- pure host code under AddressSanitizer and UBSan: the stand-alone driver ---------------------------------------------------------------------------

SAN = ["-g", "-O1", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
WHY = {1: "centre", 2: "half length", 3: "shift", 4: "out of order", 5: "step"}
_driver = {}


def driver(tmp_path_factory):
    """The stand-alone program: tests/sanitize/formant_host.cpp with the planner and the one host function it calls, host code only, under ASan and UBSan."""
    if "exe" not in _driver:
        exe = str(tmp_path_factory.mktemp("formant_host") / "formant_host")
        cmd = [RU.HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-x", "hip", "-std=c++17"] + SAN + [
            os.path.join(ROOT, "tests", "sanitize", "formant_host.cpp"), os.path.join(CSRC, "psola", "pv_formant_plan.hip"), os.path.join(CSRC, "stretch", "pv_tune_plan.hip"),
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
    """What the driver says about a table: ("bad", index, why) or ("tiles", int64[ntiles, 4], the int32 src0 per tile)."""
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
    """pv_formant.h's check and walk, the text pv_formant_process runs, against formant_model.check_grains and formant_model.tiles with ==: the tables of
    tests/test_gpu_tsm.py unwarped, with every third grain warped and with all grains warped; calls from output 0, from an odd output and near 2^30; every
    refusal with the model's index and reason."""
    exe = driver(tmp_path_factory)
    path = str(tmp_path / "grains.bin")
    checked = 0
    for name in ("small", "mid", "big", "tiny", "huge", "sweep", "gap", "empty", "slow", "fast"):
        mp, R, nin, g = TGT._grains(name)
        for table in (g, warp_table(g), warp_table(g, 1, 0)):
            assert FoM.check_grains(table, mp) is None
            for first, nout in ((0, TGT.NOUT), (777, TGT.NOUT - 777), (1024, 1), (5, 0)):
                kind, got, src0 = _tiles(exe, path, table, mp, first, nout)
                want = FoM.tiles(table, mp, first, nout)
                assert kind == "tiles" and got.shape == want.shape and np.array_equal(got, want), (name, first)
                assert np.array_equal(src0, want[:, 2])
                checked += want.shape[0]
        assert g.shape[0] < 3 or (FoM.warped(warp_table(g)).sum() >= (g.shape[0] - 1) // 3 and FoM.warped(warp_table(g, 1, 0)).all())
    assert checked > 150
    # a planned table
    args, kw, mp, R = TMM.track(5)
    nrec = np.asarray(args[0]).reshape(-1, 4).shape[0]
    g, n = FoM.formant_plan(*args, warps=_warps(5, nrec), **kw)
    kind, got, _ = _tiles(exe, path, g, mp, 0, n)
    assert kind == "tiles" and np.array_equal(got, FoM.tiles(g, mp, 0, n)) and FoM.warped(g).any()
    # the far ends: outputs near 2^30 with D at either end of its range; src0 comes within a few thousand of 2^31 and, as uploaded, still is itself
    top = (1 << 30) - 1
    far = np.array([[top - 2000, 512 * STEP + 7, 1 - (1 << 30), 64], [top - 1500, 128 * STEP + 256 * 200, (1 << 30) - 1, 64], [top - 40, 300 * STEP, 1 - (1 << 30), 64],
                    [top, 5, (1 << 30) - 1, 64]])
    assert FoM.check_grains(far, 64) is None
    kind, got, src0 = _tiles(exe, path, far, 64, top - 3000, 3001)
    want = FoM.tiles(far, 64, top - 3000, 3001)
    assert kind == "tiles" and np.array_equal(got, want)
    assert (1 << 31) - 3000 < want[:, 2].max() < 1 << 31 and np.array_equal(src0, want[:, 2])
    # the one corner where src0 leaves int32: a tile that begins past the centre of a compressed grain with D = 1 - 2^30; the upload carries its low 32 bits
    past = np.array([[top - 1000, 512 * STEP, 1 - (1 << 30), 1000]])
    kind, got, src0 = _tiles(exe, path, past, 1024, top - 10, 11)
    want = FoM.tiles(past, 1024, top - 10, 11)
    assert kind == "tiles" and np.array_equal(got, want) and want[0, 2] >= 1 << 31 and src0[0] == want[0, 2] - (1 << 32)
    # every refusal, with the model's index and reason
    mp, R, nin, g = TGT._grains("small")
    last = g.shape[0] - 1
    for idx, col, val in [(7, 3, 1), (7, 3, mp + 1), (0, 0, -1), (5, 0, 1 << 30), (9, 1, 1 << 27), (9, 1, -1), (9, 1, 127 * STEP), (9, 1, STEP), (9, 1, 513 * STEP + 3),
                          (9, 1, 1023 * STEP), (9, 1, 65536), (9, 1, 65536 + 300 * STEP), (11, 2, 1 << 30), (11, 2, -(1 << 30)), (last, 0, 5), (20, 0, int(g[19, 0]) - 1)]:
        for table in (g, warp_table(g)):
            bad = np.array(table, np.int64)
            bad[idx, col] = val
            want = FoM.check_grains(bad, mp)
            assert want is not None and want[0] == idx
            assert _tiles(exe, path, bad, mp, 0, TGT.NOUT) == ("bad",) + want, (idx, col, val)
    assert FoM.check_grains(np.array([[5, 1 << 27, 0, 9]]), 64)[1] == "step"


@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_the_planner_runs_clean_under_sanitizers_and_gives_the_models_grains(tmp_path_factory, tmp_path):
    """The driver sizes in two calls into a buffer of exactly the capacity, and again into a smaller one."""
    exe = driver(tmp_path_factory)
    path = str(tmp_path / "track.bin")
    warped = 0
    for seed in (3, 5, 10, 17, 23):
        args, kw, mp, R = TMM.track(seed)
        recs = np.ascontiguousarray(args[0], np.int32).reshape(-1, 4)
        nrec = recs.shape[0]
        ep = kw["epochs"] if kw["epochs"] is not None else np.zeros((nrec, 4), np.int32)
        warps = _warps(seed, nrec)
        with open(path, "wb") as f:
            for a in (recs, np.ascontiguousarray(kw["ratios"], np.float64), np.ascontiguousarray(kw["rates"], np.float64), warps, np.ascontiguousarray(ep, np.int32)):
                f.write(a.tobytes())
        for with_warps in (0, 1):
            lines = [ln for ln in _run(exe, "plan", path, nrec, args[1], args[2], args[3], repr(args[4]), args[5], args[6], with_warps, int(kw["epochs"] is not None), 0,
                                       repr(kw["lock"])) if ln]
            want, want_len = FoM.formant_plan(*args, warps=warps if with_warps else None, **kw)
            assert lines[0].split() == ["n", str(want.shape[0]), str(want_len)]
            got = np.array([[int(v) for v in ln.split()] for ln in lines[1:]], np.int64).reshape(-1, 4)
            assert np.array_equal(got, want), (seed, with_warps)
            warped += int(FoM.warped(got).sum())
    assert warped > 50
    # a refused plan
    with open(path, "wb") as f:
        f.write(np.zeros(0, np.int32).tobytes())
    assert _run(exe, "plan", path, 0, 64, 32, 1 << 30, "128.0", 32, 512, 1, 0, 0, "0.125")[0] == "refused -2"


# ---- kernel resources -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_formant_kernel_uses_no_spill_no_scratch_no_agprs():
    """One kernel, pv_formant_kernel: no spill, no scratch, no AGPRs, no static LDS beside the dynamic arrays, at most 128 VGPRs (occupancy here is set by the
    LDS of a launch, not by registers); DESIGN.md "Formant shifting" quotes its figures."""
    kernels = RU.resources("psola/pv_formant_kernels.hip")
    assert len(kernels) == 1 and all("pv_formant_kernel" in n for n in kernels), sorted(kernels)
    for n, v in kernels.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs"] <= 128 and v["LDS Size"] == 0, (n, v)


def test_the_new_files_stand_beside_the_existing_overlap_add_kernels():
    """The kernel file restates pv_tsm_kernel's arithmetic in its own file: it and its contract include none of the other overlap-add files and name none of
    their kernels or launchers, and use no inline assembly."""
    src = open(os.path.join(CSRC, "psola", "pv_formant_kernels.hip")).read()
    includes = re.findall(r'#include "([^"]+)"', src)
    assert "pv_formant.h" in includes and not any(i.endswith(".hip") for i in includes)
    assert not {"pv_psola.h", "pv_epoch.h", "pv_harmony.h", "pv_takes.h", "pv_mirror.h"} & set(includes)
    contract = re.findall(r'#include "([^"]+)"', open(os.path.join(CSRC, "psola", "pv_formant.h")).read())
    assert contract == ["pv_tsm.h"]
    code = re.sub(r"//.*", "", src)
    for name in ("pv_psola_kernel", "pv_epoch_kernel", "pv_tsm_kernel", "pv_harmony_kernel", "pv_takes_kernel", "pv_mirror_kernel", "pv_launch_tsm", "pv_launch_psola",
                 "pv_launch_harmony", "pv_launch_takes", "pv_launch_mirror", "asm"):
        assert name not in code, name
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "pv_formant_kernels.hip" in make.split("stretch-resource-usage:")[1]
    assert all(f"psola/pv_formant_{part}" in make.split("OBJS =")[0] for part in ("kernels.hip", "capi.hip", "plan.hip")) and "psola/pv_formant.h" in make


# ---- the example ------------------------------------------------------------------------------------------------------------------------------

def build_example(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_formant")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_formant.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_formant_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_example(tmp_path)
    if not _has_gpu():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device error" in r.stderr                    # no CPU fallback behind the C ABI
