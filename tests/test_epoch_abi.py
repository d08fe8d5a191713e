"""CPU checks of the epoch surface: the header declares, the library exports and the ctypes binding gives argument types to every pv_epoch_* name, the
ABI stays 6, pv_epoch_plan and pv_epoch_periods equal the Python model (tests/epoch_model.py) bit for bit, both size in two calls and refuse every bad
argument, bad configs are refused before any device is touched, the kernel file compiles for gfx950 without spills, scratch or AGPRs, and
examples/pv_epoch.c builds as pedantic C99 (tests/test_gpu_epoch.py runs it)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import epoch_model as EM
import f0_model as FM
import psola_model as PM
import resource_usage as RU
import test_epoch_model as TEM
import test_psola_abi as TPA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
SURFACE = {"pv_epoch_create": 2, "pv_epoch_destroy": 1, "pv_epoch_last_error": 1, "pv_epoch_set_stream": 2, "pv_epoch_synchronize": 1, "pv_epoch_track": 8,
           "pv_epoch_track_device": 8, "pv_epoch_periods": 4, "pv_epoch_plan": 8}
DEVICE_POINTERS = {"pv_epoch_track_device": (1, 5, 6)}                      # void * in the binding
IP, DP, FP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float)

_lib = TPA._lib
_has_gpu = TPA._has_gpu
_declaration = TPA._declaration


def test_header_declares_library_exports_and_binding_types_the_surface():
    import phaze_amd
    from phaze_amd import capi
    text = open(HEADER).read()
    declared = set(re.findall(r"PV_API\s+[\w ]+?\*?\s*\b(pv_epoch_\w+)\s*\(", text))
    assert declared == set(SURFACE)
    assert set(SURFACE) <= set(capi.EXPORTS)
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pv_\w+)", out))
    assert set(SURFACE) <= exported and {n for n in exported if n.startswith("pv_epoch_")} == set(SURFACE)
    vp = C.c_void_p
    types = {"pv_epoch *": vp, "const pv_epoch *": vp, "pv_epoch **": C.POINTER(vp), "const pv_epoch_config *": C.POINTER(capi._EpochConfig),
             "const pv_epoch_params *": C.POINTER(capi._EpochParams), "const pv_psola_params *": C.POINTER(capi._PsolaParams), "void *": vp, "const float *": FP,
             "int32_t": C.c_int32, "int64_t": C.c_int64, "const int32_t *": IP, "int32_t *": IP, "const double *": DP}
    for name, nargs in SURFACE.items():
        ret, decl = _declaration(name)
        got = getattr(L, name).argtypes
        assert len(got) == len(decl) == nargs, (name, decl)
        for i, (d, g) in enumerate(zip(decl, got)):
            want = vp if i in DEVICE_POINTERS.get(name, ()) else types[d]
            assert g == want, (name, i, d, g)
        assert getattr(L, name).restype == {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p}[ret], (name, ret)
    assert L.pv_abi_version() == capi.ABI_VERSION == 6 == int(re.search(r"#define PV_ABI_VERSION (\d+)", text).group(1))
    note = text[text.index("#define PV_ABI_VERSION") - 2000:text.index("#define PV_ABI_VERSION")]
    assert "pv_epoch_" in note                                              # recorded on the line for 6
    assert "PV_EPOCH_CONFIG_INIT" in text and "PV_EPOCH_PARAMS_INIT" in text
    assert C.sizeof(capi._EpochConfig) == 32 and C.sizeof(capi._EpochParams) == 16
    for struct, cls in (("pv_epoch_config", capi._EpochConfig), ("pv_epoch_params", capi._EpochParams)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, re.S).group(1)
        fields = re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+);", body, re.M)
        assert [(n, {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}[t]) for t, n in fields] == list(cls._fields_), struct
    assert re.search(r"#define PV_EPOCH_PARAMS_INIT \{ \(int32_t\)sizeof\(pv_epoch_params\), 0, 0\.125 \}", text)
    e = capi.make_epoch_params()
    assert (e.struct_size, e.min_strength, e.lock) == (16, 0, EM.DEFAULT_LOCK)
    for name in ("EpochTracker", "epoch_periods", "epoch_plan"):
        assert getattr(phaze_amd, name) is getattr(capi, name) and name in phaze_amd.__all__
    assert hasattr(capi.EpochTracker, "track") and hasattr(capi.EpochTracker, "track_device")
    import inspect
    assert inspect.signature(capi.Psola.process_tuned).parameters["epochs"].default is False


def test_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    x = (C.c_float * 64)()
    p = (C.c_int32 * 1)(2048)
    r = (C.c_int32 * 4)(7, 7, 7, 7)
    bad = capi.PV_ERR_ARGUMENT
    assert L.pv_epoch_destroy(None) == bad and L.pv_epoch_synchronize(None) == bad and L.pv_epoch_set_stream(None, None) == bad
    assert L.pv_epoch_track(None, x, 1, 1, 64, p, r, 1) == bad
    assert L.pv_epoch_track_device(None, None, 1, 1, 64, None, None, 1) == bad
    assert L.pv_epoch_create(None, None) == bad
    assert list(r) == [7, 7, 7, 7]


def test_config_errors_appear_without_a_device():
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    h = C.c_void_p()

    def create(cfg):
        rc = L.pv_epoch_create(C.byref(cfg), C.byref(h))
        return rc, L.pv_epoch_last_error(None).decode()

    for args, word in [((2048, 256, 7), "max_period"), ((8192, 256, 2049), "max_period"), ((2048, 256, 0), "max_period"), ((2048, 256, -8), "max_period"),
                       ((2047, 256, 1024), "window"), ((8193, 256, 1024), "window"), ((15, 4, 8), "window"), ((2048, 0, 1024), "hop"), ((2048, 4097, 1024), "hop"),
                       ((2048, -1, 1024), "hop")]:
        rc, msg = create(capi.make_epoch_config(*args))
        assert rc == capi.PV_ERR_ARGUMENT and word in msg, (args, msg)
    cfg = capi.make_epoch_config(2048, 256, 1024)
    cfg.struct_size -= 4
    rc, msg = create(cfg)
    assert rc == capi.PV_ERR_ARGUMENT and "struct_size" in msg
    rc, msg = create(capi.make_epoch_config(2048, 256, 1024, flags=1))
    assert rc == capi.PV_ERR_ARGUMENT and "flags" in msg
    rc, msg = create(capi.make_epoch_config(2048, 256, 1024, max_channels=-1))
    assert rc == capi.PV_ERR_ARGUMENT and "max_channels" in msg
    assert create(capi.make_epoch_config(2048, 256, 1024, max_channels=65536))[0] == capi.PV_ERR_ARGUMENT
    rc, msg = create(capi.make_epoch_config(2048, 256, 1024, max_frames=-1))
    assert rc == capi.PV_ERR_ARGUMENT and "max_frames" in msg
    with pytest.raises(phaze_amd.PvError):
        phaze_amd.EpochTracker(2048, 256, 2049)
    if not _has_gpu():
        for args in ((16, 1, 8), (2048, 256, 1024), (8192, 4096, 2048)):    # the corners of the legal range get as far as the device
            rc, msg = create(capi.make_epoch_config(*args))
            assert rc == capi.PV_ERR_DEVICE and "HIP device" in msg        # fails loudly: no CPU fallback
        with pytest.raises(phaze_amd.PvError):
            phaze_amd.EpochTracker(2048, 256, 1024)


# ---- pure host code: the periods and the planner ----------------------------------------------------------------------------------------------

def _cases():
    """(records, ratios, planner arguments, epoch records): the tracks of tests/test_psola_abi.py and the random tracks of tests/test_psola_model.py, each
    with random epoch records."""
    rng = np.random.default_rng(23)
    out = []
    for recs, ratios, kw in TPA._tracks():
        out.append((recs, ratios, kw, TEM.random_epochs(rng, np.asarray(recs).reshape(-1, 4).shape[0], 2 * kw["max_period"])))
    for seed in range(6):
        recs, ratios, kw = TEM.track_arguments(seed)
        out.append((recs, ratios, kw, TEM.random_epochs(rng, recs.shape[0])))
    return out


def test_plan_equals_the_model_exactly():
    import phaze_amd
    total = moved = 0
    for recs, ratios, kw, ep in _cases():
        base = phaze_amd.psola_plan(recs, ratios=ratios, **kw)
        assert np.array_equal(phaze_amd.epoch_plan(recs, ratios=ratios, **kw), base), kw                       # epochs NULL: pv_psola_plan's bits
        for extra in (dict(), dict(lock=1.0), dict(lock=0.5, min_strength=6000), dict(min_strength=EM.S_ONE)):
            want = EM.epoch_plan(recs, ratios=ratios, epochs=ep, **kw, **extra)
            got = phaze_amd.epoch_plan(recs, ratios=ratios, epochs=ep, **kw, **extra)
            assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (kw, extra)
            assert PM.check_grains(got, kw["max_period"]) is None
            total += got.shape[0]
            moved += got.shape != base.shape or int(np.sum(got != base))
    assert total > 8000 and moved > 1000


def test_periods_equal_the_model_exactly():
    import phaze_amd
    for freq in FM.PLAN_TONES:
        recs = np.array(FM.plan_records(freq))
        recs[3:6, 0] *= -1
        recs[9] = 0
        got = phaze_amd.epoch_periods(recs)
        assert got.dtype == np.int32 and np.array_equal(got, EM.periods(recs)) and np.all(got[3:6] == 0) and got[9] == 0 and got[0] > 0
    assert phaze_amd.epoch_periods(np.zeros((0, 4), np.int32)).shape == (0,)


def test_plan_and_periods_size_in_two_calls_and_write_no_more_than_the_capacity():
    from phaze_amd import capi
    L = _lib()
    recs = np.ascontiguousarray(FM.plan_records(452.0))
    nrec = recs.shape[0]
    ratios = PM.tune_ratios(recs, FM.SAMPLE_RATE)
    ep = np.ascontiguousarray(TEM.random_epochs(np.random.default_rng(5), nrec))
    want = EM.epoch_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, ratios=ratios, epochs=ep)
    p = capi.make_psola_params(256, 1024, FM.PLAN_LEN, 256.0, 32, 1024)
    e = capi.make_epoch_params()
    rp, qp, ep_ = recs.ctypes.data_as(IP), ratios.ctypes.data_as(DP), ep.ctypes.data_as(IP)
    n = L.pv_epoch_plan(C.byref(p), C.byref(e), rp, nrec, qp, ep_, None, 0)
    assert n == want.shape[0] > 50
    g = np.full((n + 4, 4), -7, np.int32)
    assert L.pv_epoch_plan(C.byref(p), C.byref(e), rp, nrec, qp, ep_, g.ctypes.data_as(IP), n - 5) == n
    assert np.array_equal(g[:n - 5], want[:n - 5]) and np.all(g[n - 5:] == -7)
    assert L.pv_epoch_plan(C.byref(p), C.byref(e), rp, nrec, qp, ep_, g.ctypes.data_as(IP), n + 4) == n
    assert np.array_equal(g[:n], want) and np.all(g[n:] == -7)
    out = np.full(nrec + 4, -7, np.int32)
    assert L.pv_epoch_periods(rp, nrec, None, 0) == nrec
    assert L.pv_epoch_periods(rp, nrec, out.ctypes.data_as(IP), 5) == nrec
    assert np.array_equal(out[:5], EM.periods(recs)[:5]) and np.all(out[5:] == -7)
    assert L.pv_epoch_periods(rp, nrec, out.ctypes.data_as(IP), out.size) == nrec
    assert np.array_equal(out[:nrec], EM.periods(recs)) and np.all(out[nrec:] == -7)


def test_plan_and_periods_reject_every_bad_argument():
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    recs = np.ascontiguousarray(FM.plan_records(452.0))
    nrec = recs.shape[0]
    rp = recs.ctypes.data_as(IP)
    g = np.zeros((512, 4), np.int32)
    gp = g.ctypes.data_as(IP)
    ones = np.ones(nrec)
    ep = np.ascontiguousarray(TEM.random_epochs(np.random.default_rng(6), nrec))
    bad = -capi.PV_ERR_ARGUMENT

    def plan(records=rp, n=nrec, ratios=None, epochs=ep, out=gp, capacity=512, struct_delta=0, reserved=0, e_delta=0, min_strength=0, lock=0.125, no_e=False, **kw):
        args = dict(f0_hop=256, f0_center=1024, input_len=FM.PLAN_LEN, unvoiced_period=256.0, min_period=32, max_period=1024)
        args.update(kw)
        p = capi.make_psola_params(**args)
        p.struct_size += struct_delta
        p.reserved = reserved
        e = capi.make_epoch_params(min_strength, lock)
        e.struct_size += e_delta
        return L.pv_epoch_plan(C.byref(p), None if no_e else C.byref(e), records, n, None if ratios is None else ratios.ctypes.data_as(DP),
                               None if epochs is None else epochs.ctypes.data_as(IP), out, capacity)

    assert plan() == EM.epoch_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, epochs=ep).shape[0]
    assert L.pv_epoch_plan(None, C.byref(capi.make_epoch_params()), rp, nrec, None, None, gp, 512) == bad
    before = g.copy()
    two = ones.copy()
    two[7] = 2.0000001
    nan = ones.copy()
    nan[0] = np.nan
    for kw in (dict(struct_delta=8), dict(struct_delta=-8), dict(reserved=1), dict(records=None), dict(n=-1), dict(out=None), dict(capacity=-1), dict(f0_hop=0),
               dict(min_period=1), dict(min_period=0), dict(max_period=4097), dict(min_period=600, max_period=500, unvoiced_period=550.0), dict(unvoiced_period=31.9),
               dict(unvoiced_period=1024.5), dict(unvoiced_period=float("nan")), dict(input_len=-1), dict(input_len=1 << 30), dict(ratios=two), dict(ratios=nan),
               dict(ratios=ones * 0.49), dict(ratios=-ones), dict(no_e=True), dict(e_delta=8), dict(e_delta=-8), dict(min_strength=-1), dict(min_strength=16385),
               dict(lock=0.0), dict(lock=-0.5), dict(lock=1.0000001), dict(lock=float("nan")), dict(lock=float("inf"))):
        assert plan(**kw) == bad, kw
    assert np.array_equal(g, before)                                        # nothing written by a refused call
    assert plan(records=None, n=0, epochs=None) == PM.psola_plan(np.zeros((0, 4), np.int32), 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024).shape[0]
    assert plan(out=None, capacity=0) == plan()
    assert plan(epochs=None) == PM.psola_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024).shape[0]
    assert plan(lock=1.0, min_strength=16384) > 0
    with pytest.raises(ValueError):
        phaze_amd.epoch_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, lock=0.0)
    with pytest.raises(ValueError):
        phaze_amd.epoch_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, epochs=ep[:-1])
    with pytest.raises(ValueError):
        phaze_amd.epoch_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, ratios=np.ones(nrec - 1))

    out = np.zeros(nrec, np.int32)
    op = out.ctypes.data_as(IP)
    assert L.pv_epoch_periods(rp, nrec, op, nrec) == nrec
    for args in ((None, nrec, op, nrec), (rp, -1, op, nrec), (rp, nrec, None, nrec), (rp, nrec, op, -1)):
        assert L.pv_epoch_periods(*args) == bad, args
    assert L.pv_epoch_periods(None, 0, None, 0) == 0


# ---- kernel resources -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_epoch_kernel_uses_no_spill_no_scratch_no_agprs():
    """One kernel, pv_epoch_kernel: DESIGN.md "Epoch marks" quotes its figures (35 VGPRs, no static LDS beside the dynamic array)."""
    kernels = RU.resources("psola/pv_epoch_kernels.hip")
    assert len(kernels) == 1 and all("pv_epoch_kernel" in n for n in kernels), sorted(kernels)
    for n, v in kernels.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs"] <= 64 and v["LDS Size"] == 0, (n, v)


# ---- the example ------------------------------------------------------------------------------------------------------------------------------

def build_example(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_epoch")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_epoch.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_epoch_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_example(tmp_path)
    if not _has_gpu():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device error" in r.stderr                    # no CPU fallback behind the C ABI
