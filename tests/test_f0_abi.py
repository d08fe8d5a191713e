"""CPU checks of the pitch-tracking and pitch-correction surface: the header declares, the library exports and the ctypes binding gives argument types
to every pv_f0_* / pv_tune_* name, the ABI stays 6, pv_f0_period and pv_tune_plan equal the Python model (tests/f0_model.py) exactly, the planner
sizes in two calls, every bad argument is refused, bad configs are refused before any device is touched, the kernel file compiles for gfx950 without
spills or scratch, and examples/pv_tune.c builds as pedantic C99 (tests/test_gpu_f0.py runs it)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import f0_model as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SURFACE = {"pv_f0_create": 2, "pv_f0_destroy": 1, "pv_f0_last_error": 1, "pv_f0_set_stream": 2, "pv_f0_synchronize": 1, "pv_f0_track": 8,
           "pv_f0_track_device": 8, "pv_f0_period": 1, "pv_tune_plan": 6}
DEVICE_POINTERS = {"pv_f0_track_device": (1, 6)}                            # void * in the binding


def _lib():
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    return phaze_amd.load_library()


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _declaration(name):
    m = re.search(r"PV_API\s+([\w ]+?\*?)\s*\b" + name + r"\s*\(([^)]*)\)", open(HEADER).read())
    assert m, name
    params = []
    for p in m.group(2).split(","):
        p = p.strip()
        if p.endswith("]"):                                                  # const int32_t rec[4]: a pointer
            p = re.sub(r"\s*\w+\[\d*\]$", " *", p)
        else:
            p = re.sub(r"\b\w+$", "", p)
        params.append(re.sub(r"\s+", " ", p).strip())
    return m.group(1).strip(), params


def test_header_declares_library_exports_and_binding_types_the_surface():
    import phaze_amd
    from phaze_amd import capi
    text = open(HEADER).read()
    declared = set(re.findall(r"PV_API\s+[\w ]+?\*?\s*\b(pv_(?:f0|tune)_\w+)\s*\(", text))
    assert declared == set(SURFACE)
    assert set(SURFACE) <= set(capi.EXPORTS)
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    assert set(SURFACE) <= set(re.findall(r" T (pv_\w+)", out))
    fp, vp, ip = C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_int32)
    types = {"pv_f0 *": vp, "const pv_f0 *": vp, "pv_f0 **": C.POINTER(vp), "const pv_f0_config *": C.POINTER(capi._F0Config),
             "const pv_tune_params *": C.POINTER(capi._TuneParams), "void *": vp, "const float *": fp, "int32_t": C.c_int32, "int64_t": C.c_int64,
             "const int32_t *": ip, "int32_t *": ip, "double *": C.POINTER(C.c_double)}
    for name, nargs in SURFACE.items():
        ret, decl = _declaration(name)
        got = getattr(L, name).argtypes
        assert len(got) == len(decl) == nargs, (name, decl)
        for i, (d, g) in enumerate(zip(decl, got)):
            want = vp if i in DEVICE_POINTERS.get(name, ()) else types[d]
            assert g == want, (name, i, d, g)
        assert getattr(L, name).restype == {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p, "double": C.c_double}[ret], (name, ret)
    assert L.pv_abi_version() == capi.ABI_VERSION == 6 == int(re.search(r"#define PV_ABI_VERSION (\d+)", text).group(1))
    note = text[text.index("#define PV_ABI_VERSION") - 2200:text.index("#define PV_ABI_VERSION")]
    assert "pv_f0_" in note and "pv_tune_plan" in note                       # recorded on the line for 6
    assert "PV_F0_CONFIG_INIT" in text and "PV_TUNE_PARAMS_INIT" in text
    assert C.sizeof(capi._F0Config) == 36 and C.sizeof(capi._TuneParams) == 80
    # the struct layouts, field by field, against the header
    for struct, cls in (("pv_f0_config", capi._F0Config), ("pv_tune_params", capi._TuneParams)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, re.S).group(1)
        fields = re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+);", body, re.M)
        assert [(n, {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}[t]) for t, n in fields] == list(cls._fields_), struct
    assert phaze_amd.F0Tracker is capi.F0Tracker and phaze_amd.tune_plan is capi.tune_plan and phaze_amd.f0_period is capi.f0_period
    assert hasattr(capi.PitchGlide, "process_tuned")


def test_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    x = (C.c_float * 8)()
    rec = (C.c_int32 * 4)()
    bad = capi.PV_ERR_ARGUMENT
    assert L.pv_f0_destroy(None) == bad and L.pv_f0_synchronize(None) == bad and L.pv_f0_set_stream(None, None) == bad
    assert L.pv_f0_track(None, x, 1, 1, 8, 2458, rec, 1) == bad
    assert L.pv_f0_track_device(None, None, 1, 1, 8, 2458, None, 1) == bad
    assert L.pv_f0_create(None, None) == bad
    assert L.pv_f0_period(None) == 0.0


def test_config_errors_appear_without_a_device():
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    h = C.c_void_p()

    def create(cfg):
        rc = L.pv_f0_create(C.byref(cfg), C.byref(h))
        return rc, L.pv_f0_last_error(None).decode()

    for W, hop, lo, hi, word in [(15, 16, 2, 16, "window"), (4097, 16, 2, 16, "window"), (1024, 0, 32, 1024, "hop"), (1024, 4097, 32, 1024, "hop"),
                                 (1024, 256, 1, 1024, "min_lag"), (1024, 256, 512, 512, "min_lag"), (1024, 256, 600, 512, "min_lag"),
                                 (1024, 256, 32, 4097, "4096"), (-1, 256, 32, 1024, "window")]:
        rc, msg = create(capi.make_f0_config(W, hop, lo, hi))
        assert rc == capi.PV_ERR_ARGUMENT and word in msg, (W, hop, lo, hi, msg)
    cfg = capi.make_f0_config(1024, 256, 32, 1024)
    cfg.struct_size -= 4
    rc, msg = create(cfg)
    assert rc == capi.PV_ERR_ARGUMENT and "struct_size" in msg
    rc, msg = create(capi.make_f0_config(1024, 256, 32, 1024, flags=1))
    assert rc == capi.PV_ERR_ARGUMENT and "flags" in msg
    assert create(capi.make_f0_config(1024, 256, 32, 1024, max_channels=-1))[0] == capi.PV_ERR_ARGUMENT
    assert create(capi.make_f0_config(1024, 256, 32, 1024, max_channels=65536))[0] == capi.PV_ERR_ARGUMENT
    assert create(capi.make_f0_config(1024, 256, 32, 1024, max_frames=-1))[0] == capi.PV_ERR_ARGUMENT
    with pytest.raises(phaze_amd.PvError):
        phaze_amd.F0Tracker(8, 4, 2, 8)
    if not _has_gpu():
        for W, hop, lo, hi in [(1024, 256, 32, 1024), (16, 1, 2, 3), (4096, 4096, 4095, 4096), (257, 64, 2, 301)]:    # the corners of the legal range get as far as the device
            assert create(capi.make_f0_config(W, hop, lo, hi))[0] == capi.PV_ERR_DEVICE         # fails loudly: no CPU fallback
        with pytest.raises(phaze_amd.PvError):
            phaze_amd.F0Tracker(1024, 256, 32, 1024)


# ---- pure host code: the period and the planner ---------------------------------------------------------------------------------------------

def test_period_equals_the_model():
    import phaze_amd
    recs = np.concatenate([FM.plan_records(f) for f in FM.PLAN_TONES]
                          + [np.array([[0, 0, 0, 0], [-40, 9000, 8000, 9000], [40, 500, 100, 500], [40, 100, 100, 100], [40, 50, 100, 70], [2, 16384, 0, 1],
                                       [4095, 2 ** 26, 0, 2 ** 26], [77, 3, 1, 2 ** 26]], np.int32)])
    got = phaze_amd.f0_period(recs)
    want = np.array([FM.period(r) for r in recs])
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert got[-8] == 0.0 and got[-7] == 0.0 and got[-6] == 40.0 and got[-5] == 40.0 and got[-4] == 40.0      # empty, unvoiced, symmetric, flat, a maximum
    assert phaze_amd.f0_period(recs.reshape(2, -1, 4)).shape == (2, recs.shape[0] // 2)


PLAN_VARIANTS = [dict(), dict(retune=0.25), dict(scale_mask=FM.C_MAJOR), dict(strength=0.0), dict(strength=0.5, retune=0.6, a4=442.0), dict(shift=700),
                 dict(shift=-5000), dict(input_len=5000), dict(input_len=127), dict(input_len=0), dict(scale_mask=1), dict(f0_center=0),
                 dict(synthesis_hop=320, min_hop=200, max_hop=440), dict(min_hop=250, max_hop=260), dict(sample_rate=44100.0)]


def _c_plan(records, curve=True, **kw):
    import phaze_amd
    g = FM.PLAN_GEOMETRY
    args = dict(f0_hop=g["hop"], f0_center=(g["W"] + g["max_lag"]) // 2, sample_rate=FM.SAMPLE_RATE, synthesis_hop=256, min_hop=128, max_hop=512, input_len=FM.PLAN_LEN)
    args.update(kw)
    return phaze_amd.tune_plan(records, curve=curve, **args)


@pytest.mark.parametrize("freq", FM.PLAN_TONES + (470.0,))
def test_plan_equals_the_model_exactly(freq):
    recs = FM.plan_records(freq)
    for kw in PLAN_VARIANTS:
        want_h, want_r = FM.plan(recs, **kw)
        got_h, got_r = _c_plan(recs, **kw)
        assert got_h.dtype == np.int32 and np.array_equal(got_h, want_h), (freq, kw)
        assert np.array_equal(got_r, want_r), (freq, kw, float(np.max(np.abs(got_r - want_r))))      # the same libm, the same operations: the same bits
    mixed = np.array(recs)
    mixed[5:9, 0] *= -1                                                     # a stretch of unvoiced frames: the target returns to 0 there
    mixed[15] = 0
    for kw in (dict(), dict(retune=0.3)):
        want_h, want_r = FM.plan(mixed, **kw)
        got_h, got_r = _c_plan(mixed, **kw)
        assert np.array_equal(got_h, want_h) and np.array_equal(got_r, want_r)
    assert np.array_equal(_c_plan(np.zeros((0, 4), np.int32))[0], FM.plan(np.zeros((0, 4), np.int32))[0])


def test_plan_sizes_in_two_calls_and_writes_no_more_than_the_capacity():
    from phaze_amd import capi
    L = _lib()
    recs = np.ascontiguousarray(FM.plan_records(452.0))
    want_h, want_r = FM.plan(recs)
    p = capi.make_tune_params(256, 1024, FM.SAMPLE_RATE, 256, 128, 512, FM.PLAN_LEN)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rp = recs.ctypes.data_as(ip)
    n = L.pv_tune_plan(C.byref(p), rp, recs.shape[0], None, None, 0)
    assert n == want_h.size
    hops, curve = np.full(n + 4, -7, np.int32), np.full(n + 4, -7.0)
    assert L.pv_tune_plan(C.byref(p), rp, recs.shape[0], hops.ctypes.data_as(ip), curve.ctypes.data_as(dp), n - 5) == n
    assert np.array_equal(hops[:n - 5], want_h[:n - 5]) and np.all(hops[n - 5:] == -7) and np.all(curve[n - 5:] == -7.0)
    assert L.pv_tune_plan(C.byref(p), rp, recs.shape[0], hops.ctypes.data_as(ip), None, n + 4) == n            # the curve is optional
    assert np.array_equal(hops[:n], want_h) and np.all(hops[n:] == -7)
    assert L.pv_tune_plan(C.byref(p), rp, recs.shape[0], hops.ctypes.data_as(ip), curve.ctypes.data_as(dp), n) == n
    assert np.array_equal(curve[:n], want_r)


def test_plan_rejects_every_bad_argument():
    from phaze_amd import capi
    L = _lib()
    recs = np.ascontiguousarray(FM.plan_records(452.0))
    ip = C.POINTER(C.c_int32)
    rp = recs.ctypes.data_as(ip)
    hops = np.zeros(64, np.int32)
    hp = hops.ctypes.data_as(ip)
    bad = -capi.PV_ERR_ARGUMENT

    def call(records=rp, nrec=recs.shape[0], out=hp, capacity=64, struct_delta=0, reserved=0, **kw):
        args = dict(f0_hop=256, f0_center=1024, sample_rate=FM.SAMPLE_RATE, synthesis_hop=256, min_hop=128, max_hop=512, input_len=FM.PLAN_LEN)
        args.update(kw)
        p = capi.make_tune_params(**args)
        p.struct_size += struct_delta
        p.reserved = reserved
        return L.pv_tune_plan(C.byref(p), records, nrec, out, None, capacity)

    assert call() == FM.plan(recs)[0].size
    assert L.pv_tune_plan(None, rp, recs.shape[0], hp, None, 64) == bad
    for kw in (dict(struct_delta=8), dict(struct_delta=-8), dict(reserved=1), dict(records=None), dict(nrec=-1), dict(out=None), dict(capacity=-1),
               dict(scale_mask=0), dict(scale_mask=0x1000), dict(scale_mask=-1), dict(strength=-0.1), dict(strength=1.1), dict(strength=float("nan")),
               dict(retune=0.0), dict(retune=1.5), dict(retune=float("nan")), dict(sample_rate=0.0), dict(sample_rate=-48000.0), dict(sample_rate=float("inf")),
               dict(a4=-1.0), dict(a4=float("nan")), dict(f0_hop=0), dict(synthesis_hop=0), dict(min_hop=0), dict(min_hop=300, max_hop=200), dict(input_len=-1)):
        assert call(**kw) == bad, kw
    assert call(records=None, nrec=0) == FM.PLAN_LEN // 256                   # no records at all: every frame at the synthesis hop
    assert call(out=None, capacity=0) == FM.plan(recs)[0].size
    assert call(a4=0.0) == call(a4=440.0)                                     # 0 selects the default
    import phaze_amd
    with pytest.raises(ValueError):
        phaze_amd.tune_plan(recs, 256, FM.SAMPLE_RATE, 256, 128, 512, FM.PLAN_LEN, scale_mask=0)


# ---- kernel resources -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_f0_kernel_uses_no_spill_no_scratch_no_agprs():
    """One kernel, pv_f0_kernel: DESIGN.md "Pitch tracking" quotes its figures (36 VGPRs, 48 bytes of static LDS beside the dynamic arrays)."""
    src = os.path.join(ROOT, "phaze_amd", "csrc")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                          "-o", os.devnull, "stretch/pv_f0_kernels.hip"], cwd=src, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
    assert len(kernels) == 1 and all("pv_f0_kernel" in n for n in kernels), sorted(kernels)
    for n, v in kernels.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs"] <= 64, (n, v)


# ---- the example ------------------------------------------------------------------------------------------------------------------------------

def build_example(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_tune")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_tune.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_tune_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_example(tmp_path)
    if not _has_gpu():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device error" in r.stderr                    # no CPU fallback behind the C ABI
