"""CPU checks of the pitch-synchronous overlap-add surface: the header declares, the library exports and the ctypes binding gives argument types to
every pv_psola_* name, the ABI stays 6, pv_psola_plan and pv_psola_ratios equal the Python model (tests/psola_model.py) bit for bit, both size in two
calls and refuse every bad argument, the window table is the model's, bad configs are refused before any device is touched, the kernel file compiles
for gfx950 without spills, scratch or AGPRs, and examples/pv_psola.c builds as pedantic C99 (tests/test_gpu_psola.py runs it)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import f0_model as FM
import psola_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SURFACE = {"pv_psola_create": 2, "pv_psola_destroy": 1, "pv_psola_last_error": 1, "pv_psola_set_stream": 2, "pv_psola_synchronize": 1, "pv_psola_process": 11,
           "pv_psola_process_device": 11, "pv_psola_window": 2, "pv_psola_ratios": 5, "pv_psola_plan": 6}
DEVICE_POINTERS = {"pv_psola_process_device": (1, 7)}                       # void * in the binding
IP, DP, FP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float)


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
    return m.group(1).strip(), [re.sub(r"\s+", " ", re.sub(r"\b\w+$", "", p.strip())).strip() for p in m.group(2).split(",")]


def test_header_declares_library_exports_and_binding_types_the_surface():
    import phaze_amd
    from phaze_amd import capi
    text = open(HEADER).read()
    declared = set(re.findall(r"PV_API\s+[\w ]+?\*?\s*\b(pv_psola_\w+)\s*\(", text))
    assert declared == set(SURFACE)
    assert set(SURFACE) <= set(capi.EXPORTS)
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    assert set(SURFACE) <= set(re.findall(r" T (pv_\w+)", out))
    vp = C.c_void_p
    types = {"pv_psola *": vp, "const pv_psola *": vp, "pv_psola **": C.POINTER(vp), "const pv_psola_config *": C.POINTER(capi._PsolaConfig),
             "const pv_psola_params *": C.POINTER(capi._PsolaParams), "const pv_tune_params *": C.POINTER(capi._TuneParams), "void *": vp, "const float *": FP,
             "float *": FP, "int32_t": C.c_int32, "int64_t": C.c_int64, "const int32_t *": IP, "int32_t *": IP, "double *": DP, "const double *": DP}
    for name, nargs in SURFACE.items():
        ret, decl = _declaration(name)
        got = getattr(L, name).argtypes
        assert len(got) == len(decl) == nargs, (name, decl)
        for i, (d, g) in enumerate(zip(decl, got)):
            want = vp if i in DEVICE_POINTERS.get(name, ()) else types[d]
            assert g == want, (name, i, d, g)
        assert getattr(L, name).restype == {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p}[ret], (name, ret)
    assert L.pv_abi_version() == capi.ABI_VERSION == 6 == int(re.search(r"#define PV_ABI_VERSION (\d+)", text).group(1))
    note = text[text.index("#define PV_ABI_VERSION") - 2200:text.index("#define PV_ABI_VERSION")]
    assert "pv_psola_" in note                                              # recorded on the line for 6
    assert "PV_PSOLA_CONFIG_INIT" in text and "PV_PSOLA_PARAMS_INIT" in text
    assert C.sizeof(capi._PsolaConfig) == 24 and C.sizeof(capi._PsolaParams) == 40
    for struct, cls in (("pv_psola_config", capi._PsolaConfig), ("pv_psola_params", capi._PsolaParams)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, re.S).group(1)
        fields = re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+);", body, re.M)
        assert [(n, {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}[t]) for t, n in fields] == list(cls._fields_), struct
    for name in ("Psola", "tune_ratios", "psola_plan", "psola_window"):
        assert getattr(phaze_amd, name) is getattr(capi, name) and name in phaze_amd.__all__
    assert hasattr(capi.Psola, "process_tuned") and hasattr(capi.Psola, "process_device")


def test_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    x = (C.c_float * 8)()
    g = (C.c_int32 * 4)(4, 0, 0, 2)
    bad = capi.PV_ERR_ARGUMENT
    assert L.pv_psola_destroy(None) == bad and L.pv_psola_synchronize(None) == bad and L.pv_psola_set_stream(None, None) == bad
    assert L.pv_psola_process(None, x, 8, 8, 1, g, 1, x, 0, 8, 8) == bad
    assert L.pv_psola_process_device(None, None, 8, 8, 1, g, 1, None, 0, 8, 8) == bad
    assert L.pv_psola_create(None, None) == bad
    assert L.pv_psola_window(None, 4) == -bad and L.pv_psola_window(x, -1) == -bad


def test_config_errors_appear_without_a_device():
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    h = C.c_void_p()

    def create(cfg):
        rc = L.pv_psola_create(C.byref(cfg), C.byref(h))
        return rc, L.pv_psola_last_error(None).decode()

    for mp, word in [(1, "max_period"), (0, "max_period"), (4097, "max_period"), (-3, "max_period")]:
        rc, msg = create(capi.make_psola_config(mp))
        assert rc == capi.PV_ERR_ARGUMENT and word in msg, (mp, msg)
    cfg = capi.make_psola_config(512)
    cfg.struct_size -= 4
    rc, msg = create(cfg)
    assert rc == capi.PV_ERR_ARGUMENT and "struct_size" in msg
    rc, msg = create(capi.make_psola_config(512, flags=1))
    assert rc == capi.PV_ERR_ARGUMENT and "flags" in msg
    rc, msg = create(capi.make_psola_config(512, max_channels=-1))
    assert rc == capi.PV_ERR_ARGUMENT and "max_channels" in msg
    assert create(capi.make_psola_config(512, max_channels=65536))[0] == capi.PV_ERR_ARGUMENT
    rc, msg = create(capi.make_psola_config(512, max_outputs=-1))
    assert rc == capi.PV_ERR_ARGUMENT and "max_outputs" in msg
    with pytest.raises(phaze_amd.PvError):
        phaze_amd.Psola(1)
    if not _has_gpu():
        for mp in (2, 512, 4096):                                           # the corners of the legal range get as far as the device
            rc, msg = create(capi.make_psola_config(mp))
            assert rc == capi.PV_ERR_DEVICE and "HIP device" in msg        # fails loudly: no CPU fallback
        with pytest.raises(phaze_amd.PvError):
            phaze_amd.Psola(512)


def test_c_window_equals_the_models_table():
    import phaze_amd
    H = phaze_amd.psola_window()
    want = PM.window()
    assert H.dtype == np.float32 and H.shape == want.shape == (1026,)
    d = np.abs(H.astype(np.float64) - want.astype(np.float64))
    assert np.all(d <= 2.0 ** -23 * np.abs(want.astype(np.float64))), int(np.sum(H != want))      # cos of libm and of numpy: one ulp
    assert H[0] == 1.0 and H[512] == 0.5 and np.all(H[1024:] == 0.0) and np.all(np.diff(H[:1025]) < 0) and H[1023] > 0
    L = phaze_amd.load_library()
    buf = np.full(H.size + 4, -3.0, np.float32)
    assert L.pv_psola_window(None, 0) == H.size
    assert L.pv_psola_window(buf.ctypes.data_as(FP), H.size - 5) == H.size
    assert np.all(buf[H.size - 5:] == -3.0) and np.array_equal(buf[:H.size - 5], H[:H.size - 5])
    assert L.pv_psola_window(buf.ctypes.data_as(FP), H.size + 4) == H.size and np.all(buf[H.size:] == -3.0)


# ---- pure host code: the ratios and the planner ----------------------------------------------------------------------------------------------

RATIO_VARIANTS = [dict(), dict(retune=0.25), dict(scale_mask=FM.C_MAJOR), dict(strength=0.0), dict(strength=0.5, retune=0.6, a4=442.0), dict(scale_mask=1),
                  dict(sample_rate=44100.0), dict(sample_rate=12000.0), dict(sample_rate=192000.0, scale_mask=1)]


def _mixed(freq):
    recs = np.array(FM.plan_records(freq))
    recs[5:9, 0] *= -1                                                      # a stretch of unvoiced frames: the target returns to 0 there
    recs[15] = 0
    return recs


@pytest.mark.parametrize("freq", FM.PLAN_TONES + (470.0,))
def test_ratios_equal_the_model_exactly(freq):
    import phaze_amd
    for recs in (FM.plan_records(freq), _mixed(freq)):
        for kw in RATIO_VARIANTS:
            args = dict(sample_rate=FM.SAMPLE_RATE)
            args.update(kw)
            want = PM.tune_ratios(recs, **args)
            got = phaze_amd.tune_ratios(recs, **args)
            assert got.dtype == np.float64 and np.array_equal(got, want), (freq, kw)          # the same libm, the same operations: the same bits
            assert np.all((got >= 0.5) & (got <= 2.0))
    assert phaze_amd.tune_ratios(np.zeros((0, 4), np.int32), FM.SAMPLE_RATE).shape == (0,)


def _tracks():
    """(records, ratios or None, planner arguments): closed-form tones' records, random voiced / unvoiced tracks, and the edges of the argument range."""
    out = []
    for freq in FM.PLAN_TONES:
        recs = FM.plan_records(freq)
        base = dict(f0_hop=256, f0_center=1024, input_len=FM.PLAN_LEN, unvoiced_period=256.0, min_period=32, max_period=1024)
        out.append((recs, PM.tune_ratios(recs, FM.SAMPLE_RATE), base))
        out.append((_mixed(freq), PM.tune_ratios(_mixed(freq), FM.SAMPLE_RATE, retune=0.3), base))
        out.append((recs, None, dict(base, f0_center=0, input_len=5000)))
        out.append((recs, np.full(recs.shape[0], 0.5), dict(base, max_period=4096, unvoiced_period=4096.0)))
        out.append((recs, np.full(recs.shape[0], 2.0), dict(base, min_period=2, unvoiced_period=2.0, max_period=64)))
    rng = np.random.default_rng(11)
    for k in range(6):
        periods, ratios = [], []
        for s in range(8):
            v = rng.integers(0, 3)
            periods += [float(rng.uniform(10.0, 700.0)) if v else (0.0, -77.0)[s % 2]] * int(rng.integers(3, 40))
        recs = PM.records_of(periods)
        ratios = rng.uniform(0.5, 2.0, recs.shape[0])
        mp = (512, 4096, 33, 2)[k % 4]
        lo = min(20, mp)
        out.append((recs, ratios, dict(f0_hop=64, f0_center=(32, 0, 500)[k % 3], input_len=recs.shape[0] * 64 - k, unvoiced_period=float(max(lo, min(100, mp))),
                                       min_period=lo, max_period=mp)))
    out.append((np.zeros((0, 4), np.int32), None, dict(f0_hop=64, f0_center=32, input_len=3000, unvoiced_period=99.5, min_period=20, max_period=512)))
    out.append((PM.records_of([100.0] * 4), None, dict(f0_hop=64, f0_center=32, input_len=0, unvoiced_period=99.5, min_period=20, max_period=512)))
    out.append((PM.records_of([100.0] * 4), None, dict(f0_hop=64, f0_center=32, input_len=1, unvoiced_period=99.5, min_period=20, max_period=512)))
    return out


def test_plan_equals_the_model_exactly():
    import phaze_amd
    total = 0
    for recs, ratios, kw in _tracks():
        want = PM.psola_plan(recs, ratios=ratios, **kw)
        got = phaze_amd.psola_plan(recs, ratios=ratios, **kw)
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), kw
        assert PM.check_grains(got, kw["max_period"]) is None
        total += got.shape[0]
    assert total > 2000


def test_plan_and_ratios_size_in_two_calls_and_write_no_more_than_the_capacity():
    from phaze_amd import capi
    L = _lib()
    recs = np.ascontiguousarray(FM.plan_records(452.0))
    ratios = PM.tune_ratios(recs, FM.SAMPLE_RATE)
    want = PM.psola_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, ratios=ratios)
    p = capi.make_psola_params(256, 1024, FM.PLAN_LEN, 256.0, 32, 1024)
    rp, qp = recs.ctypes.data_as(IP), ratios.ctypes.data_as(DP)
    n = L.pv_psola_plan(C.byref(p), rp, recs.shape[0], qp, None, 0)
    assert n == want.shape[0] > 50
    g = np.full((n + 4, 4), -7, np.int32)
    assert L.pv_psola_plan(C.byref(p), rp, recs.shape[0], qp, g.ctypes.data_as(IP), n - 5) == n
    assert np.array_equal(g[:n - 5], want[:n - 5]) and np.all(g[n - 5:] == -7)
    assert L.pv_psola_plan(C.byref(p), rp, recs.shape[0], qp, g.ctypes.data_as(IP), n + 4) == n
    assert np.array_equal(g[:n], want) and np.all(g[n:] == -7)
    t = capi.make_tune_params(0, 0, FM.SAMPLE_RATE, 0, 0, 0, 0)
    out = np.full(recs.shape[0] + 4, -7.0)
    assert L.pv_psola_ratios(C.byref(t), rp, recs.shape[0], None, 0) == recs.shape[0]
    assert L.pv_psola_ratios(C.byref(t), rp, recs.shape[0], out.ctypes.data_as(DP), 5) == recs.shape[0]
    assert np.array_equal(out[:5], ratios[:5]) and np.all(out[5:] == -7.0)
    assert L.pv_psola_ratios(C.byref(t), rp, recs.shape[0], out.ctypes.data_as(DP), out.size) == recs.shape[0]
    assert np.array_equal(out[:recs.shape[0]], ratios) and np.all(out[recs.shape[0]:] == -7.0)


def test_plan_and_ratios_reject_every_bad_argument():
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    recs = np.ascontiguousarray(FM.plan_records(452.0))
    nrec = recs.shape[0]
    rp = recs.ctypes.data_as(IP)
    g = np.zeros((512, 4), np.int32)
    gp = g.ctypes.data_as(IP)
    ones = np.ones(nrec)
    bad = -capi.PV_ERR_ARGUMENT

    def plan(records=rp, n=nrec, ratios=None, out=gp, capacity=512, struct_delta=0, reserved=0, **kw):
        args = dict(f0_hop=256, f0_center=1024, input_len=FM.PLAN_LEN, unvoiced_period=256.0, min_period=32, max_period=1024)
        args.update(kw)
        p = capi.make_psola_params(**args)
        p.struct_size += struct_delta
        p.reserved = reserved
        return L.pv_psola_plan(C.byref(p), records, n, None if ratios is None else ratios.ctypes.data_as(DP), out, capacity)

    assert plan() == PM.psola_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024).shape[0]
    assert L.pv_psola_plan(None, rp, nrec, None, gp, 512) == bad
    two = ones.copy()
    two[7] = 2.0000001
    nan = ones.copy()
    nan[0] = np.nan
    for kw in (dict(struct_delta=8), dict(struct_delta=-8), dict(reserved=1), dict(records=None), dict(n=-1), dict(out=None), dict(capacity=-1), dict(f0_hop=0),
               dict(min_period=1), dict(min_period=0), dict(max_period=4097), dict(min_period=600, max_period=500, unvoiced_period=550.0), dict(unvoiced_period=31.9),
               dict(unvoiced_period=1024.5), dict(unvoiced_period=float("nan")), dict(input_len=-1), dict(input_len=1 << 30), dict(ratios=two), dict(ratios=nan),
               dict(ratios=ones * 0.49), dict(ratios=-ones)):
        assert plan(**kw) == bad, kw
    assert plan(records=None, n=0) == PM.psola_plan(np.zeros((0, 4), np.int32), 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024).shape[0]
    assert plan(out=None, capacity=0) == plan()
    assert plan(ratios=ones) == plan()
    with pytest.raises(ValueError):
        phaze_amd.psola_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 1, 1024)
    with pytest.raises(ValueError):
        phaze_amd.psola_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, ratios=np.ones(nrec - 1))

    out = np.zeros(nrec)
    op = out.ctypes.data_as(DP)

    def ratios(records=rp, n=nrec, dst=op, capacity=nrec, struct_delta=0, reserved=0, **kw):
        args = dict(f0_hop=0, f0_center=0, sample_rate=FM.SAMPLE_RATE, synthesis_hop=0, min_hop=0, max_hop=0, input_len=0)
        args.update(kw)
        t = capi.make_tune_params(**args)
        t.struct_size += struct_delta
        t.reserved = reserved
        return L.pv_psola_ratios(C.byref(t), records, n, dst, capacity)

    assert ratios() == nrec
    assert L.pv_psola_ratios(None, rp, nrec, op, nrec) == bad
    for kw in (dict(struct_delta=8), dict(struct_delta=-8), dict(reserved=1), dict(records=None), dict(n=-1), dict(dst=None), dict(capacity=-1), dict(scale_mask=0),
               dict(scale_mask=0x1000), dict(scale_mask=-1), dict(strength=-0.1), dict(strength=1.1), dict(strength=float("nan")), dict(retune=0.0), dict(retune=1.5),
               dict(retune=float("nan")), dict(sample_rate=0.0), dict(sample_rate=-48000.0), dict(sample_rate=float("inf")), dict(a4=-1.0), dict(a4=float("nan"))):
        assert ratios(**kw) == bad, kw
    assert ratios(records=None, n=0) == 0 and ratios(dst=None, capacity=0) == nrec
    assert ratios(f0_hop=-5, synthesis_hop=-1, min_hop=9, max_hop=3, input_len=-4, shift=12) == nrec      # the hop fields are ignored
    with pytest.raises(ValueError):
        phaze_amd.tune_ratios(recs, FM.SAMPLE_RATE, scale_mask=0)


# ---- kernel resources -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_psola_kernel_uses_no_spill_no_scratch_no_agprs():
    """One kernel, pv_psola_kernel: DESIGN.md "Pitch-synchronous correction" quotes its figures (33 VGPRs, no static LDS beside the dynamic arrays)."""
    src = os.path.join(ROOT, "phaze_amd", "csrc")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                          "-o", os.devnull, "psola/pv_psola_kernels.hip"], cwd=src, capture_output=True, text=True, timeout=900)
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
    assert len(kernels) == 1 and all("pv_psola_kernel" in n for n in kernels), sorted(kernels)
    for n, v in kernels.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs"] <= 64, (n, v)


# ---- the example ------------------------------------------------------------------------------------------------------------------------------

def build_example(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_psola")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_psola.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_psola_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_example(tmp_path)
    if not _has_gpu():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device error" in r.stderr                    # no CPU fallback behind the C ABI
