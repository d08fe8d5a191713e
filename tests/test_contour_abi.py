"""CPU checks of the pitch contour surface: the header declares, the library exports and the ctypes binding gives argument types to every pv_contour_* name,
the ABI stays 6, calls without a handle and bad configs are refused before any device is touched, pv_contour_path equals the Python model
(tests/contour_model.py) with == on records and states and refuses every bad argument with the output untouched, the kernel file compiles for gfx950 to one
kernel without spills, scratch or AGPRs, and examples/pv_contour.c builds as pedantic C99 (tests/test_gpu_contour.py runs it).  The path search also runs in a
stand-alone program (tests/sanitize/contour_host.cpp) built with AddressSanitizer and UBSan: host code only, nothing of it is loaded into this process."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import contour_model as CM
import resource_usage as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
CSRC = os.path.join(ROOT, "phaze_amd", "csrc")
SURFACE = {"pv_contour_create": 2, "pv_contour_destroy": 1, "pv_contour_last_error": 1, "pv_contour_set_stream": 2, "pv_contour_synchronize": 1,
           "pv_contour_track": 8, "pv_contour_track_device": 8, "pv_contour_path": 5}
DEVICE_POINTERS = {"pv_contour_track_device": (1, 6)}                       # void * in the binding
IP = C.POINTER(C.c_int32)
ML = CM.GEOMETRY["max_lag"]


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
    params = [re.sub(r"\s+", " ", re.sub(r"\b\w+$", "", p.strip())).strip() for p in m.group(2).split(",")]
    return m.group(1).strip(), params


def test_header_declares_library_exports_and_binding_types_the_surface():
    import phaze_amd
    from phaze_amd import capi
    text = open(HEADER).read()
    declared = set(re.findall(r"PV_API\s+[\w ]+?\*?\s*\b(pv_contour_\w+)\s*\(", text))
    assert declared == set(SURFACE)
    assert set(SURFACE) <= set(capi.EXPORTS) and {n for n in capi.EXPORTS if n.startswith("pv_contour_")} == set(SURFACE)
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pv_\w+)", out))
    assert set(SURFACE) <= exported and {n for n in exported if n.startswith("pv_contour_")} == set(SURFACE)
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    types = {"pv_contour *": vp, "const pv_contour *": vp, "pv_contour **": C.POINTER(vp), "const pv_contour_config *": C.POINTER(capi._ContourConfig),
             "const pv_contour_params *": C.POINTER(capi._ContourParams), "void *": vp, "const float *": fp, "int32_t": C.c_int32, "int64_t": C.c_int64,
             "const int32_t *": IP, "int32_t *": IP}
    for name, nargs in SURFACE.items():
        ret, decl = _declaration(name)
        got = getattr(L, name).argtypes
        assert len(got) == len(decl) == nargs, (name, decl)
        for i, (d, g) in enumerate(zip(decl, got)):
            want = vp if i in DEVICE_POINTERS.get(name, ()) else types[d]
            assert g == want, (name, i, d, g)
        assert getattr(L, name).restype == {"int": C.c_int, "const char *": C.c_char_p}[ret], (name, ret)
    assert L.pv_abi_version() == capi.ABI_VERSION == 6 == int(re.search(r"#define PV_ABI_VERSION (\d+)", text).group(1))
    note = text[text.index("#define PV_ABI_VERSION") - 2000:text.index("#define PV_ABI_VERSION")]
    assert "pv_contour_" in note                                             # recorded on the line for 6
    assert "PV_CONTOUR_CONFIG_INIT" in text and "PV_CONTOUR_PARAMS_INIT" in text
    assert C.sizeof(capi._ContourConfig) == 40 and C.sizeof(capi._ContourParams) == 32
    for struct, cls in (("pv_contour_config", capi._ContourConfig), ("pv_contour_params", capi._ContourParams)):      # field by field, against the header
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, re.S).group(1)
        fields = re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+);", body, re.M)
        assert [(n, {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}[t]) for t, n in fields] == list(cls._fields_), struct
    init = re.search(r"#define PV_CONTOUR_PARAMS_INIT \{([^}]*)\}", text).group(1).split(",")
    assert [v.strip() for v in init[1:]] == ["8", "0", "1024", "2458", "2458", "16384", "0"]
    p = capi.make_contour_params(8, 512)
    assert (p.struct_size, p.candidates, p.max_lag, p.bias, p.unvoiced_cost, p.voicing_cost, p.jump_cost, p.reserved) == (32, 8, 512, 1024, 2458, 2458, 16384, 0)
    assert phaze_amd.ContourTracker is capi.ContourTracker and phaze_amd.contour_path is capi.contour_path
    assert phaze_amd.make_contour_config is capi.make_contour_config
    for name in ("frames", "candidates", "track", "track_device"):
        assert callable(getattr(capi.ContourTracker, name))
    assert not re.search(r"PV_FLAG_\w*CONTOUR", text)


def test_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    x = (C.c_float * 8)()
    cand = (C.c_int32 * 32)()
    bad = capi.PV_ERR_ARGUMENT
    assert L.pv_contour_destroy(None) == bad and L.pv_contour_synchronize(None) == bad and L.pv_contour_set_stream(None, None) == bad
    assert L.pv_contour_track(None, x, 1, 1, 8, 1024, cand, 1) == bad
    assert L.pv_contour_track_device(None, None, 1, 1, 8, 1024, None, 1) == bad
    assert L.pv_contour_create(None, None) == bad
    assert not any(cand)


def test_config_errors_appear_without_a_device():
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    h = C.c_void_p()

    def create(cfg):
        rc = L.pv_contour_create(C.byref(cfg), C.byref(h))
        return rc, L.pv_contour_last_error(None).decode()

    for W, hop, lo, hi, word in [(15, 16, 2, 16, "window"), (4097, 16, 2, 16, "window"), (1024, 0, 32, 1024, "hop"), (1024, 4097, 32, 1024, "hop"),
                                 (1024, 256, 1, 1024, "min_lag"), (1024, 256, 512, 512, "min_lag"), (1024, 256, 600, 512, "min_lag"),
                                 (1024, 256, 32, 4097, "4096"), (-1, 256, 32, 1024, "window")]:
        rc, msg = create(capi.make_contour_config(W, hop, lo, hi))
        assert rc == capi.PV_ERR_ARGUMENT and word in msg, (W, hop, lo, hi, msg)
    cfg = capi.make_contour_config(1024, 256, 32, 1024)
    cfg.struct_size -= 4
    rc, msg = create(cfg)
    assert rc == capi.PV_ERR_ARGUMENT and "struct_size" in msg
    rc, msg = create(capi.make_contour_config(1024, 256, 32, 1024, flags=1))
    assert rc == capi.PV_ERR_ARGUMENT and "flags" in msg
    for k in (-1, 9):
        rc, msg = create(capi.make_contour_config(1024, 256, 32, 1024, candidates=k))
        assert rc == capi.PV_ERR_ARGUMENT and "candidates" in msg
    assert create(capi.make_contour_config(1024, 256, 32, 1024, max_channels=-1))[0] == capi.PV_ERR_ARGUMENT
    assert create(capi.make_contour_config(1024, 256, 32, 1024, max_channels=65536))[0] == capi.PV_ERR_ARGUMENT
    assert create(capi.make_contour_config(1024, 256, 32, 1024, max_frames=-1))[0] == capi.PV_ERR_ARGUMENT
    with pytest.raises(phaze_amd.PvError):
        phaze_amd.ContourTracker(8, 4, 2, 8)
    if not _has_gpu():
        for W, hop, lo, hi, k in [(1024, 256, 32, 1024, 8), (16, 1, 2, 3, 0), (4096, 4096, 4095, 4096, 1), (257, 64, 2, 301, 3)]:    # the corners of the legal range
            assert create(capi.make_contour_config(W, hop, lo, hi, candidates=k))[0] == capi.PV_ERR_DEVICE         # fails loudly: no CPU fallback
        with pytest.raises(phaze_amd.PvError):
            phaze_amd.ContourTracker(1024, 256, 32, 1024)


# ---- pure host code: the path ---------------------------------------------------------------------------------------------------------------------

COSTS = [CM.DEFAULTS, dict(bias=0, unvoiced_cost=100, voicing_cost=0, jump_cost=0), dict(bias=16384, unvoiced_cost=16384, voicing_cost=5000, jump_cost=1 << 20),
         dict(bias=1024, unvoiced_cost=1, voicing_cost=1 << 20, jump_cost=300)]


def _same(table, max_lag, **kw):
    import phaze_amd
    want_r, want_s = CM.path(table, max_lag, **kw)
    got_r, got_s = phaze_amd.contour_path(table, max_lag, states=True, **kw)
    assert got_r.dtype == got_s.dtype == np.int32 and got_r.shape == want_r.shape
    assert np.array_equal(got_r, want_r) and np.array_equal(got_s, want_s), (table.shape, kw, np.argwhere(got_s != want_s)[:4].tolist())
    assert np.array_equal(phaze_amd.contour_path(table, max_lag, **kw), want_r)                  # the states are optional


def test_path_equals_the_model_on_the_signals_tables():
    for name in CM.FADES + CM.NOISY + ["leap", "tnt"]:
        _same(CM.table(name), ML)
    for name in CM.NOISY:
        _same(CM.table(name, 2), ML)
    _same(CM.table("tnt"), ML, bias=1024, unvoiced_cost=600, voicing_cost=100, jump_cost=40000)
    _same(CM.table("leap"), ML, bias=0, unvoiced_cost=16384, voicing_cost=0, jump_cost=1 << 20)


def test_path_equals_the_model_on_random_tables():
    rng = np.random.default_rng(11)
    sizes = [0, 1, 1, 5000] + [int(v) for v in rng.integers(2, 60, 196)]
    seen = set()
    for trial, T in enumerate(sizes):
        K = trial % 8 + 1
        t = CM.random_table(rng, T, K, max_lag=512, lead=int(rng.integers(0, 4)) if T > 4 else 0)
        if trial % 10 == 9:
            t[:, :, 0] = np.where(t[:, :, 0] > 0, 65535, 0)                  # the largest lag a table may hold, in every slot: every jump a tie
        _same(t, 4096 if trial % 10 == 9 else 512, **COSTS[trial % len(COSTS)])
        seen.add(K)
    assert len(sizes) == 200 and seen == set(range(1, 9))


def test_path_rejects_every_bad_argument_and_leaves_the_output_untouched():
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    t = np.ascontiguousarray(CM.table(CM.FADES[3]))
    nrec = t.shape[0]
    rec, st = np.full((nrec, 4), -77, np.int32), np.full(nrec, -77, np.int32)

    def call(table=t, n=nrec, records=rec, states=st, struct_delta=0, reserved=0, null_params=False, **kw):
        args = dict(candidates=8, max_lag=ML)
        args.update(kw)
        p = capi.make_contour_params(**args)
        p.struct_size += struct_delta
        p.reserved = reserved
        return L.pv_contour_path(None if null_params else C.byref(p), None if table is None else table.ctypes.data_as(IP), n,
                                 None if records is None else records.ctypes.data_as(IP), None if states is None else states.ctypes.data_as(IP))

    def poisoned(i, k, f, v):
        b = np.array(t)
        b[i, k, f] = v
        return b

    for kw in (dict(null_params=True), dict(struct_delta=4), dict(struct_delta=-4), dict(reserved=1), dict(table=None), dict(records=None), dict(n=-1),
               dict(candidates=0), dict(candidates=9), dict(max_lag=2), dict(max_lag=4097), dict(bias=-1), dict(bias=16385), dict(unvoiced_cost=0),
               dict(unvoiced_cost=16385), dict(voicing_cost=-1), dict(voicing_cost=(1 << 20) + 1), dict(jump_cost=-1), dict(jump_cost=(1 << 20) + 1),
               dict(table=poisoned(0, 0, 0, -5)), dict(table=poisoned(85, 7, 0, 65536)), dict(table=poisoned(40, 3, 1, -1)), dict(table=poisoned(40, 3, 2, -1)),
               dict(table=poisoned(85, 7, 3, -(1 << 31)))):
        assert call(**kw) == capi.PV_ERR_ARGUMENT, list(kw)
        assert np.all(rec == -77) and np.all(st == -77), list(kw)
    assert call(n=0) == capi.PV_OK and call(n=0, table=None, records=None, states=None) == capi.PV_OK and np.all(rec == -77)
    assert call(table=poisoned(85, 7, 0, 65535)) == capi.PV_OK                # the largest lag
    assert call(states=None) == capi.PV_OK
    want = CM.path(t, ML)
    assert np.array_equal(rec, want[0]) and call() == capi.PV_OK and np.array_equal(st, want[1])
    with pytest.raises(ValueError):
        phaze_amd.contour_path(t, ML, bias=-1)
    with pytest.raises(ValueError):
        phaze_amd.contour_path(t[:, :, :3], ML)
    with pytest.raises(ValueError):
        phaze_amd.contour_path(poisoned(3, 3, 0, -1), ML)
    assert phaze_amd.contour_path(np.zeros((0, 5, 4), np.int32), ML).shape == (0, 4)


# ---- pure host code under AddressSanitizer and UBSan: the stand-alone driver ---------------------------------------------------------------------------

SAN = ["-g", "-O1", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_the_path_runs_clean_under_sanitizers_and_gives_the_models_records(tmp_path):
    """tests/sanitize/contour_host.cpp with pv_contour_path.hip as host code, on its own: the tables of the fading tone and of tone / noise / tone, random
    tables at K = 1, 3 and 8 with empty slots and frames, no frame at all, a table that is refused and the widest costs at the largest lag."""
    exe = str(tmp_path / "contour_host")
    cmd = [RU.HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-x", "hip", "-std=c++17"] + SAN + [
        os.path.join(ROOT, "tests", "sanitize", "contour_host.cpp"), os.path.join(CSRC, "stretch", "pv_contour_path.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    path = str(tmp_path / "table.bin")
    rng = np.random.default_rng(5)

    def run(table, max_lag=ML, **kw):
        c = dict(CM.DEFAULTS)
        c.update(kw)
        table = np.ascontiguousarray(table, np.int32)
        with open(path, "wb") as f:
            f.write(table.tobytes())
        r = subprocess.run([exe, path] + [str(v) for v in (table.shape[0], table.shape[1], max_lag, c["bias"], c["unvoiced_cost"], c["voicing_cost"], c["jump_cost"])],
                           capture_output=True, text=True, env=ENV, timeout=300)
        txt = r.stdout + r.stderr
        assert "AddressSanitizer" not in txt and "runtime error:" not in txt and "LeakSanitizer" not in txt, txt[-3000:]
        assert r.returncode == 0, (r.returncode, txt[-2000:])
        return r.stdout

    def same(table, max_lag=ML, **kw):
        want_r, want_s = CM.path(table, max_lag, **kw)
        got = np.array([[int(v) for v in line.split()] for line in run(table, max_lag, **kw).splitlines()], np.int64).reshape(-1, 5)
        assert np.array_equal(got[:, :4], want_r) and np.array_equal(got[:, 4], want_s)

    same(CM.table(CM.FADES[3]))
    same(CM.table("tnt"))
    for K in (1, 3, 8):
        same(CM.random_table(rng, 300, K, lead=2), **COSTS[K % len(COSTS)])
    wide = CM.random_table(rng, 200, 8)
    wide[:, :, 0] = np.where(wide[:, :, 0] > 0, rng.choice([2, 65535], size=wide.shape[:2]), 0)
    wide[:, :, 1:] = np.where(wide[:, :, :1] > 0, (1 << 31) - 1, 0)
    same(wide, 4096, bias=16384, unvoiced_cost=16384, voicing_cost=1 << 20, jump_cost=1 << 20)
    assert run(np.zeros((0, 8, 4), np.int32)) == ""
    bad = np.array(CM.table("tnt"))
    bad[85, 7, 0] = -1
    assert run(bad).strip() == "refused 2"


# ---- kernel resources -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_contour_kernel_uses_no_spill_no_scratch_no_agprs():
    """One kernel, pv_contour_kernel: DESIGN.md "Pitch contour" quotes its figures (38 VGPRs, 48 bytes of static LDS beside the dynamic arrays)."""
    kernels = RU.resources("stretch/pv_contour_kernels.hip")
    assert len(kernels) == 1 and all("pv_contour_kernel" in n for n in kernels), sorted(kernels)
    for n, v in kernels.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs"] <= 64, (n, v)


# ---- the example ------------------------------------------------------------------------------------------------------------------------------

def build_example(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_contour")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_contour.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_contour_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_example(tmp_path)
    if not _has_gpu():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device error" in r.stderr                    # no CPU fallback behind the C ABI
