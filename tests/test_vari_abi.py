"""CPU checks of the variable-ratio resampler and pitch-curve surface: the header declares, the library exports and the ctypes binding gives argument
types to every pv_vari_* / pv_glide_* name, the ABI stays 6, calls without a handle and bad configs are refused before any device is touched, the C
prototype table agrees with the numpy model (tests/vari_model.py), the new kernel file compiles for gfx950 without spills, scratch or AGPRs, and
examples/pv_glide.c builds as pedantic C99 (tests/test_gpu_glide.py runs it)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import vari_model as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SURFACE = {"pv_vari_create": 2, "pv_vari_destroy": 1, "pv_vari_reset": 1, "pv_vari_last_error": 1, "pv_vari_set_stream": 2, "pv_vari_synchronize": 1,
           "pv_vari_process": 10, "pv_vari_process_device": 10, "pv_vari_export_state": 5, "pv_vari_import_state": 5, "pv_vari_prototype": 2,
           "pv_vari_half_width": 3,
           "pv_glide_create": 2, "pv_glide_destroy": 1, "pv_glide_reset": 1, "pv_glide_last_error": 1, "pv_glide_set_stream": 2, "pv_glide_synchronize": 1,
           "pv_glide_process": 10, "pv_glide_process_device": 10, "pv_glide_stretch": 1, "pv_glide_resampler": 1}
DEVICE_POINTERS = {"pv_vari_process_device": (1, 6), "pv_glide_process_device": (1, 2)}       # void * in the binding


def _lib():
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    return phaze_amd.load_library()


def _declaration(name):
    m = re.search(r"PV_API\s+([\w ]+?\*?)\s*\b" + name + r"\s*\(([^)]*)\)", open(HEADER).read())
    assert m, name
    return m.group(1).strip(), [re.sub(r"\s+", " ", re.sub(r"\b\w+$", "", p.strip())).strip() for p in m.group(2).split(",")]


def _c_types():
    from phaze_amd import capi
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    return {"pv_vari *": vp, "const pv_vari *": vp, "pv_glide *": vp, "const pv_glide *": vp, "pv_vari **": C.POINTER(vp), "pv_glide **": C.POINTER(vp),
            "const pv_vari_config *": C.POINTER(capi._VariConfig), "const pv_glide_config *": C.POINTER(capi._GlideConfig), "void *": vp,
            "const float *": fp, "float *": fp, "int32_t": C.c_int32, "int64_t": C.c_int64, "const int32_t *": C.POINTER(C.c_int32),
            "int64_t *": C.POINTER(C.c_int64), "const uint8_t *": C.POINTER(C.c_uint8)}


def test_header_declares_library_exports_and_binding_types_the_surface():
    import phaze_amd
    from phaze_amd import capi
    text = open(HEADER).read()
    declared = set(re.findall(r"PV_API\s+[\w ]+?\*?\s*\b(pv_(?:vari|glide)_\w+)\s*\(", text))
    assert declared == set(SURFACE)
    assert set(SURFACE) <= set(capi.EXPORTS)
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    assert set(SURFACE) <= set(re.findall(r" T (pv_\w+)", out))
    types = _c_types()
    for name, nargs in SURFACE.items():
        ret, decl = _declaration(name)
        got = getattr(L, name).argtypes
        assert len(got) == len(decl) == nargs, (name, decl)
        for i, (d, g) in enumerate(zip(decl, got)):
            want = C.c_void_p if i in DEVICE_POINTERS.get(name, ()) else types[d]
            assert g == want, (name, i, d, g)
        want_ret = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "const char *": C.c_char_p, "pv_stretch *": C.c_void_p, "pv_vari *": C.c_void_p}[ret]
        assert getattr(L, name).restype == want_ret, (name, ret)
    assert L.pv_abi_version() == capi.ABI_VERSION == 6 == int(re.search(r"#define PV_ABI_VERSION (\d+)", text).group(1))
    note = text[text.index("#define PV_ABI_VERSION") - 2000:text.index("#define PV_ABI_VERSION")]
    assert "pv_vari_" in note and "pv_glide_" in note                                       # recorded on the line for 6
    assert "PV_VARI_CONFIG_INIT" in text and "PV_GLIDE_CONFIG_INIT" in text
    assert C.sizeof(capi._VariConfig) == 32 and C.sizeof(capi._GlideConfig) == 36
    assert phaze_amd.VariResampler is capi.VariResampler and phaze_amd.PitchGlide is capi.PitchGlide


def test_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    x = (C.c_float * 8)()
    cnt = (C.c_int32 * 1)(8)
    n = C.c_int64()
    bad = capi.PV_ERR_ARGUMENT
    assert L.pv_vari_destroy(None) == bad and L.pv_vari_reset(None) == bad and L.pv_vari_synchronize(None) == bad
    assert L.pv_vari_set_stream(None, None) == bad
    assert L.pv_vari_process(None, x, 1, 1, cnt, 8, x, 8, 8, C.byref(n)) == bad
    assert L.pv_vari_process_device(None, None, 1, 1, cnt, 8, None, 8, 8, C.byref(n)) == bad
    assert L.pv_vari_export_state(None, 0, x, None, None) == bad and L.pv_vari_import_state(None, 0, x, 0, 0) == bad
    assert L.pv_glide_destroy(None) == bad and L.pv_glide_reset(None) == bad and L.pv_glide_synchronize(None) == bad
    assert L.pv_glide_set_stream(None, None) == bad
    assert L.pv_glide_process(None, x, x, 1, 1, cnt, None, 0, 8, 8) == bad
    assert L.pv_glide_process_device(None, None, None, 1, 1, cnt, None, 0, 8, 8) == bad
    assert L.pv_glide_stretch(None) is None and L.pv_glide_resampler(None) is None
    assert L.pv_vari_create(None, None) == bad and L.pv_glide_create(None, None) == bad
    assert L.pv_vari_prototype(None, 4) == -bad and L.pv_vari_prototype(x, -1) == -bad


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_config_errors_appear_without_a_device():
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    h = C.c_void_p()

    def create(cfg):
        rc = L.pv_vari_create(C.byref(cfg), C.byref(h))
        return rc, L.pv_vari_last_error(None).decode()

    for B, lo, hi, word in [(0, 1, 1, "block"), (4097, 4096, 4096, "block"), (-5, 1, 1, "block"), (320, 0, 440, "min_count"), (320, 300, 200, "min_count"),
                            (320, 200, 8193, "8192"), (320, 39, 440, "8 * min_count"), (64, 8, 513, "8 * block"), (1, 1, 9, "8 * block")]:
        rc, msg = create(capi.make_vari_config(B, lo, hi))
        assert rc == capi.PV_ERR_ARGUMENT and word in msg, (B, lo, hi, msg)
        assert L.pv_vari_half_width(B, lo, hi) == -capi.PV_ERR_ARGUMENT and word in L.pv_vari_last_error(None).decode()
        with pytest.raises(ValueError):
            VM.half_width(B, lo, hi)
    cfg = capi.make_vari_config(320, 200, 440)
    cfg.struct_size -= 4
    rc, msg = create(cfg)
    assert rc == capi.PV_ERR_ARGUMENT and "struct_size" in msg
    rc, msg = create(capi.make_vari_config(320, 200, 440, flags=1))
    assert rc == capi.PV_ERR_ARGUMENT and "flags" in msg
    assert create(capi.make_vari_config(320, 200, 440, max_channels=-1))[0] == capi.PV_ERR_ARGUMENT
    for B, lo, hi in [(320, 200, 440), (64, 8, 512), (1, 1, 8), (4096, 512, 8192), (320, 40, 2560), (4095, 4000, 4096)]:
        assert L.pv_vari_half_width(B, lo, hi) == VM.half_width(B, lo, hi) == phaze_amd.vari_half_width(B, lo, hi)

    def gcreate(cfg):
        rc = L.pv_glide_create(C.byref(cfg), C.byref(h))
        return rc, L.pv_glide_last_error(None).decode()

    cfg = capi.make_glide_config(1024, 320, 200, 440)
    cfg.struct_size += 4
    assert gcreate(cfg)[0] == capi.PV_ERR_ARGUMENT and "struct_size" in gcreate(cfg)[1]
    assert gcreate(capi.make_glide_config(1024, 320, 200, 440, flags=2))[0] == capi.PV_ERR_ARGUMENT
    rc, msg = gcreate(capi.make_glide_config(1024, 320, 200, 1025))
    assert rc == capi.PV_ERR_ARGUMENT and "fft_size" in msg                                # max_hop > N
    rc, msg = gcreate(capi.make_glide_config(1024, 320, 39, 440))
    assert rc == capi.PV_ERR_ARGUMENT and "8 * min_count" in msg                            # hs > 8 min_hop: the resampler's config error comes through
    assert gcreate(capi.make_glide_config(1024, 320, 300, 200))[0] == capi.PV_ERR_ARGUMENT
    assert gcreate(capi.make_glide_config(1024, 32, 16, 300))[0] == capi.PV_ERR_ARGUMENT    # max_hop > 8 hs
    assert gcreate(capi.make_glide_config(1000, 320, 200, 440))[0] == capi.PV_ERR_FFT_SIZE  # the stretch's own config errors come through
    assert gcreate(capi.make_glide_config(1024, 600, 200, 440))[0] == capi.PV_ERR_ARGUMENT  # hs above N / 2
    if not _has_gpu():
        assert create(capi.make_vari_config(320, 200, 440))[0] == capi.PV_ERR_DEVICE         # fails loudly: no CPU fallback
        assert gcreate(capi.make_glide_config(1024, 320, 200, 440))[0] == capi.PV_ERR_DEVICE
        with pytest.raises(phaze_amd.PvError):
            phaze_amd.VariResampler(320, 200, 440)
        with pytest.raises(phaze_amd.PvError):
            phaze_amd.PitchGlide(1024, 320, 200, 440)
    with pytest.raises(phaze_amd.PvError):
        phaze_amd.VariResampler(320, 39, 440)


def test_c_prototype_equals_the_models_table_within_one_ulp():
    import phaze_amd
    P = phaze_amd.vari_prototype()
    want = VM.prototype()
    assert P.dtype == np.float32 and P.shape == want.shape == (32 * 256 + 2,)
    d = np.abs(P.astype(np.float64) - want.astype(np.float64))
    assert np.all(d <= 2.0 ** -23 * np.abs(want.astype(np.float64))), int(np.sum(P != want))
    assert np.all(P[32 * 256:] == 0.0) and P[0] == np.float32(0.91)
    # two-call sizing: the return value is the table's length whatever the capacity, and nothing is written past the capacity
    L = phaze_amd.load_library()
    buf = np.full(P.size + 4, -3.0, np.float32)
    assert L.pv_vari_prototype(None, 0) == P.size
    assert L.pv_vari_prototype(buf.ctypes.data_as(C.POINTER(C.c_float)), P.size - 5) == P.size
    assert np.all(buf[P.size - 5:] == -3.0) and np.array_equal(buf[:P.size - 5], P[:P.size - 5])
    assert L.pv_vari_prototype(buf.ctypes.data_as(C.POINTER(C.c_float)), P.size + 4) == P.size and np.all(buf[P.size:] == -3.0)


# ---- kernel resources -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_vari_kernels_use_no_spill_no_scratch_no_agprs():
    """Two instances of pv_vari_kernel: four outputs per thread, and three for the shapes whose span would not fit beside the table otherwise."""
    src = os.path.join(ROOT, "phaze_amd", "csrc")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                          "-o", os.devnull, "resample/pv_vari_kernels.hip"], cwd=src, capture_output=True, text=True, timeout=900)
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
    assert len(kernels) == 2 and all("pv_vari_kernel" in n for n in kernels), sorted(kernels)
    for n, v in kernels.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs"] <= 128, (n, v)


# ---- the example ------------------------------------------------------------------------------------------------------------------------------

def build_example(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_glide")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_glide.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_glide_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_example(tmp_path)
    if not _has_gpu():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device error" in r.stderr                    # no CPU fallback behind the C ABI
