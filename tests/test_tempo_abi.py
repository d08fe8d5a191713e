"""CPU checks of the variable-tempo surface: the header declares and the library exports pv_tempo_process / pv_tempo_process_device with the
argument types the ctypes binding gives them, the ABI stays 6, and examples/pv_tempo.c builds as pedantic C99 and fails loudly without a GPU.  (The
kernels' registers: tests/test_stretch_resources.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
TEMPO = ["pv_tempo_process", "pv_tempo_process_device"]


def _lib():
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    return phaze_amd.load_library()


def _declaration(name):
    """The parameter types of `name` in the header, one string per parameter ("const float *", "int64_t", ...)."""
    m = re.search(r"PV_API\s+int\s+" + name + r"\s*\(([^)]*)\)", open(HEADER).read())
    assert m, name
    return [re.sub(r"\s+", " ", re.sub(r"\b\w+$", "", p.strip())).strip() for p in m.group(1).split(",")]


C_TYPES = {"pv_stretch *": C.c_void_p, "const float *": C.POINTER(C.c_float), "float *": C.POINTER(C.c_float), "int32_t": C.c_int32,
           "const int32_t *": C.POINTER(C.c_int32), "int64_t": C.c_int64}


def test_header_declares_and_library_exports_the_tempo_surface():
    from phaze_amd import capi
    declared = set(re.findall(r"PV_API\s+[\w\s\*]+?\b(pv_tempo_\w+)\s*\(", open(HEADER).read()))
    assert declared == set(TEMPO)
    assert set(TEMPO) <= set(capi.EXPORTS)
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    assert set(TEMPO) <= set(re.findall(r" T (pv_\w+)", out))
    # the argument types the binding declares are the header's (device pointers are void * in the binding)
    for name in TEMPO:
        decl = _declaration(name)
        got = getattr(L, name).argtypes
        assert len(got) == len(decl) == 9, (name, decl)
        for i, (d, g) in enumerate(zip(decl, got)):
            want = C.c_void_p if (name.endswith("_device") and i in (1, 2)) else C_TYPES[d]
            assert g == want, (name, i, d, g)
        assert getattr(L, name).restype == C.c_int


def test_the_tempo_surface_keeps_abi_six_and_the_stretch_prefix_set():
    from phaze_amd import capi
    L = _lib()
    text = open(HEADER).read()
    assert L.pv_abi_version() == capi.ABI_VERSION == 6 == int(re.search(r"#define PV_ABI_VERSION (\d+)", text).group(1))
    assert not any(n.startswith("pv_stretch_") for n in TEMPO)
    assert len(set(re.findall(r"PV_API\s+[\w\s\*]+?\b(pv_stretch_\w+)\s*\(", text))) == 10
    assert "pv_tempo_process" in text[text.index("#define PV_ABI_VERSION") - 2000:text.index("#define PV_ABI_VERSION")]   # recorded on the line for 6


def test_tempo_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    x = (C.c_float * 8)()
    hops = (C.c_int32 * 2)(256, 256)
    assert L.pv_tempo_process(None, x, x, 1, 2, hops, 0, 8, 8) == capi.PV_ERR_ARGUMENT
    assert L.pv_tempo_process_device(None, None, None, 1, 2, hops, 0, 8, 8) == capi.PV_ERR_ARGUMENT


def _build(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_tempo")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_tempo.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_tempo_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    exe = _build(tmp_path)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device error" in r.stderr                    # no CPU fallback behind the C ABI
