"""CPU checks of the linked-channel surface: the header declares and the library exports pv_link_channels with the argument types the ctypes binding
gives it, the ABI stays 6 with the pv_stretch_* and pv_tempo_* sets unchanged, calls without a handle are rejected, and examples/pv_link.c builds as
pedantic C99 and fails loudly without a GPU.  (The kernels' registers: tests/test_stretch_resources.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")


def _lib():
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    return phaze_amd.load_library()


def test_header_declares_and_library_exports_pv_link_channels():
    from phaze_amd import capi
    text = open(HEADER).read()
    m = re.search(r"PV_API\s+int\s+pv_link_channels\s*\(([^)]*)\)", text)
    assert m
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["pv_stretch *h", "int32_t channels_per_group"], params
    assert "pv_link_channels" in capi.EXPORTS
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    assert "pv_link_channels" in re.findall(r" T (pv_\w+)", out)
    assert L.pv_link_channels.argtypes == [C.c_void_p, C.c_int32]
    assert L.pv_link_channels.restype == C.c_int


def test_abi_six_and_the_stretch_and_tempo_sets():
    from phaze_amd import capi
    L = _lib()
    text = open(HEADER).read()
    assert L.pv_abi_version() == capi.ABI_VERSION == 6 == int(re.search(r"#define PV_ABI_VERSION (\d+)", text).group(1))
    assert len(set(re.findall(r"PV_API\s+[\w\s\*]+?\b(pv_stretch_\w+)\s*\(", text))) == 10
    assert len(set(re.findall(r"PV_API\s+[\w\s\*]+?\b(pv_tempo_\w+)\s*\(", text))) == 2
    head = text[:text.index("#define PV_ABI_VERSION")]
    assert "pv_link_channels" in head[head.rindex("6 ="):]                                 # recorded on the line for 6


def test_link_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    assert L.pv_link_channels(None, 2) == capi.PV_ERR_ARGUMENT


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_link_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_link")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_link.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device error" in r.stderr                    # no CPU fallback behind the C ABI
