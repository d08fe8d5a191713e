"""CPU checks of the time-stretch C ABI: the header declares and the library exports every pv_stretch_* entry point, and configuration errors come
back before any device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
STRETCH = ["pv_stretch_create", "pv_stretch_destroy", "pv_stretch_reset", "pv_stretch_last_error", "pv_stretch_process", "pv_stretch_process_device",
           "pv_stretch_set_stream", "pv_stretch_synchronize", "pv_stretch_export_state", "pv_stretch_import_state"]


def _lib():
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    return phaze_amd.load_library()


def test_header_declares_and_library_exports_the_stretch_surface():
    from phaze_amd import capi
    declared = set(re.findall(r"PV_API\s+[\w\s\*]+?\b(pv_stretch_\w+)\s*\(", open(HEADER).read()))
    assert declared == set(STRETCH)
    assert set(STRETCH) <= set(capi.EXPORTS)
    _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    assert set(STRETCH) <= set(re.findall(r" T (pv_\w+)", out))


def test_abi_version_is_six():
    from phaze_amd import capi
    L = _lib()
    assert L.pv_abi_version() == capi.ABI_VERSION == 6 == int(re.search(r"#define PV_ABI_VERSION (\d+)", open(HEADER).read()).group(1))


@pytest.mark.parametrize("args,code,text", [
    ((1000, 256, 256), 1, "FFT size must be a power of two and bigger than 1"),
    ((0, 256, 256), 1, "FFT size must be a power of two and bigger than 1"),
    ((128, 32, 32), 3, "256..8192"),
    ((16384, 4096, 4096), 3, "256..8192"),
    ((1024, 256, 1024), 2, "synthesis_hop"),                        # R_s = 1 < 2
    ((1024, 256, 600), 2, "synthesis_hop"),                         # R_s < 2
    ((1024, 256, 0), 2, "synthesis_hop"),
    ((1024, 0, 256), 2, "analysis_hop"),
    ((1024, 1025, 256), 2, "analysis_hop"),
])
def test_config_errors_without_a_device(args, code, text):
    from phaze_amd import capi
    L = _lib()
    h = C.c_void_p()
    cfg = capi.make_stretch_config(*args)
    assert L.pv_stretch_create(C.byref(cfg), C.byref(h)) == code
    assert text in L.pv_stretch_last_error(None).decode()
    assert not h.value


def test_layout_and_flag_guards():
    from phaze_amd import capi
    L = _lib()
    h = C.c_void_p()
    cfg = capi.make_stretch_config(1024, 256, 320)
    cfg.struct_size -= 4
    assert L.pv_stretch_create(C.byref(cfg), C.byref(h)) == capi.PV_ERR_ARGUMENT and "struct_size" in L.pv_stretch_last_error(None).decode()
    cfg = capi.make_stretch_config(1024, 256, 320, flags=1)
    assert L.pv_stretch_create(C.byref(cfg), C.byref(h)) == capi.PV_ERR_ARGUMENT and "flags" in L.pv_stretch_last_error(None).decode()
    assert L.pv_stretch_create(None, C.byref(h)) == capi.PV_ERR_ARGUMENT


def test_python_class_raises_like_pv_create():
    import phaze_amd
    with pytest.raises(ValueError):
        phaze_amd.TimeStretch(1000, 250, 250)
    with pytest.raises(phaze_amd.PvError):
        phaze_amd.TimeStretch(1024, 256, 1024)
