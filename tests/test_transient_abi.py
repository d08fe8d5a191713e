"""CPU checks of the transient surface: the header declares and the library exports pv_transient_process / _device, pv_onset_strength / _device,
pv_transient_plan, pv_onsets_from_strength and the two chain-layout test hooks with the argument types the ctypes binding gives them, the ABI stays 6, the
C planner and onset rule agree exactly with the numpy ones (tests/transient_model.py), and examples/pv_transient.c builds as pedantic C99 (and, on a
GPU, runs).  (The kernels' registers: tests/test_stretch_resources.py.)"""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import transient_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
SURFACE = {"pv_transient_process": 11, "pv_transient_process_device": 11, "pv_onset_strength": 7, "pv_onset_strength_device": 7, "pv_transient_plan": 12,
           "pv_onsets_from_strength": 7, "pv_transient_chain_layout": 5, "pv_onset_chain_layout": 4}


def _lib():
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    return phaze_amd.load_library()


def _declaration(name):
    m = re.search(r"PV_API\s+(\w+)\s+" + name + r"\s*\(([^)]*)\)", open(HEADER).read())
    assert m, name
    return m.group(1), [re.sub(r"\s+", " ", re.sub(r"\b\w+$", "", p.strip())).strip() for p in m.group(2).split(",")]


C_TYPES = {"pv_stretch *": C.c_void_p, "const float *": C.POINTER(C.c_float), "float *": C.POINTER(C.c_float), "int32_t": C.c_int32,
           "const int32_t *": C.POINTER(C.c_int32), "int32_t *": C.POINTER(C.c_int32), "int64_t": C.c_int64, "const uint8_t *": C.POINTER(C.c_uint8),
           "uint8_t *": C.POINTER(C.c_uint8), "const int64_t *": C.POINTER(C.c_int64), "int64_t *": C.POINTER(C.c_int64), "double": C.c_double}
DEVICE_POINTERS = {"pv_transient_process_device": (1, 2), "pv_onset_strength_device": (1, 5)}       # void * in the binding


def test_header_declares_and_library_exports_the_transient_surface():
    from phaze_amd import capi
    text = open(HEADER).read()
    declared = set(re.findall(r"PV_API\s+\w+\s+(pv_(?:transient|onset)\w+)\s*\(", text))
    assert declared == set(SURFACE)
    assert set(SURFACE) <= set(capi.EXPORTS)
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    assert set(SURFACE) <= set(re.findall(r" T (pv_\w+)", out))
    for name, nargs in SURFACE.items():
        ret, decl = _declaration(name)
        got = getattr(L, name).argtypes
        assert len(got) == len(decl) == nargs, (name, decl)
        for i, (d, g) in enumerate(zip(decl, got)):
            want = C.c_void_p if i in DEVICE_POINTERS.get(name, ()) else C_TYPES[d]
            assert g == want, (name, i, d, g)
        assert getattr(L, name).restype == (C.c_int64 if ret == "int64_t" else C.c_int), name
    assert L.pv_abi_version() == capi.ABI_VERSION == 6 == int(re.search(r"#define PV_ABI_VERSION (\d+)", text).group(1))
    assert "pv_transient_process" in text[text.index("#define PV_ABI_VERSION") - 2000:text.index("#define PV_ABI_VERSION")]   # recorded on the line for 6


def test_transient_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    x = (C.c_float * 8)()
    c = (C.c_int32 * 2)()
    assert L.pv_transient_process(None, x, x, 1, 2, None, 0, None, 0, 8, 8) == capi.PV_ERR_ARGUMENT
    assert L.pv_transient_process_device(None, None, None, 1, 2, None, 0, None, 0, 8, 8) == capi.PV_ERR_ARGUMENT
    assert L.pv_onset_strength(None, x, 1, 2, 8, c, 2) == capi.PV_ERR_ARGUMENT
    assert L.pv_onset_strength_device(None, None, 1, 2, 8, None, 2) == capi.PV_ERR_ARGUMENT
    assert L.pv_transient_chain_layout(None, 1, 1, None, None) == capi.PV_ERR_ARGUMENT
    assert L.pv_onset_chain_layout(None, 1, 1, None) == capi.PV_ERR_ARGUMENT


# ---- the host planner and onset rule against the numpy ones ---------------------------------------------------------------------------------

PLAN_SHAPES = [(1024, 256, 205, 320, None, None), (1024, 256, 205, 384, 0, 0), (2048, 512, 300, 300, None, 0), (1024, 341, 200, 256, None, 1024),
               (256, 100, 64, 97, 16, None), (4096, 1024, 512, 1536, 2048, 77), (1024, 256, 256, 320, None, None),
               (512, 64, 1, 1, 3, 5)]                      # (N, ha, floor, hs, lead, release); the last two cannot repay a debt


@pytest.mark.parametrize("N,ha,floor,hs,lead,release", PLAN_SHAPES)
def test_c_planner_equals_the_numpy_planner(N, ha, floor, hs, lead, release):
    import phaze_amd
    rng = np.random.default_rng(N + hs)
    for trial in range(25):
        n = int(rng.integers(0, 50 * N))
        onsets = np.sort(rng.integers(-N, n + N, int(rng.integers(0, 12))))
        if trial % 5 == 0 and onsets.size > 2:
            onsets[1] = onsets[0]                                       # a repeated position
        hops, resets = phaze_amd.transient_plan(onsets, n, N, ha, floor, hs, lead, release)
        want_h, want_r, _ = TM.transient_plan(onsets, n, N, ha, floor, hs, lead, release)
        assert hops.dtype == np.int32 and resets.dtype == np.uint8
        assert np.array_equal(hops, want_h) and np.array_equal(resets, want_r), trial


def test_c_planner_sizing_and_refusals():
    import phaze_amd
    L = _lib()
    lp, ip, bp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    on = np.array([3000, 9000], np.int64)
    n = L.pv_transient_plan(on.ctypes.data_as(lp), 2, 20000, 1024, 256, 205, 320, -1, -1, None, None, 0)
    assert n > 0
    hops, resets = np.full(n + 2, -7, np.int32), np.full(n + 2, 9, np.uint8)
    assert L.pv_transient_plan(on.ctypes.data_as(lp), 2, 20000, 1024, 256, 205, 320, -1, -1, hops.ctypes.data_as(ip), resets.ctypes.data_as(bp), n - 3) == n
    assert np.all(hops[n - 3:] == -7) and np.all(resets[n - 3:] == 9) and np.all(hops[:n - 3] > 0)      # never past the capacity
    bad = -2                                                             # -PV_ERR_ARGUMENT
    assert L.pv_transient_plan(on.ctypes.data_as(lp), 2, 20000, 1024, 256, 205, 200, -1, -1, None, None, 0) == bad          # hs < floor
    assert L.pv_transient_plan(on.ctypes.data_as(lp), 2, 20000, 1024, 200, 205, 320, -1, -1, None, None, 0) == bad          # nominal hop below the floor
    assert L.pv_transient_plan(on.ctypes.data_as(lp), 2, 20000, 1024, 256, 205, 320, 513, -1, None, None, 0) == bad     # lead > N / 2
    assert L.pv_transient_plan(on.ctypes.data_as(lp), 2, 20000, 1024, 256, 205, 320, -1, 1025, None, None, 0) == bad    # release > N
    assert L.pv_transient_plan(on[::-1].copy().ctypes.data_as(lp), 2, 20000, 1024, 256, 205, 320, -1, -1, None, None, 0) == bad   # unsorted
    with pytest.raises(ValueError):
        phaze_amd.transient_plan(on, 20000, 1024, 256, 205, 200)
    with pytest.raises(ValueError):
        TM.transient_plan(on, 20000, 1024, 256, 205, 200)


def test_c_onset_rule_equals_the_numpy_rule():
    import phaze_amd
    rng = np.random.default_rng(9)
    for N, ha in [(1024, 256), (256, 100), (4096, 1024)]:
        for tau in (0.4, 0.2, 0.66):
            c = rng.integers(0, N // 2, 400).astype(np.int32)
            c[rng.integers(0, 400, 40)] = int(np.ceil(tau * (N // 2 - 1)))      # values on the threshold
            assert np.array_equal(phaze_amd.onsets_from_strength(c, N, ha, tau), TM.onsets_from_strength(c, N, ha, tau))
    assert phaze_amd.onsets_from_strength(np.zeros(0, np.int32), 1024, 256).size == 0
    with pytest.raises(ValueError):
        phaze_amd.onsets_from_strength([1, 2], 1024, 256, 0.0)


# ---- the example ------------------------------------------------------------------------------------------------------------------------------

def _build(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_transient")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_transient.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_transient_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    exe = _build(tmp_path)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device error" in r.stderr                    # no CPU fallback behind the C ABI


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
@pytest.mark.parametrize("args", [[], ["1024", "256", "192", "160", "2"], ["4096", "1024", "1536", "768", "2"], ["256", "64", "96", "48", "4"]])
def test_transient_example_one_call_equals_frame_by_frame(tmp_path, args):
    exe = _build(tmp_path)
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    nb = int(args[4]) if args else 3
    assert j["one_call_equals_frame_by_frame"] is True and j["output_rms"] > 1e-3
    assert j["onsets"] == nb + 1 and j["held_frames"] >= 2 * nb, j         # the start of the buffer and every burst
