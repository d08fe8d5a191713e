"""CPU checks of the harmony surface: the header declares, the library exports and the ctypes binding gives argument types to every pv_harmony_* name,
the ABI stays 6, pv_harmony_ratios equals the Python model (tests/harmony_model.py) bit for bit, sizes in two calls and refuses every bad argument, bad and
oversized configs are refused before any device is touched, the kernel file compiles for gfx950 without spills, scratch or AGPRs, and
examples/pv_harmony.c builds as pedantic C99 (tests/test_gpu_harmony.py holds the refusals of pv_harmony_process, which need a handle)."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import f0_model as FM
import harmony_model as HM
import psola_model as PM
import resource_usage as RU
import test_harmony_model as THM
import test_psola_abi as TPA
import tsm_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
SURFACE = {"pv_harmony_create": 2, "pv_harmony_destroy": 1, "pv_harmony_last_error": 1, "pv_harmony_set_stream": 2, "pv_harmony_synchronize": 1,
           "pv_harmony_process": 13, "pv_harmony_process_device": 13, "pv_harmony_ratios": 7}
DEVICE_POINTERS = {"pv_harmony_process_device": (1, 9)}                      # void * in the binding
IP, DP, FP, LP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64)
C_MAJOR = THM.C_MAJOR

_lib = TPA._lib
_has_gpu = TPA._has_gpu
_declaration = TPA._declaration


def test_header_declares_library_exports_and_binding_types_the_surface():
    import phaze_amd
    from phaze_amd import capi
    text = open(HEADER).read()
    declared = set(re.findall(r"PV_API\s+[\w ]+?\*?\s*\b(pv_harmony_\w+)\s*\(", text))
    assert declared == set(SURFACE)
    assert set(SURFACE) <= set(capi.EXPORTS)
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pv_\w+)", out))
    assert set(SURFACE) <= exported and {n for n in exported if n.startswith("pv_harmony_")} == set(SURFACE)
    assert exported == set(capi.EXPORTS)                                    # and nothing else came with them
    vp = C.c_void_p
    types = {"pv_harmony *": vp, "const pv_harmony *": vp, "pv_harmony **": C.POINTER(vp), "const pv_harmony_config *": C.POINTER(capi._HarmonyConfig),
             "const pv_tune_params *": C.POINTER(capi._TuneParams), "void *": vp, "const float *": FP, "float *": FP, "int32_t": C.c_int32, "int64_t": C.c_int64,
             "const int32_t *": IP, "const int64_t *": LP, "double *": DP}
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
    assert "pv_harmony_" in note and "pv_tsm_" in note and "6 = the time-stretch handle" in note                   # recorded on the line for 6
    assert C.sizeof(capi._HarmonyConfig) == 32
    body = re.search(r"typedef struct pv_harmony_config \{(.*?)\} pv_harmony_config;", text, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+);", body, re.M)
    assert [(n, C.c_int32) for t, n in fields] == list(capi._HarmonyConfig._fields_) and all(t == "int32_t" for t, _ in fields)
    assert [n for _, n in fields] == ["struct_size", "max_period", "max_rate", "max_voices", "max_channels", "max_outputs", "device_id", "flags"]
    assert re.search(r"#define PV_HARMONY_CONFIG_INIT \{ \(int32_t\)sizeof\(pv_harmony_config\), 0, 0, 0, 0, 0, 0, 0 \}", text)
    for name in ("Harmony", "harmony_ratios"):
        assert getattr(phaze_amd, name) is getattr(capi, name) and name in phaze_amd.__all__
    for method in ("process", "process_device", "process_tuned"):
        assert hasattr(capi.Harmony, method)
    sig = inspect.signature(capi.Harmony.process_tuned).parameters
    assert sig["degrees"].default == (0, 2, 4) and sig["gains"].default is None and sig["rate"].default == 1.0 and sig["epochs"].default is False
    sig = inspect.signature(capi.harmony_ratios).parameters
    assert list(sig)[:3] == ["records", "sample_rate", "degrees"] and sig["scale_mask"].default == 0xFFF and sig["a4"].default == 440.0


def test_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    x = (C.c_float * 8)()
    g = (C.c_int32 * 4)(4, 0, 0, 2)
    first = (C.c_int64 * 2)(0, 1)
    gain = (C.c_float * 1)(1.0)
    bad = capi.PV_ERR_ARGUMENT
    assert L.pv_harmony_destroy(None) == bad and L.pv_harmony_synchronize(None) == bad and L.pv_harmony_set_stream(None, None) == bad
    assert L.pv_harmony_process(None, x, 8, 8, 1, g, first, 1, gain, x, 0, 8, 8) == bad
    assert L.pv_harmony_process_device(None, None, 8, 8, 1, g, first, 1, gain, None, 0, 8, 8) == bad
    assert L.pv_harmony_create(None, None) == bad
    assert list(x) == [0.0] * 8


def test_config_errors_and_oversized_configs_appear_without_a_device():
    """The span is pv_tsm's, applied to the hull: the same pairs are refused with PV_ERR_UNSUPPORTED, before any device is touched."""
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    h = C.c_void_p()

    def create(cfg):
        rc = L.pv_harmony_create(C.byref(cfg), C.byref(h))
        return rc, L.pv_harmony_last_error(None).decode()

    for (mp, rate), word in [((1, 1), "max_period"), ((0, 1), "max_period"), ((4097, 1), "max_period"), ((-3, 1), "max_period"), ((512, 0), "max_rate"),
                             ((512, 5), "max_rate"), ((512, -1), "max_rate")]:
        rc, msg = create(capi.make_harmony_config(mp, rate))
        assert rc == capi.PV_ERR_ARGUMENT and word in msg, (mp, rate, msg)
    cfg = capi.make_harmony_config(512, 2)
    cfg.struct_size -= 4
    rc, msg = create(cfg)
    assert rc == capi.PV_ERR_ARGUMENT and "struct_size" in msg
    rc, msg = create(capi.make_harmony_config(512, 2, flags=1))
    assert rc == capi.PV_ERR_ARGUMENT and "flags" in msg
    for nv in (-1, 9):
        rc, msg = create(capi.make_harmony_config(512, 2, max_voices=nv))
        assert rc == capi.PV_ERR_ARGUMENT and "max_voices" in msg
    rc, msg = create(capi.make_harmony_config(512, 2, max_channels=-1))
    assert rc == capi.PV_ERR_ARGUMENT and "max_channels" in msg
    assert create(capi.make_harmony_config(512, 2, max_channels=65536))[0] == capi.PV_ERR_ARGUMENT
    rc, msg = create(capi.make_harmony_config(512, 2, max_outputs=-1))
    assert rc == capi.PV_ERR_ARGUMENT and "max_outputs" in msg
    fits = {(mp, rate): TM.lds_bytes(mp, rate) <= TM.LDS_BYTES for mp in (2, 64, 1024, 2048, 2300, 2400, 3000, 4096) for rate in (1, 2, 3, 4)}
    assert fits[(4096, 1)] and not fits[(4096, 2)] and fits[(2048, 4)] and not fits[(3000, 4)]
    for (mp, rate), ok in fits.items():
        rc, msg = create(capi.make_harmony_config(mp, rate, max_voices=8))
        if not ok:
            assert rc == capi.PV_ERR_UNSUPPORTED and "LDS" in msg and str(TM.lds_bytes(mp, rate)) in msg, (mp, rate, msg)
        elif not _has_gpu():
            assert rc == capi.PV_ERR_DEVICE and "HIP device" in msg, (mp, rate, msg)              # gets as far as the device and fails loudly: no CPU fallback
        else:
            assert rc == capi.PV_OK and L.pv_harmony_destroy(h) == capi.PV_OK
    with pytest.raises(phaze_amd.PvError) as e:
        phaze_amd.Harmony(4096, 4)
    assert e.value.status == capi.PV_ERR_UNSUPPORTED
    with pytest.raises(phaze_amd.PvError):
        phaze_amd.Harmony(1)
    if not _has_gpu():
        with pytest.raises(phaze_amd.PvError):
            phaze_amd.Harmony(512)


# ---- pure host code: the ratios ----------------------------------------------------------------------------------------------------------------

def test_ratios_equal_the_model_exactly():
    """Random tracks with unvoiced and empty records, the masks, strengths and retune speeds of the model tests, every degree from -24 to 24 in groups of
    up to eight voices; the row of degree 0 is tune_ratios's."""
    import phaze_amd
    rng = np.random.default_rng(41)
    checked = 0
    for mask, strength, retune, a4 in ((0xFFF, 1.0, 1.0, 440.0), (C_MAJOR, 0.7, 0.25, 440.0), (0x001, 1.0, 0.5, 432.0), (0x821, 0.0, 1.0, 440.0),
                                       (C_MAJOR, 1.0, 0.05, 415.3)):
        recs = THM._track(rng, 400)
        lead = phaze_amd.tune_ratios(recs, FM.SAMPLE_RATE, mask, strength, retune, a4)
        for group in (list(range(-24, -16)), list(range(-16, -8)), list(range(-8, 0)), [0, 2, 4], list(range(1, 9)), list(range(9, 17)), list(range(17, 25)), [0]):
            want = HM.harmony_ratios(recs, FM.SAMPLE_RATE, group, mask, strength, retune, a4)
            got = phaze_amd.harmony_ratios(recs, FM.SAMPLE_RATE, group, mask, strength, retune, a4)
            assert got.dtype == np.float64 and got.shape == want.shape == (len(group), 400) and np.array_equal(got, want), (hex(mask), group)
            if 0 in group:
                assert np.array_equal(got[group.index(0)], lead)
            checked += got.size
        assert np.all((got >= 0.5) & (got <= 2.0))
    assert checked > 100000
    assert phaze_amd.harmony_ratios(np.zeros((0, 4), np.int32), FM.SAMPLE_RATE, [0, 2]).shape == (2, 0)


def test_ratios_size_in_two_calls_and_write_no_more_than_the_capacity():
    from phaze_amd import capi
    L = _lib()
    recs = np.ascontiguousarray(THM._track(np.random.default_rng(8), 97))
    deg = np.array([0, 2, -3], np.int32)
    want = HM.harmony_ratios(recs, FM.SAMPLE_RATE, deg, C_MAJOR)
    p = capi.make_tune_params(0, 0, FM.SAMPLE_RATE, 0, 0, 0, 0, C_MAJOR)
    rp, dp = recs.ctypes.data_as(IP), deg.ctypes.data_as(IP)
    assert L.pv_harmony_ratios(C.byref(p), rp, 97, dp, 3, None, 0) == 97
    for cap in (40, 97, 120):
        out = np.full(3 * cap + 5, -7.0)
        assert L.pv_harmony_ratios(C.byref(p), rp, 97, dp, 3, out.ctypes.data_as(DP), cap) == 97
        rows = out[:3 * cap].reshape(3, cap)
        m = min(cap, 97)
        assert np.array_equal(rows[:, :m], want[:, :m]) and np.all(rows[:, m:] == -7.0) and np.all(out[3 * cap:] == -7.0)        # row v lives at v * capacity


def test_ratios_reject_every_bad_argument():
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    recs = np.ascontiguousarray(PM.records_of([200.0] * 12))
    rp = recs.ctypes.data_as(IP)
    out = np.full(8 * 12, -7.0)
    bad = -capi.PV_ERR_ARGUMENT

    def ratios(records=rp, n=12, degrees=(0, 2), nvoices=None, rows=out, capacity=12, struct_delta=0, reserved=0, no_p=False, **kw):
        args = dict(f0_hop=0, f0_center=0, sample_rate=FM.SAMPLE_RATE, synthesis_hop=0, min_hop=0, max_hop=0, input_len=0)
        args.update(kw)
        p = capi.make_tune_params(**args)
        p.struct_size += struct_delta
        p.reserved = reserved
        deg = None if degrees is None else np.array(degrees, np.int32)
        return L.pv_harmony_ratios(None if no_p else C.byref(p), records, n, None if deg is None else deg.ctypes.data_as(IP),
                                   (0 if deg is None else deg.size) if nvoices is None else nvoices, None if rows is None else rows.ctypes.data_as(DP), capacity)

    assert ratios() == 12 and np.all(out[:24] > 0) and np.all(out[24:] == -7.0)
    out[:] = -7.0
    for kw in (dict(no_p=True), dict(struct_delta=8), dict(struct_delta=-8), dict(reserved=1), dict(records=None), dict(n=-1), dict(rows=None), dict(capacity=-1),
               dict(sample_rate=0.0), dict(sample_rate=-1.0), dict(sample_rate=float("nan")), dict(sample_rate=float("inf")), dict(a4=-1.0), dict(a4=float("nan")),
               dict(scale_mask=0), dict(scale_mask=0x1000), dict(scale_mask=-1), dict(strength=-0.1), dict(strength=1.1), dict(strength=float("nan")), dict(retune=0.0),
               dict(retune=1.1), dict(retune=float("nan")), dict(degrees=None, nvoices=2), dict(degrees=(), nvoices=0), dict(degrees=(0,), nvoices=0),
               dict(degrees=(0,) * 8, nvoices=9), dict(degrees=(0,), nvoices=-1), dict(degrees=(25,)), dict(degrees=(0, -25)), dict(degrees=(0, 1 << 30)),
               dict(degrees=(0, -(1 << 31)))):
        assert ratios(**kw) == bad, kw
    assert np.all(out == -7.0)                                              # nothing written by a refused call
    assert ratios(rows=None, capacity=0) == 12 and ratios(records=None, n=0) == 0 and ratios(degrees=(24, -24) * 4) == 12
    for kw in (dict(degrees=[]), dict(degrees=[0] * 9), dict(degrees=[25]), dict(scale_mask=0), dict(retune=0.0)):
        args = dict(records=recs, sample_rate=FM.SAMPLE_RATE, degrees=[0, 2])
        args.update(kw)
        with pytest.raises(ValueError):
            phaze_amd.harmony_ratios(**args)
    with pytest.raises(ValueError):
        phaze_amd.harmony_ratios(recs, FM.SAMPLE_RATE, [[0, 2]])


# ---- kernel resources -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_harmony_kernel_uses_no_spill_no_scratch_no_agprs():
    """One kernel, pv_harmony_kernel, within pv_tsm_kernel's pinned ceiling of 64 VGPRs: DESIGN.md "Harmony voices" quotes its figures (no static LDS
    beside the dynamic arrays)."""
    kernels = RU.resources("psola/pv_harmony_kernels.hip")
    assert len(kernels) == 1 and all("pv_harmony_kernel" in n for n in kernels), sorted(kernels)
    for n, v in kernels.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs"] <= 64 and v["LDS Size"] == 0, (n, v)


def test_the_existing_overlap_add_kernels_are_untouched():
    """pv_psola_kernels.hip, pv_epoch_kernels.hip and pv_tsm_kernels.hip have pinned resource figures: the new kernel restates pv_tsm_kernel's arithmetic in
    its own file, includes none of them and instantiates none of their kernels; the product of the mix goes through mul_rounded, never an fmaf."""
    src = open(os.path.join(ROOT, "phaze_amd", "csrc", "psola", "pv_harmony_kernels.hip")).read()
    includes = re.findall(r'#include "([^"]+)"', src)
    assert "pv_harmony.h" in includes and "../pv_mul_rounded.h" in includes and not any(i.endswith(".hip") for i in includes)
    assert "pv_psola.h" not in includes and "pv_epoch.h" not in includes
    code = re.sub(r"//.*", "", src)
    for name in ("pv_psola_kernel", "pv_epoch_kernel", "pv_tsm_kernel", "pv_launch_tsm", "pv_launch_psola"):
        assert name not in code, name
    assert "mul_rounded(gain," in code
    make = open(os.path.join(ROOT, "phaze_amd", "csrc", "Makefile")).read()
    assert "pv_harmony_kernels.hip" in make.split("stretch-resource-usage:")[1]
    assert all(f"psola/pv_harmony_{part}" in make.split("OBJS =")[0] for part in ("kernels.hip", "capi.hip", "plan.hip")) and "psola/pv_harmony.h" in make


# ---- the example ------------------------------------------------------------------------------------------------------------------------------

def build_example(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_harmony")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_harmony.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_harmony_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_example(tmp_path)
    if not _has_gpu():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device error" in r.stderr                    # no CPU fallback behind the C ABI
