"""CPU checks of the time-scale modification surface: the header declares, the library exports and the ctypes binding gives argument types to every
pv_tsm_* name, the ABI stays 6, pv_tsm_plan equals the Python model (tests/tsm_model.py) bit for bit, sizes in two calls and refuses every bad argument, bad
and oversized configs are refused before any device is touched, the kernel file compiles for gfx950 without spills, scratch or AGPRs, and
examples/pv_tsm.c builds as pedantic C99 (tests/test_gpu_tsm.py runs it, and holds the refusals of pv_tsm_process, which need a handle)."""
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
import test_epoch_abi as TEA
import test_epoch_model as TEM
import test_psola_abi as TPA
import tsm_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
SURFACE = {"pv_tsm_create": 2, "pv_tsm_destroy": 1, "pv_tsm_last_error": 1, "pv_tsm_set_stream": 2, "pv_tsm_synchronize": 1, "pv_tsm_process": 11,
           "pv_tsm_process_device": 11, "pv_tsm_plan": 10}
DEVICE_POINTERS = {"pv_tsm_process_device": (1, 7)}                          # void * in the binding
IP, DP, FP, LP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64)

_lib = TPA._lib
_has_gpu = TPA._has_gpu
_declaration = TPA._declaration


def test_header_declares_library_exports_and_binding_types_the_surface():
    import phaze_amd
    from phaze_amd import capi
    text = open(HEADER).read()
    declared = set(re.findall(r"PV_API\s+[\w ]+?\*?\s*\b(pv_tsm_\w+)\s*\(", text))
    assert declared == set(SURFACE)
    assert set(SURFACE) <= set(capi.EXPORTS)
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pv_\w+)", out))
    assert set(SURFACE) <= exported and {n for n in exported if n.startswith("pv_tsm_")} == set(SURFACE)
    assert exported == set(capi.EXPORTS)                                    # and nothing else came with them
    vp = C.c_void_p
    types = {"pv_tsm *": vp, "const pv_tsm *": vp, "pv_tsm **": C.POINTER(vp), "const pv_tsm_config *": C.POINTER(capi._TsmConfig),
             "const pv_epoch_params *": C.POINTER(capi._EpochParams), "const pv_psola_params *": C.POINTER(capi._PsolaParams), "void *": vp, "const float *": FP,
             "float *": FP, "int32_t": C.c_int32, "int64_t": C.c_int64, "const int32_t *": IP, "int32_t *": IP, "const double *": DP, "int64_t *": LP}
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
    assert "pv_tsm_" in note and "pv_epoch_" in note and "pv_tempo_process" in note and "6 = the time-stretch handle" in note      # recorded on the line for 6
    assert "PV_TSM_CONFIG_INIT" in text
    assert C.sizeof(capi._TsmConfig) == 28
    body = re.search(r"typedef struct pv_tsm_config \{(.*?)\} pv_tsm_config;", text, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+);", body, re.M)
    assert [(n, C.c_int32) for t, n in fields] == list(capi._TsmConfig._fields_) and all(t == "int32_t" for t, _ in fields)
    assert [n for _, n in fields] == ["struct_size", "max_period", "max_rate", "max_channels", "max_outputs", "device_id", "flags"]
    assert re.search(r"#define PV_TSM_CONFIG_INIT \{ \(int32_t\)sizeof\(pv_tsm_config\), 0, 0, 0, 0, 0, 0 \}", text)
    for name in ("Tsm", "tsm_plan"):
        assert getattr(phaze_amd, name) is getattr(capi, name) and name in phaze_amd.__all__
    for method in ("process", "process_device", "process_tuned"):
        assert hasattr(capi.Tsm, method)
    import inspect
    sig = inspect.signature(capi.Tsm.process_tuned).parameters
    assert sig["rate"].default == 1.0 and sig["epochs"].default is False


def test_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    x = (C.c_float * 8)()
    g = (C.c_int32 * 4)(4, 0, 0, 2)
    bad = capi.PV_ERR_ARGUMENT
    assert L.pv_tsm_destroy(None) == bad and L.pv_tsm_synchronize(None) == bad and L.pv_tsm_set_stream(None, None) == bad
    assert L.pv_tsm_process(None, x, 8, 8, 1, g, 1, x, 0, 8, 8) == bad
    assert L.pv_tsm_process_device(None, None, 8, 8, 1, g, 1, None, 0, 8, 8) == bad
    assert L.pv_tsm_create(None, None) == bad
    assert list(x) == [0.0] * 8


def test_config_errors_and_oversized_configs_appear_without_a_device():
    """The span, P and Hn must fit the 160 KiB of LDS of a compute unit: max_period 4096 goes with max_rate 1 only.  The limit is the model's."""
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    h = C.c_void_p()

    def create(cfg):
        rc = L.pv_tsm_create(C.byref(cfg), C.byref(h))
        return rc, L.pv_tsm_last_error(None).decode()

    for (mp, rate), word in [((1, 1), "max_period"), ((0, 1), "max_period"), ((4097, 1), "max_period"), ((-3, 1), "max_period"), ((512, 0), "max_rate"),
                             ((512, 5), "max_rate"), ((512, -1), "max_rate")]:
        rc, msg = create(capi.make_tsm_config(mp, rate))
        assert rc == capi.PV_ERR_ARGUMENT and word in msg, (mp, rate, msg)
    cfg = capi.make_tsm_config(512, 2)
    cfg.struct_size -= 4
    rc, msg = create(cfg)
    assert rc == capi.PV_ERR_ARGUMENT and "struct_size" in msg
    rc, msg = create(capi.make_tsm_config(512, 2, flags=1))
    assert rc == capi.PV_ERR_ARGUMENT and "flags" in msg
    rc, msg = create(capi.make_tsm_config(512, 2, max_channels=-1))
    assert rc == capi.PV_ERR_ARGUMENT and "max_channels" in msg
    assert create(capi.make_tsm_config(512, 2, max_channels=65536))[0] == capi.PV_ERR_ARGUMENT
    rc, msg = create(capi.make_tsm_config(512, 2, max_outputs=-1))
    assert rc == capi.PV_ERR_ARGUMENT and "max_outputs" in msg
    fits = {(mp, rate): TM.lds_bytes(mp, rate) <= TM.LDS_BYTES for mp in (2, 64, 1024, 2048, 2300, 2400, 3000, 4096) for rate in (1, 2, 3, 4)}
    assert fits[(4096, 1)] and not fits[(4096, 2)] and not fits[(4096, 4)] and fits[(1024, 4)] and fits[(2048, 4)] and not fits[(3000, 4)]
    assert 100000 < TM.lds_bytes(1024, 4) < 110000 and 138000 < TM.lds_bytes(4096, 1) < 145000                  # about 105 KB and 141 KB
    for (mp, rate), ok in fits.items():
        rc, msg = create(capi.make_tsm_config(mp, rate))
        if not ok:
            assert rc == capi.PV_ERR_UNSUPPORTED and "LDS" in msg and str(TM.lds_bytes(mp, rate)) in msg, (mp, rate, msg)
        elif not _has_gpu():
            assert rc == capi.PV_ERR_DEVICE and "HIP device" in msg, (mp, rate, msg)              # gets as far as the device and fails loudly: no CPU fallback
        else:
            assert rc == capi.PV_OK and L.pv_tsm_destroy(h) == capi.PV_OK
    with pytest.raises(phaze_amd.PvError) as e:
        phaze_amd.Tsm(4096, 4)
    assert e.value.status == capi.PV_ERR_UNSUPPORTED
    with pytest.raises(phaze_amd.PvError):
        phaze_amd.Tsm(1)
    if not _has_gpu():
        with pytest.raises(phaze_amd.PvError):
            phaze_amd.Tsm(512)


# ---- pure host code: the planner ----------------------------------------------------------------------------------------------------------------

def test_plan_equals_the_model_exactly():
    """The tracks of tests/test_epoch_abi.py, each at rate 1 (NULL), and at random rates per record within [1/2, 2] and within [1/8, 8] (held within [1/4, 4]),
    with and without epoch records."""
    import phaze_amd
    rng = np.random.default_rng(29)
    total = far = 0
    for recs, ratios, kw, ep in TEA._cases():
        nrec = np.asarray(recs).reshape(-1, 4).shape[0]
        base = phaze_amd.epoch_plan(recs, ratios=ratios, epochs=ep, **kw)
        got, n = phaze_amd.tsm_plan(recs, ratios=ratios, epochs=ep, **kw)
        assert np.array_equal(got, TM.from_psola(base)) and n == kw["input_len"], kw                                 # rates NULL: pv_epoch_plan's bits
        for R, extra in ((2, dict()), (8, dict(lock=1.0)), (4, dict(lock=0.5, min_strength=6000))):
            rates = np.exp(rng.uniform(-np.log(R), np.log(R), nrec))
            for epochs in (None, ep):
                want, want_len = TM.tsm_plan(recs, ratios=ratios, rates=rates, epochs=epochs, **kw, **extra)
                got, got_len = phaze_amd.tsm_plan(recs, ratios=ratios, rates=rates, epochs=epochs, **kw, **extra)
                assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want) and got_len == want_len, (kw, R, extra)
                assert TM.check_grains(got, kw["max_period"]) is None
                total += got.shape[0]
                far += int(not TM.is_near(got, kw["max_period"]))
    assert total > 50000 and far > 50


def test_plan_sizes_in_two_calls_and_writes_no_more_than_the_capacity():
    from phaze_amd import capi
    L = _lib()
    recs = np.ascontiguousarray(FM.plan_records(452.0))
    nrec = recs.shape[0]
    ratios = PM.tune_ratios(recs, FM.SAMPLE_RATE)
    rates = np.full(nrec, 0.5)
    ep = np.ascontiguousarray(TEM.random_epochs(np.random.default_rng(5), nrec))
    want, want_len = TM.tsm_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, ratios=ratios, rates=rates, epochs=ep)
    p = capi.make_psola_params(256, 1024, FM.PLAN_LEN, 256.0, 32, 1024)
    e = capi.make_epoch_params()
    rp, qp, sp, ep_ = recs.ctypes.data_as(IP), ratios.ctypes.data_as(DP), rates.ctypes.data_as(DP), ep.ctypes.data_as(IP)
    n_out = C.c_int64(-7)
    n = L.pv_tsm_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, ep_, None, 0, C.byref(n_out))
    assert n == want.shape[0] > 100 and n_out.value == want_len and abs(want_len - 2 * FM.PLAN_LEN) <= 2 * 1024
    g = np.full((n + 4, 4), -7, np.int32)
    assert L.pv_tsm_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, ep_, g.ctypes.data_as(IP), n - 5, None) == n          # output_len may be NULL
    assert np.array_equal(g[:n - 5], want[:n - 5]) and np.all(g[n - 5:] == -7)
    assert L.pv_tsm_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, ep_, g.ctypes.data_as(IP), n + 4, C.byref(n_out)) == n
    assert np.array_equal(g[:n], want) and np.all(g[n:] == -7) and n_out.value == want_len


def test_plan_rejects_every_bad_argument():
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    recs = np.ascontiguousarray(FM.plan_records(452.0))
    nrec = recs.shape[0]
    rp = recs.ctypes.data_as(IP)
    g = np.zeros((2048, 4), np.int32)
    gp = g.ctypes.data_as(IP)
    ones = np.ones(nrec)
    ep = np.ascontiguousarray(TEM.random_epochs(np.random.default_rng(6), nrec))
    bad = -capi.PV_ERR_ARGUMENT
    n_out = C.c_int64(-7)

    def plan(records=rp, n=nrec, ratios=None, rates=None, epochs=ep, out=gp, capacity=2048, struct_delta=0, reserved=0, e_delta=0, min_strength=0, lock=0.125,
             no_e=False, **kw):
        args = dict(f0_hop=256, f0_center=1024, input_len=FM.PLAN_LEN, unvoiced_period=256.0, min_period=32, max_period=1024)
        args.update(kw)
        p = capi.make_psola_params(**args)
        p.struct_size += struct_delta
        p.reserved = reserved
        e = capi.make_epoch_params(min_strength, lock)
        e.struct_size += e_delta
        return L.pv_tsm_plan(C.byref(p), None if no_e else C.byref(e), records, n, None if ratios is None else ratios.ctypes.data_as(DP),
                             None if rates is None else rates.ctypes.data_as(DP), None if epochs is None else epochs.ctypes.data_as(IP), out, capacity, C.byref(n_out))

    assert plan() == EM.epoch_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, epochs=ep).shape[0] and n_out.value == FM.PLAN_LEN
    assert L.pv_tsm_plan(None, C.byref(capi.make_epoch_params()), rp, nrec, None, None, None, gp, 2048, None) == bad
    g[:] = 0
    n_out.value = -7
    two = ones.copy()
    two[7] = 2.0000001
    nan = ones.copy()
    nan[0] = np.nan
    zero = ones.copy()
    zero[3] = 0.0
    inf = ones.copy()
    inf[nrec - 1] = np.inf
    for kw in (dict(struct_delta=8), dict(struct_delta=-8), dict(reserved=1), dict(records=None), dict(n=-1), dict(out=None), dict(capacity=-1), dict(f0_hop=0),
               dict(min_period=1), dict(min_period=0), dict(max_period=4097), dict(min_period=600, max_period=500, unvoiced_period=550.0), dict(unvoiced_period=31.9),
               dict(unvoiced_period=1024.5), dict(unvoiced_period=float("nan")), dict(input_len=-1), dict(input_len=1 << 30), dict(ratios=two), dict(ratios=nan),
               dict(ratios=ones * 0.49), dict(ratios=-ones), dict(rates=nan), dict(rates=zero), dict(rates=-ones), dict(rates=inf), dict(no_e=True), dict(e_delta=8),
               dict(e_delta=-8), dict(min_strength=-1), dict(min_strength=16385), dict(lock=0.0), dict(lock=-0.5), dict(lock=1.0000001), dict(lock=float("nan")),
               dict(lock=float("inf"))):
        assert plan(**kw) == bad, kw
    assert not g.any() and n_out.value == -7                                # nothing written by a refused call
    # an output that would pass 2^30 cannot be written down: refused, whatever the capacity
    assert plan(input_len=(1 << 30) - 1, rates=ones * 0.25, epochs=None, out=None, capacity=0, max_period=4096, unvoiced_period=4096.0, min_period=2048) == bad
    assert plan(records=None, n=0, epochs=None) == PM.psola_plan(np.zeros((0, 4), np.int32), 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024).shape[0]
    assert plan(out=None, capacity=0) == plan()
    assert plan(rates=ones) == plan() and plan(rates=ones * 1000.0) == plan(rates=ones * 4.0) and plan(rates=ones * 1e-9) == plan(rates=ones * 0.25)
    assert plan(rates=ones * 0.5) > plan() > plan(rates=ones * 2.0) > 0
    with pytest.raises(ValueError):
        phaze_amd.tsm_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, rates=ones[:-1])
    with pytest.raises(ValueError):
        phaze_amd.tsm_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, rates=zero)
    with pytest.raises(ValueError):
        phaze_amd.tsm_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, epochs=ep[:-1])
    with pytest.raises(ValueError):
        phaze_amd.tsm_plan(recs, 256, 1024, FM.PLAN_LEN, 256.0, 32, 1024, lock=0.0)


# ---- kernel resources -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_tsm_kernel_uses_no_spill_no_scratch_no_agprs():
    """One kernel, pv_tsm_kernel: DESIGN.md "Time-scale modification" quotes its figures (no static LDS beside the dynamic arrays)."""
    kernels = RU.resources("psola/pv_tsm_kernels.hip")
    assert len(kernels) == 1 and all("pv_tsm_kernel" in n for n in kernels), sorted(kernels)
    for n, v in kernels.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs"] <= 64 and v["LDS Size"] == 0, (n, v)


def test_the_existing_overlap_add_kernels_are_untouched():
    """pv_psola_kernels.hip and pv_epoch_kernels.hip have pinned resource figures: the new kernel restates their arithmetic in its own file and includes neither
    (nor their contract headers)."""
    src = open(os.path.join(ROOT, "phaze_amd", "csrc", "psola", "pv_tsm_kernels.hip")).read()
    assert '#include "pv_tsm.h"' in src and "pv_psola.h" not in re.findall(r'#include "([^"]+)"', src) and "pv_psola_kernel<" not in src
    assert "pv_tsm_kernels.hip" in open(os.path.join(ROOT, "phaze_amd", "csrc", "Makefile")).read().split("stretch-resource-usage:")[1]


# ---- the example ------------------------------------------------------------------------------------------------------------------------------

def build_example(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_tsm")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_tsm.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_tsm_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_example(tmp_path)
    if not _has_gpu():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device error" in r.stderr                    # no CPU fallback behind the C ABI
