"""CPU checks of the per-take surface: the header declares, the library exports and the ctypes binding gives argument types to every pv_takes_* name, the
ABI stays 6, bad and oversized configs are refused before any device is touched, pv_takes_tiles (the host's tile walk, pure host code) equals the Python
model (tests/takes_model.py) with == on ragged calls, sizes in two calls and refuses every bad call with its status and a message that names take and
grain, the kernel file compiles for gfx950 without spills, scratch or AGPRs, and examples/pv_takes.c builds as pedantic C99 (tests/test_gpu_takes.py
runs it, and holds the refusals that need a handle: channels, buffers, strides and overlapping outputs)."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resource_usage as RU
import takes_model as KM
import test_gpu_tsm as TGT
import test_psola_abi as TPA
import test_takes_model as TKM
import tsm_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "phaze_amd.h")
SURFACE = {"pv_takes_create": 2, "pv_takes_destroy": 1, "pv_takes_last_error": 1, "pv_takes_set_stream": 2, "pv_takes_synchronize": 1, "pv_takes_process": 4,
           "pv_takes_process_device": 4, "pv_takes_tiles": 5}
IP = C.POINTER(C.c_int32)
TILE = KM.TILE
NOUT = TGT.NOUT

_lib = TPA._lib
_has_gpu = TPA._has_gpu
_declaration = TPA._declaration


def test_header_declares_library_exports_and_binding_types_the_surface():
    import phaze_amd
    from phaze_amd import capi
    text = open(HEADER).read()
    declared = set(re.findall(r"PV_API\s+[\w ]+?\*?\s*\b(pv_takes_\w+)\s*\(", text))
    assert declared == set(SURFACE)
    assert set(SURFACE) <= set(capi.EXPORTS)
    L = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "phaze_amd", "lib", "libphaze_amd.so")], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pv_\w+)", out))
    assert set(SURFACE) <= exported and {n for n in exported if n.startswith("pv_takes_")} == set(SURFACE)
    assert exported == set(capi.EXPORTS)                                    # new symbols only, every one of them pv_takes_*
    vp = C.c_void_p
    types = {"pv_takes *": vp, "const pv_takes *": vp, "pv_takes **": C.POINTER(vp), "const pv_takes_config *": C.POINTER(capi._TakesConfig),
             "const pv_take *": C.POINTER(capi._Take), "void *": vp, "int32_t": C.c_int32, "int64_t": C.c_int64, "int32_t *": IP}
    for name, nargs in SURFACE.items():
        ret, decl = _declaration(name)
        got = getattr(L, name).argtypes
        assert len(got) == len(decl) == nargs, (name, decl)
        for i, (d, g) in enumerate(zip(decl, got)):
            assert g == types[d], (name, i, d, g)
        assert getattr(L, name).restype == {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p}[ret], (name, ret)
    assert L.pv_abi_version() == capi.ABI_VERSION == 6 == int(re.search(r"#define PV_ABI_VERSION (\d+)", text).group(1))
    note = text[text.index("#define PV_ABI_VERSION") - 2000:text.index("#define PV_ABI_VERSION")]
    assert "pv_takes_" in note and "pv_harmony_" in note and "6 = the time-stretch handle" in note                     # recorded on the line for 6
    assert C.sizeof(capi._TakesConfig) == 28 and C.sizeof(capi._Take) == 72
    body = re.search(r"typedef struct pv_takes_config \{(.*?)\} pv_takes_config;", text, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+);", body, re.M)
    assert [(n, C.c_int32) for t, n in fields] == list(capi._TakesConfig._fields_) and all(t == "int32_t" for t, _ in fields)
    assert [n for _, n in fields] == ["struct_size", "max_period", "max_rate", "max_channels", "max_outputs", "device_id", "flags"]      # pv_tsm_config's
    assert re.search(r"#define PV_TAKES_CONFIG_INIT \{ \(int32_t\)sizeof\(pv_takes_config\), 0, 0, 0, 0, 0, 0 \}", text)
    body = re.search(r"typedef struct pv_take \{(.*?)\} pv_take;", text, re.S).group(1)
    members = [n.strip() for line in re.findall(r"^\s*(?:const\s+)?(?:float|int32_t|int64_t)\s*\*?\s*([\w, ]+);", body, re.M) for n in line.split(",")]
    assert members == ["in", "nin", "in_stride", "grains", "ngrains", "out", "out_first", "nout", "out_stride"]
    assert [n.rstrip("_") for n, _ in capi._Take._fields_] == members and all(C.sizeof(t) == 8 for _, t in capi._Take._fields_)
    for name in ("Takes", "takes_tiles"):
        assert getattr(phaze_amd, name) is getattr(capi, name) and name in phaze_amd.__all__
    for method in ("process", "process_device", "process_tuned"):
        assert hasattr(capi.Takes, method)
    sig = inspect.signature(capi.Takes.process_tuned).parameters
    assert sig["rate"].default == 1.0 and sig["epochs"].default is False and sig["threshold"].default == 2458 and sig["a4"].default == 440.0
    sig = inspect.signature(capi.Takes.__init__).parameters
    assert list(sig)[1:] == ["max_period", "max_rate", "max_channels", "max_outputs", "device_id"] and sig["max_rate"].default == 2
    assert list(inspect.signature(capi.takes_tiles).parameters) == ["max_period", "max_rate", "tables", "out_firsts", "nouts"]


def test_calls_without_a_handle_are_rejected():
    from phaze_amd import capi
    L = _lib()
    x = (C.c_float * 8)()
    g = (C.c_int32 * 4)(4, 0, 0, 2)
    take = (capi._Take * 1)(capi._Take(C.addressof(x), 8, 8, g, 1, C.addressof(x), 0, 8, 8))
    bad = capi.PV_ERR_ARGUMENT
    assert L.pv_takes_destroy(None) == bad and L.pv_takes_synchronize(None) == bad and L.pv_takes_set_stream(None, None) == bad
    assert L.pv_takes_process(None, take, 1, 1) == bad
    assert L.pv_takes_process_device(None, take, 1, 1) == bad
    assert L.pv_takes_create(None, None) == bad
    assert list(x) == [0.0] * 8


def test_config_errors_and_oversized_configs_appear_without_a_device():
    """The fields mean what pv_tsm_config's mean: the same values are refused, and the same pairs with PV_ERR_UNSUPPORTED, before any device is touched; and
    pv_takes_tiles validates its config the same way."""
    import phaze_amd
    from phaze_amd import capi
    L = _lib()
    h = C.c_void_p()

    def create(cfg):
        rc = L.pv_takes_create(C.byref(cfg), C.byref(h))
        return rc, L.pv_takes_last_error(None).decode()

    def tiles(cfg):
        rc = L.pv_takes_tiles(C.byref(cfg), None, 0, None, 0)
        return -rc, L.pv_takes_last_error(None).decode()

    for (mp, rate), word in [((1, 1), "max_period"), ((0, 1), "max_period"), ((4097, 1), "max_period"), ((-3, 1), "max_period"), ((512, 0), "max_rate"),
                             ((512, 5), "max_rate"), ((512, -1), "max_rate")]:
        for fn in (create, tiles):
            rc, msg = fn(capi.make_takes_config(mp, rate))
            assert rc == capi.PV_ERR_ARGUMENT and word in msg, (mp, rate, msg)
    for fn in (create, tiles):
        cfg = capi.make_takes_config(512, 2)
        cfg.struct_size -= 4
        rc, msg = fn(cfg)
        assert rc == capi.PV_ERR_ARGUMENT and "struct_size" in msg
        rc, msg = fn(capi.make_takes_config(512, 2, flags=1))
        assert rc == capi.PV_ERR_ARGUMENT and "flags" in msg
        rc, msg = fn(capi.make_takes_config(512, 2, max_channels=-1))
        assert rc == capi.PV_ERR_ARGUMENT and "max_channels" in msg
        assert fn(capi.make_takes_config(512, 2, max_channels=65536))[0] == capi.PV_ERR_ARGUMENT
        rc, msg = fn(capi.make_takes_config(512, 2, max_outputs=-1))
        assert rc == capi.PV_ERR_ARGUMENT and "max_outputs" in msg
    fits = {(mp, rate): TM.lds_bytes(mp, rate) <= TM.LDS_BYTES for mp in (2, 64, 1024, 2048, 2300, 2400, 3000, 4096) for rate in (1, 2, 3, 4)}
    assert fits[(4096, 1)] and not fits[(4096, 2)] and fits[(2048, 4)] and not fits[(3000, 4)]
    for (mp, rate), ok in fits.items():
        rc, msg = create(capi.make_takes_config(mp, rate))
        if not ok:
            assert rc == capi.PV_ERR_UNSUPPORTED and "LDS" in msg and str(TM.lds_bytes(mp, rate)) in msg, (mp, rate, msg)
            assert tiles(capi.make_takes_config(mp, rate))[0] == capi.PV_ERR_UNSUPPORTED
        elif not _has_gpu():
            assert rc == capi.PV_ERR_DEVICE and "HIP device" in msg, (mp, rate, msg)              # gets as far as the device and fails loudly: no CPU fallback
            assert tiles(capi.make_takes_config(mp, rate))[0] == capi.PV_OK
        else:
            assert rc == capi.PV_OK and L.pv_takes_destroy(h) == capi.PV_OK
    assert L.pv_takes_tiles(None, None, 0, None, 0) == -capi.PV_ERR_ARGUMENT
    with pytest.raises(phaze_amd.PvError) as e:
        phaze_amd.Takes(4096, 4)
    assert e.value.status == capi.PV_ERR_UNSUPPORTED
    with pytest.raises(phaze_amd.PvError):
        phaze_amd.Takes(1)
    if not _has_gpu():
        with pytest.raises(phaze_amd.PvError):
            phaze_amd.Takes(512)


# ---- pure host code: the tile walk -----------------------------------------------------------------------------------------------------------------

def ragged_call():
    """The six ragged takes of tests/test_gpu_takes.py on a (512, 4) configuration: (tables, nouts)."""
    return [TGT._grains(name)[3] for name in ("small", "tiny", "gap", "empty", "slow", "fast")], list(TKM.RAGGED_NOUTS)


def test_tiles_equal_the_model_exactly_on_ragged_calls():
    import phaze_amd
    checked = classes = 0
    seen = set()
    tables, nouts = ragged_call()
    for first in (0, 517, (1 << 20) + 17):
        for shift in range(6):                                               # every table meets every length
            tb = tables[shift:] + tables[:shift]
            firsts = [first] * 6
            assert KM.check_span(tb, 512, 4, firsts, nouts) is None
            want = KM.tiles(tb, 512, firsts, nouts)
            got = phaze_amd.takes_tiles(512, 4, tb, firsts, nouts)
            assert got.dtype == np.int32 and got.shape == want.shape == (9, 8) and np.array_equal(got, want), (first, shift)
            checked += got.shape[0]
            seen |= set(got[:, 6].tolist())
    # every table of tests/test_gpu_tsm.py on its own configuration, six ragged takes of it, each take from its own first output
    for name in TGT.CASES:
        mp, R, nin, g = TGT._grains(name)
        for firsts in ([0] * 6, [0, 517, 1024, 2048, 1, 3000], [(1 << 20) + 17] * 6):
            if KM.check_span([g] * 6, mp, R, firsts, nouts) is not None:
                with pytest.raises(phaze_amd.PvError):
                    phaze_amd.takes_tiles(mp, R, [g] * 6, firsts, nouts)
                continue
            want = KM.tiles([g] * 6, mp, firsts, nouts)
            got = phaze_amd.takes_tiles(mp, R, [g] * 6, firsts, nouts)
            assert np.array_equal(got, want), (name, firsts)
            checked += got.shape[0]
            seen |= set(got[:, 6].tolist())
    mp, R, nins, tables, firsts, nouts = TKM.class_fixture()
    want = KM.tiles(tables, mp, firsts, nouts)
    got = phaze_amd.takes_tiles(mp, R, tables, firsts, nouts)
    assert np.array_equal(got, want) and set(got[:, 6].tolist()) == {1, 2, 3, 4}
    assert checked > 300 and seen == {1, 2, 3, 4}
    assert phaze_amd.takes_tiles(512, 4, [], [], []).shape == (0, 8)
    assert phaze_amd.takes_tiles(512, 4, [tables[3]], [0], [0]).shape == (0, 8)


def test_tiles_equal_the_model_at_the_largest_accepted_spans():
    """The pairs with the largest spans, (4096, 1), (3641, 2), (2811, 3) and (2257, 4): their spans are no multiples of 64, and the widest tiles they accept
    read more samples than the last multiple of 64 that fits the LDS.  Every such tile has class 1, in the library as in the model; one sample more is
    refused."""
    import phaze_amd
    from phaze_amd import capi
    top, pairs = TKM.largest_spans()
    _, _, _, small = TGT._grains("small")
    for mp, R in pairs:
        for slack in (0, 1, 4, 12, 63, 64, 70):
            g, cap = TKM.widest_tile_table(mp, R, slack)
            tables, firsts, nouts = [small, g, g], [0, 0, 517], [NOUT, 1024, 400]
            want = KM.tiles(tables, mp, firsts, nouts)
            got = phaze_amd.takes_tiles(mp, R, tables, firsts, nouts)
            assert np.array_equal(got, want) and got[4].tolist() == [1, 0, 0, 2, 65, cap, 1, 0], (mp, R, slack)
            assert np.all((got[:, 6] >= 1) & (got[:, 6] <= 4))
        g, cap = TKM.widest_tile_table(mp, R, -1)
        with pytest.raises(phaze_amd.PvError) as e:
            phaze_amd.takes_tiles(mp, R, [small, g], [0, 0], [NOUT, 1024])
        assert e.value.status == capi.PV_ERR_ARGUMENT and "take 1: grain 0:" in str(e.value) and str(cap) in str(e.value)


def _takes(entries):
    """A pv_take array of (grains or None, ngrains or None, out_first, nout[, nin]) with null buffers."""
    from phaze_amd import capi
    arr = (capi._Take * max(len(entries), 1))()
    keep = []
    for k, e in enumerate(entries):
        g, ng, first, nout = e[:4]
        if g is not None:
            g = np.ascontiguousarray(g, np.int32)
            keep.append(g)
        arr[k] = capi._Take(None, e[4] if len(e) > 4 else 0, 0, g.ctypes.data_as(IP) if g is not None and g.size else None, (g.shape[0] if g is not None else 0) if ng is None else ng,
                            None, first, nout, 0)
    return arr, keep


def test_tiles_size_in_two_calls_and_write_no_more_than_the_capacity():
    from phaze_amd import capi
    L = _lib()
    mp, R, nins, tables, firsts, nouts = TKM.class_fixture()
    want = KM.tiles(tables, mp, firsts, nouts).astype(np.int32)
    arr, keep = _takes([(g, None, f, n) for g, f, n in zip(tables, firsts, nouts)])
    cfg = capi.make_takes_config(mp, R)
    assert L.pv_takes_tiles(C.byref(cfg), arr, 4, None, 0) == 13
    for cap in (0, 5, 13, 20):
        out = np.full((cap + 3, 8), -7, np.int32)
        assert L.pv_takes_tiles(C.byref(cfg), arr, 4, out.ctypes.data_as(IP), cap) == 13
        m = min(cap, 13)
        assert np.array_equal(out[:m], want[:m]) and np.all(out[m:] == -7)


def test_tiles_refuse_every_bad_call_and_name_take_and_grain():
    from phaze_amd import capi
    L = _lib()
    tables, nouts = ragged_call()
    bad = capi.PV_ERR_ARGUMENT
    out = np.full((64, 8), -7, np.int32)

    def tiles(entries, ntakes=None, mp=512, R=4, null=False, capacity=64, buf=True):
        arr, keep = _takes(entries)
        cfg = capi.make_takes_config(mp, R)
        rc = L.pv_takes_tiles(C.byref(cfg), None if null else arr, len(entries) if ntakes is None else ntakes, out.ctypes.data_as(IP) if buf else None, capacity)
        return rc, L.pv_takes_last_error(None).decode()

    good = [(g, None, 0, n) for g, n in zip(tables, nouts)]
    assert tiles(good)[0] == 9
    out[:] = -7
    # everything pv_tsm_process rejects in a table, in the first, a middle and the last take: the grain is counted within its take
    small = tables[0]
    last = small.shape[0] - 1
    for k in (0, 2, 5):
        for idx, col, val in [(7, 3, 1), (7, 3, 513), (0, 0, -1), (5, 0, 1 << 30), (9, 1, 65536), (9, 1, -1), (11, 2, 1 << 30), (11, 2, -(1 << 30)), (last, 0, 5),
                              (20, 0, int(small[19, 0]) - 1)]:
            g = np.array(small)
            g[idx, col] = val
            assert TM.check_grains(g, 512)[0] == idx
            entries = list(good)
            entries[k] = (g, None, 0, nouts[k])
            rc, msg = tiles(entries)
            assert rc == -bad and f"take {k}: grain {idx}:" in msg, (k, idx, msg)
    swapped = np.array(small)
    swapped[[30, 31]] = swapped[[31, 30]]
    rc, msg = tiles(good[:5] + [(swapped, None, 0, 5)])
    assert rc == -bad and "take 5: grain 31:" in msg and "out of order" in msg
    # a half length the table's own configuration allows and this one does not
    rc, msg = tiles(good, mp=32)
    assert rc == -bad and "take 0: grain" in msg and "max_period 32" in msg
    # a well-formed table with a tile beyond the span, in the third of four takes: the message names the take and the tile's first grain
    for idx, val in ((60, 100000), (100, (1 << 30) - 1), (3, -((1 << 30) - 1))):
        wide = np.array(small)
        wide[idx, 2] = val
        assert TM.check_grains(wide, 512) is None
        tb = [tables[1], tables[2], wide, tables[4]]
        k, tile, first, extent = KM.check_span(tb, 512, 4, [0] * 4, [NOUT] * 4)
        assert k == 2 and extent > TM.span(512, 4) and tile == int(small[idx, 0]) // TILE
        rc, msg = tiles([(g, None, 0, NOUT) for g in tb])
        assert rc == -bad and f"take 2: grain {first}:" in msg and "span" in msg and str(extent) in msg and str(TM.span(512, 4)) in msg, msg
        if tile > 0:                                                         # the tiles before it are fine
            assert tiles([(g, None, 0, tile * TILE - 200) for g in tb])[0] == 4 * tile
    out[:] = -7                                                              # (a span refusal comes from the walk: the records before it may be written)
    # the counts and the ranges
    for entries, word in [([(small, -1, 0, 8)], "take 0"), ([good[0], (small, None, -1, 8)], "take 1"), ([good[0], good[1], (small, None, 0, -8)], "take 2"),
                          ([(small, None, 0, 8, -1)], "take 0"), ([(small, None, (1 << 30) - 5, 8)], "2^30"), ([(small, None, 0, (1 << 30) + 1)], "2^30"),
                          ([(small, None, 0, 8, (1 << 30) + 1)], "2^30"), ([good[0], (None, 3, 0, 8)], "take 1: null grains"),
                          ([(small, (1 << 27) + 1, 0, 8)], "2^27"),
                          ([(None, 0, 0, 1 << 29), (None, 0, 0, 1 << 29)], "take 1: the takes' outputs together reach 2^30"),
                          ([(small[:1], (1 << 26) + 1, 0, 8)] * 2, "take 1: more than 2^27 grains in one call")]:      # refused on the counts, before any table is read
        rc, msg = tiles(entries)
        assert rc == -bad and word in msg, (word, msg)
    assert tiles([(None, 0, 0, 1 << 29), (None, 0, 0, (1 << 29) - 1)], capacity=0, buf=False)[0] == 2 * (1 << 19)     # just below: 2^20 empty tiles, none written
    rc, msg = tiles(good, ntakes=-1)
    assert rc == -bad and "takes" in msg
    rc, msg = tiles(good, ntakes=65537)
    assert rc == -bad and "65536" in msg
    rc, msg = tiles(good, null=True)
    assert rc == -bad and "null takes" in msg
    assert tiles(good, capacity=-1)[0] == -bad and tiles(good, buf=False)[0] == -bad
    assert tiles([], null=True)[0] == 0 and tiles(good, ntakes=0)[0] == 0
    assert np.all(out == -7)                                                 # nothing written by a call refused on its arguments


# ---- kernel resources -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(RU.HIPCC), reason="no hipcc")
def test_takes_kernel_uses_no_spill_no_scratch_no_agprs():
    """One kernel, pv_takes_kernel, within pv_tsm_kernel's pinned ceiling of 64 VGPRs: DESIGN.md "Takes" quotes its figures (no static LDS beside the
    dynamic arrays)."""
    kernels = RU.resources("psola/pv_takes_kernels.hip")
    assert len(kernels) == 1 and all("pv_takes_kernel" in n for n in kernels), sorted(kernels)
    for n, v in kernels.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs"] <= 64 and v["LDS Size"] == 0, (n, v)


def test_the_existing_overlap_add_kernels_are_untouched():
    """pv_psola_kernels.hip, pv_epoch_kernels.hip, pv_tsm_kernels.hip and pv_harmony_kernels.hip have pinned resource figures: the new kernel restates
    pv_tsm_kernel's arithmetic in its own file, includes none of them and instantiates none of their kernels."""
    src = open(os.path.join(ROOT, "phaze_amd", "csrc", "psola", "pv_takes_kernels.hip")).read()
    includes = re.findall(r'#include "([^"]+)"', src)
    assert "pv_takes.h" in includes and not any(i.endswith(".hip") for i in includes)
    assert not {"pv_psola.h", "pv_epoch.h", "pv_harmony.h"} & set(includes)
    contract = re.findall(r'#include "([^"]+)"', open(os.path.join(ROOT, "phaze_amd", "csrc", "psola", "pv_takes.h")).read())
    assert contract == ["pv_tsm.h"]
    code = re.sub(r"//.*", "", src)
    for name in ("pv_psola_kernel", "pv_epoch_kernel", "pv_tsm_kernel", "pv_harmony_kernel", "pv_launch_tsm", "pv_launch_psola", "pv_launch_harmony", "asm"):
        assert name not in code, name
    make = open(os.path.join(ROOT, "phaze_amd", "csrc", "Makefile")).read()
    assert "pv_takes_kernels.hip" in make.split("stretch-resource-usage:")[1]
    assert all(f"psola/pv_takes_{part}" in make.split("OBJS =")[0] for part in ("kernels.hip", "capi.hip")) and "psola/pv_takes.h" in make


# ---- the example ------------------------------------------------------------------------------------------------------------------------------

def build_example(tmp_path):
    import phaze_amd
    if not os.path.exists(phaze_amd.library_path()):
        phaze_amd.build_library()
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_takes")
    cmd = ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pv_takes.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_takes_example_builds_as_pedantic_c99_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_example(tmp_path)
    if not _has_gpu():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device error" in r.stderr                    # no CPU fallback behind the C ABI
