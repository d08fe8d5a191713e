"""Register budget of pv_wg16_kernel (CPU-only: hipcc cross-compiles for gfx950 and reports the resources it allocated).

The kernel runs two waves per SIMD -- two workgroups per CU at N = 8192, four at N = 4096 -- and that rests on 256 registers in all, AGPRs included.  A non-inlined
callee is compiled for the largest budget and the kernel inherits what it takes: a few AGPRs in the general residue once cost every instance its second wave (everything 1.8x
slower, the f >= 1 frames that never call it included).  This test keeps the cliff from coming back unnoticed; the resident (streaming) instances run one wave per SIMD on purpose."""
import functools
import json
import os
import re

import pytest

import resource_usage
from resource_usage import HIPCC, ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_kernel_resources_parent.json")
KERNELS = ("pv_chain_kernel", "pv_wave_kernel_1024", "pv_classify_chains", "pv_wave2k_kernel", "pv_wg_kernel", "pv_wg16_kernel")


@functools.lru_cache(maxsize=None)
def _resources(source):
    """resource_usage.resources(source), compiled once per session."""
    return resource_usage.resources(source)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_wg16_instances_keep_two_waves_per_simd():
    kernels = _resources("pv_wg16_kernel.hip")
    inst = {k: v for k, v in kernels.items() if "pv_wg16_kernel" in k}
    assert len(inst) == 24, sorted(inst)                         # 2 sizes x 4 hops x (product, tap, resident)
    for k, v in inst.items():
        log2n, rows, aux, resident = re.search(r"ILi(\d+)ELi(\d+)ELb([01])ELb([01])E", k).groups()
        if resident == "1":
            assert v["Occupancy"] == 1 and v["VGPRs Spill"] == 0, (k, v)      # the whole register file, AGPRs instead of scratch
            continue
        assert v["Occupancy"] == 2 and v["AGPRs"] == 0, (k, v)
        assert v["VGPRs"] <= 256
        if aux == "0":
            assert v["VGPRs Spill"] <= (0 if rows == "4" else 12), (k, v)   # BASELINE's shapes (hop = N/4): nothing in scratch; the other hops a handful around the residue call
        lds = 81632 if log2n == "13" else 39840
        assert (lds + 256 + 511) // 512 * 512 * (2 if log2n == "13" else 4) <= 160 * 1024


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_headline_instances_keep_three_waves_per_simd_and_their_hot_path_out_of_scratch():
    """pv_wave_kernel_1024: every batch instance runs three waves per SIMD (<= 168 VGPRs, no AGPRs).  The fp32-first instances for pitchFactor >= 1 chains (the
    headline launch) carry their rare forward transforms out of line: inlined, the register allocator parked values of the HOT path in scratch memory (round 5:
    62 spilled VGPRs, ~18 scratch accesses per frame).  A handful of loop invariants of the inline fp64-first path may live there; more means the hot path is hit again."""
    kernels = _resources("pv_wave_kernel.hip")
    inst = {k: v for k, v in kernels.items() if "pv_wave_kernel_1024" in k}
    assert len(inst) == 28, sorted(inst)                         # 4 hops x (2 classes x 2 forward forms + tap + 2 resident)
    for k, v in inst.items():
        rows, aux, resident, spread, f32 = re.search(r"ILi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])E", k).groups()
        if resident == "1":
            continue
        assert v["Occupancy"] == 3 and v["AGPRs"] == 0 and v["VGPRs"] <= 168, (k, v)
        if spread == "1" and f32 == "0":
            assert v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0, (k, v)
        if spread == "1" and f32 == "1":
            assert v["VGPRs Spill"] <= 8, (k, v)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_wg_instances_and_the_lds_ring_keep_their_registers():
    """pv_wg_kernel: N = 2048 / 4096 / 8192 (G = 2 / 4 / 8 waves), S_ROWS = 8 hop / N for hop >= N/8 and S_ROWS = 0 for the LDS overlap-add ring that
    runs every smaller hop (R up to N / 2, run-time R).  The ring instances (product and tap) hold a frame in 229..246 VGPRs: two waves per SIMD, no
    AGPRs, nothing spilled.  The resident instances (N = 8192, hop >= N/8) are not bound by this."""
    kernels = _resources("pv_wg_kernel.hip")
    inst = {k: v for k, v in kernels.items() if "pv_wg_kernel" in k}
    assert len(inst) == 34, sorted(inst)                         # 3 sizes x 5 row counts (0, 1, 2, 4, 8) x (product, tap) + 4 resident at N = 8192
    ring = 0
    for k, v in inst.items():
        log2n, rows, aux, resident = re.search(r"ILi(\d+)ELi(\d+)ELb([01])ELb([01])E", k).groups()
        assert v["LDS Size"] == 256, (k, v)                     # static LDS: what the dispatch tests add to the dynamic size
        if resident == "1":
            assert log2n == "13" and rows != "0", k
            continue
        assert v["Occupancy"] == 2 and v["AGPRs"] == 0 and v["VGPRs"] <= 256, (k, v)
        if rows == "0":
            ring += 1
            assert v["VGPRs Spill"] == 0, (k, v)
    assert ring == 6                                             # 3 sizes x (product, tap)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("source", ["pv_kernels.hip", "pv_wave_kernel.hip", "pv_wave2k_kernel.hip", "pv_wg_kernel.hip", "pv_wg16_kernel.hip"])
def test_frame_kernel_instances_keep_recorded_resources(source):
    """tests/golden/frame_kernel_resources_parent.json holds resource_usage.resources() of every __global__ instance of the frame kernel files.  The set of
    instances is the recorded one; every instance has the recorded occupancy, LDS size and AGPR count, and no more scratch and no more spilled VGPRs.
    VGPR and SGPR counts are not pinned: they move with every kernel edit.  (A non-inlined callee shows in its callers: DESIGN.md section 3.)"""
    with open(GOLDEN) as f:
        want = json.load(f)[source]
    got = {k: v for k, v in _resources(source).items() if any(re.search(r"\d" + name + r"(I|E|$)", k) for name in KERNELS)}
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        assert (g["Occupancy"], g["LDS Size"], g["AGPRs"]) == (w["Occupancy"], w["LDS Size"], w["AGPRs"]), (k, g, w)
        assert g["ScratchSize"] <= w["ScratchSize"] and g["VGPRs Spill"] <= w["VGPRs Spill"], (k, g, w)
