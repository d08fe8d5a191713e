"""Hazard pads and register copies in the frame loop of the fp32-first pitchFactor >= 1 instances of pv_wave_kernel_1024 (CPU-only: hipcc cross-compiles
pv_wave_kernel.hip for gfx950, tools/isa_copies.py walks the class-A path of the loop once per rotation mode of the scatter and counts).

The compiler pads the first read of a register that an asm statement wrote, and copies where an operand class or a tied destination forces it to: with the
packed helpers as one-instruction statements that was 91 wait states and ~52 register moves per frame at hop 256 (profiles/frame_copies_parent.md, the parent's
sources through the same tool).  The fused helpers, SGPR operands and the select form of the register transpose took most of them out; the counts of
profiles/frame_copies_after.md are held as caps, so that a helper edit which brings them back does not go unnoticed."""
import functools
import os
import sys

import pytest

from resource_usage import HIPCC, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_copies as C  # noqa: E402
import lds_wait_points as W  # noqa: E402

PARENT = os.path.join(ROOT, "profiles", "frame_copies_parent.md")
AFTER = os.path.join(ROOT, "profiles", "frame_copies_after.md")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


@functools.lru_cache(maxsize=None)
def _asm():
    return W.compile_asm("pv_wave_kernel.hip")


@functools.lru_cache(maxsize=None)
def _counts(hop):
    return {m: c for m, (c, _) in C.frame_paths(_asm(), C.INSTANCES[hop]).items()}


def test_the_recorded_tables_cover_every_instance_and_mode():
    for path in (PARENT, AFTER):
        got = C.read_table(path)
        assert set(got) == {(hop, m) for hop in C.INSTANCES for m in C.MODES}, (path, sorted(got))


@pytest.mark.parametrize("hop", sorted(C.INSTANCES))
def test_the_frame_loop_stays_within_the_recorded_counts(hop):
    cap = C.read_table(AFTER)
    for m in C.MODES:
        got, want = _counts(hop)[m], cap[(hop, m)]
        print(f"hop {hop} {m}: {got} (recorded {want})")
        for field in C.FIELDS:
            assert getattr(got, field) <= getattr(want, field), (hop, m, field, got, want)


def test_hop_256_lost_fifty_pads_and_twenty_moves():
    parent = C.read_table(PARENT)
    for m in C.MODES:
        got, was = _counts(256)[m], parent[(256, m)]
        print(f"hop 256 {m}: {was} -> {got}")
        assert got.pads <= was.pads - 50, (m, got, was)
        assert got.vv + got.sv <= was.vv + was.sv - 20, (m, got, was)
