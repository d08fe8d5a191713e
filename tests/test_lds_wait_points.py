"""Where the N = 1024 f >= 1 frame waits for LDS (CPU-only: hipcc cross-compiles pv_wave_kernel.hip for gfx950, tools/lds_wait_points.py reads the assembly).

Three groups of reads are issued ahead of the work that hides them, and that has to hold in the ISA, not only in the source -- the scheduler, short of
registers, likes to put a read next to its use.  For the four fp32-first instances of the pitchFactor >= 1 class (hop 128 / 256 / 512 / 1024):

* scatter: the nine routes of a lane are read in one batch in front of every Y store of every rotation mode, and one wait covers them (before: five
  dependent LDS round trips, a pair of reads behind each pair of stores);
* the 0.5 * Hann rows of the overlap-add and the twiddles of passes 1 and 2 of both packed transforms: at least 20 VALU instructions between the issue of
  a read and the wait that retires it, and between the read and the first instruction that names its registers (before: 0..15).

The scatter phase is the code between the frame loop's two `s_setprio 3` (PH_SCATTER, PH_C2R).  The batch and its wait must be one straight line at its head
that no branch of the phase jumps back into, with every Y store behind it in the text: then every path through the three rotation modes runs the batch once, first."""
import functools
import os
import re
import sys

import pytest

from resource_usage import HIPCC, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import lds_wait_points as W  # noqa: E402

INSTANCES = {128: "pv_wave_kernel_1024ILi1ELb0ELb0ELb1ELb1E", 256: "pv_wave_kernel_1024ILi2ELb0ELb0ELb1ELb1E",
             512: "pv_wave_kernel_1024ILi4ELb0ELb0ELb1ELb1E", 1024: "pv_wave_kernel_1024ILi8ELb0ELb0ELb1ELb1E"}
MIN_VALU = 20

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


@functools.lru_cache(maxsize=None)
def _asm():
    return W.compile_asm("pv_wave_kernel.hip")


@functools.lru_cache(maxsize=None)
def _listing(hop):
    return W.listing(_asm(), INSTANCES[hop])


def _scatter_phase(ins, segments):
    """(first, last) index into ins: from the s_setprio of PH_SCATTER up to the s_setprio of PH_C2R, the only two marks of level 3 of the table."""
    first, last = segments[0]["first"], segments[-1]["last"]
    marks = [k for k in range(first, last + 1) if ins[k].op == "s_setprio" and ins[k].text.split()[1] == "3"]
    assert len(marks) == 2, [ins[k].line for k in marks]
    return marks[0], marks[1]


@pytest.mark.parametrize("hop", sorted(INSTANCES))
def test_scatter_reads_its_routes_in_one_batch_and_waits_once(hop):
    ins, (segments, reads, waits) = _listing(hop)
    a, b = _scatter_phase(ins, segments)
    routes = [r for r in reads if a <= r.index < b]
    assert len(routes) == 9 and all(r.text.startswith("ds_read_b32") for r in routes), [r.text for r in routes]
    last_read = max(r.index for r in routes)
    first_read = min(r.index for r in routes)
    behind = [ins[k].line for k in range(first_read, last_read) if ins[k].op.startswith("ds_write")]
    assert not behind, f"hop {hop}: route reads issued behind the LDS stores at lines {behind}"
    lines = sorted({r.wait_line for r in routes})                 # the waits that retire a route read
    wait = next(k for k in range(last_read, b) if ins[k].line == lines[0])
    y_stores = [k for k in range(wait, b) if ins[k].op == "ds_write_b64"]    # (the stores that zero Y may stand between the batch and its wait: they queue behind the reads)
    assert len(y_stores) >= 9, len(y_stores)
    print(f"hop {hop}: 9 route reads at lines {routes[0].line}..{routes[-1].line}, waits at {lines}, {len(y_stores)} Y stores behind them")
    assert len(lines) == 1, f"hop {hop}: {len(lines)} waits for the routes (lines {lines})"
    # the batch and its wait are one straight line that no branch of the phase jumps back into: every path through the rotation modes runs them once, first
    assert not any(ins[k].text.endswith(":") or ins[k].op.startswith(("s_cbranch", "s_branch")) for k in range(first_read, wait)), "the batch is not one block"
    label = {i.text[:-1]: k for k, i in enumerate(ins) if i.text.endswith(":")}
    for k in range(wait, b):
        if ins[k].op.startswith(("s_cbranch", "s_branch")):
            assert label[ins[k].text.split()[-1]] > wait, f"the branch at line {ins[k].line} re-enters the batch"
    assert all(ins[k].op != "v_readfirstlane_b32" for k in range(first_read, b)), "bin 256 goes through a scalar branch again"


@pytest.mark.parametrize("hop", sorted(INSTANCES))
def test_hann_rows_and_twiddles_are_issued_twenty_valu_ahead_of_their_use(hop):
    ins, (segments, reads, waits) = _listing(hop)
    by_table = {t: [r for r in reads if r.table == t] for t in ("TW1F", "TW2F", "HANN")}
    for t, rs in by_table.items():
        print(f"hop {hop} {t}: " + ", ".join(f"@{r.line} use +{r.use_valu} wait +{r.valu}" for r in rs))
    # four reads per pass and transform (forward and inverse), four window rows
    assert len(by_table["TW1F"]) == 8 and len(by_table["TW2F"]) == 8 and len(by_table["HANN"]) == 4, {t: len(rs) for t, rs in by_table.items()}
    for t, rs in by_table.items():
        for r in rs:
            # the wait that retires the read (an earlier wait for older traffic retires it too) and the first use of its registers: both that far away
            assert r.valu is not None and min(r.valu, r.use_valu) >= MIN_VALU, \
                f"hop {hop}: {t} read at line {r.line}: waited for {r.valu}, used {r.use_valu} VALU instructions after its issue"


def test_the_listing_of_the_headline_instance_names_every_table_read():
    """The tool's own output: a markdown table with one row per lgkmcnt wait."""
    import io
    out = io.StringIO()
    W.report(_asm(), W.HEADLINE, out)
    text = out.getvalue()
    assert "(HANN)" in text and "(TW1F)" in text and "(TW2F)" in text and text.count("| lgkmcnt(") > 40
    assert re.search(r"frame loop = lines \d+\.\.\d+", text)
