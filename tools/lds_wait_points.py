#!/usr/bin/env python3
"""Where a frame kernel waits for LDS, read off the compiler's assembly (no GPU needed).

    python tools/lds_wait_points.py                                   # the headline instance of pv_wave_kernel.hip
    python tools/lds_wait_points.py --source pv_wave2k_kernel.hip --instance pv_wave2k_kernelILi4ELb0ELb0ELb1E
    python tools/lds_wait_points.py --csrc <dir with another copy of the kernel sources>      # e.g. the parent commit's, for a before / after pair

The kernel file is compiled as tests/resource_usage.py compiles it (device side only, the product's optimisation flags, -S), the frame loop of the named
instance is found (the smallest loop that holds at least eight s_setprio marks) and cut into segments at the s_setprio marks and the `; wave barrier`
comments.  LDS instructions of one wave return in order, so `s_waitcnt lgkmcnt(n)` waits for everything but the n youngest: for every such wait the listing
gives the segment, the youngest LDS READ the wait covers, the number of VALU instructions issued between that read and the wait -- the work that hides the
round trip -- and the number between the read and the first instruction that names its destination registers.  0..15 is an exposed round trip, a few dozen
is a hidden one.

The walk is in text order.  The queue of outstanding operations is kept across labels (the compiler's own insertion is conservative at joins) and dropped
behind an unconditional branch; inside a segment with forward branches only, text order is a superset of every path's order.
"""
import argparse
import os
import re
import subprocess
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from resource_usage import HIPCC  # noqa: E402

HEADLINE = "pv_wave_kernel_1024ILi2ELb0ELb0ELb1ELb1E"
# the shared tables of pv_wave_kernel.hip's LDS carve (TAB_*): absolute byte offsets, the lane's part of the address is in the register
TABLES = (("TW1F", 9216, 13312), ("TW2F", 13312, 13824), ("HANN", 13824, 17920))

Ins = namedtuple("Ins", "line op text")                       # line: 1-based line of the kernel's own listing
# wait_line / valu: the wait that retires the read (None: none in the loop); use_valu: VALU instructions between the read and the first instruction that names
# one of its destination registers -- the wait that CONSUMES it stands there or earlier (a wait for older traffic retires younger reads as well)
Read = namedtuple("Read", "index line text table segment wait_line valu use_valu")
Wait = namedtuple("Wait", "line n segment prio youngest valu retired")


def compile_asm(source="pv_wave_kernel.hip", csrc=None, extra=()):
    """The device assembly of phaze_amd/csrc/<source> (or of <csrc>/<source>; headers it does not hold come from the tree)."""
    tree = os.path.join(ROOT, "phaze_amd", "csrc")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", tree, *extra, "-o", "-", source]
    out = subprocess.run(cmd, cwd=csrc or tree, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def kernel_body(asm, instance):
    """The instructions of the one kernel whose mangled name contains `instance`."""
    lines = asm.splitlines()
    starts = [i for i, s in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(instance) + r"\S*:", s)]
    assert len(starts) == 1, (instance, len(starts))
    body = []
    for s in lines[starts[0] + 1:]:
        if s.startswith(".Lfunc_end") or s.strip().startswith(".end_amdhsa_kernel"):
            break
        body.append(s)
    return body


def instructions(body):
    out = []
    for i, s in enumerate(body, 1):
        t = s.split(";")[0].strip() if "wave barrier" not in s else "; wave barrier"
        if t:
            out.append(Ins(i, t.split()[0] if t[0] != ";" else ";barrier", t))
    return out


def frame_loop(ins):
    """(first, last) index into `ins` of the smallest loop with at least eight s_setprio marks."""
    label = {i.text[:-1]: k for k, i in enumerate(ins) if i.text.endswith(":")}
    best = None
    for k, i in enumerate(ins):
        if i.op.startswith(("s_cbranch", "s_branch")):
            t = label.get(i.text.split()[-1])
            if t is not None and t < k and sum(1 for j in ins[t:k] if j.op == "s_setprio") >= 8:
                if best is None or k - t < best[1] - best[0]:
                    best = (t, k)
    assert best, "no frame loop"
    return best


def _offset(text):
    m = re.search(r"offset:(\d+)", text)
    return int(m.group(1)) if m else 0


def table_of(text):
    if not text.startswith(("ds_read_b128", "ds_read_b64")):     # (b64: the compiler narrows the read of a row of which one half is used)
        return ""
    o = _offset(text)
    return next((n for n, a, b in TABLES if a <= o < b), "")


def is_lds_read(op):
    return op.startswith(("ds_read", "ds_load", "ds_bpermute", "ds_permute", "ds_swizzle"))


def _vregs(operand):
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", operand)
    return {int(m.group(1))} if m else set()


def first_use_valu(ins, k, last):
    """VALU instructions between ins[k] (an LDS read) and the first later instruction that names one of its destination registers."""
    dest = _vregs(ins[k].text.split()[1].rstrip(","))
    n = 0
    for j in ins[k + 1:last + 1]:
        named = set()
        for tok in re.findall(r"v\[\d+:\d+\]|v\d+", j.text):
            named |= _vregs(tok)
        if dest & named:
            return n
        if j.op.startswith("v_"):
            n += 1
    return n


def analyse(ins, first, last):
    """(segments, reads, waits) of ins[first..last].  A segment is {"id", "prio", "first", "last"} (indices into ins)."""
    segments, reads, waits = [], [], []
    seg = {"id": 0, "prio": None, "first": first, "last": first}
    queue = []                                       # outstanding lgkm operations: (index into ins, index into reads or None)
    valu_at = {}
    valu = 0
    for k in range(first, last + 1):
        i = ins[k]
        if i.op in ("s_setprio", ";barrier"):
            seg["last"] = k - 1
            segments.append(seg)
            seg = {"id": seg["id"] + 1, "prio": int(i.text.split()[1]) if i.op == "s_setprio" else seg["prio"], "first": k, "last": k}
        valu_at[k] = valu
        if i.op.startswith("v_"):
            valu += 1
        elif i.op.startswith(("ds_", "s_load", "s_buffer_load", "flat_")):
            r = None
            if is_lds_read(i.op):
                r = len(reads)
                reads.append(Read(k, i.line, i.text, table_of(i.text), seg["id"], None, None, first_use_valu(ins, k, last)))
            queue.append((k, r))
        elif i.op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", i.text)
            if m:
                n = int(m.group(1))
                keep = max(0, len(queue) - n)                    # (n may exceed what the walk has seen: operations issued in front of the loop, or a queue dropped behind a branch)
                gone, queue = queue[:keep], queue[keep:]
                covered = [(q, r) for q, r in gone if r is not None]
                for q, r in covered:
                    reads[r] = reads[r]._replace(wait_line=i.line, valu=valu_at[k] - valu_at[q] - (1 if ins[q].op.startswith("v_") else 0))
                y = reads[covered[-1][1]] if covered else None
                waits.append(Wait(i.line, n, seg["id"], seg["prio"], y, y.valu if y else None, len(covered)))
        elif i.op in ("s_branch", "s_endpgm", "s_setpc_b64"):
            queue = []
    seg["last"] = last
    segments.append(seg)
    return segments, reads, waits


def listing(asm, instance):
    ins = instructions(kernel_body(asm, instance))
    first, last = frame_loop(ins)
    return ins, analyse(ins, first, last)


def report(asm, instance, out=sys.stdout):
    ins, (segments, reads, waits) = listing(asm, instance)
    first, last = segments[0]["first"], segments[-1]["last"]
    print(f"# {instance}: frame loop = lines {ins[first].line}..{ins[last].line} of the kernel's listing, {len(segments)} segments, "
          f"{sum(1 for i in ins[first:last + 1] if i.op.startswith('v_'))} VALU, {sum(1 for i in ins[first:last + 1] if i.op.startswith('ds_'))} LDS instructions, "
          f"{len(waits)} lgkmcnt waits", file=out)
    print("| line | seg | prio | wait | reads retired | VALU since the youngest | VALU to its first use | youngest LDS read covered |", file=out)
    print("|---:|---:|---:|---|---:|---:|---:|---|", file=out)
    for w in waits:
        y = w.youngest
        what = f"`{y.text}`" + (f" ({y.table})" if y.table else "") + f" @{y.line}" if y else "(no LDS read: stores / scalar loads)"
        print(f"| {w.line} | {w.segment} | {'' if w.prio is None else w.prio} | lgkmcnt({w.n}) | {w.retired} | {'' if w.valu is None else w.valu} | {y.use_valu if y else ''} | {what} |", file=out)
    exposed = [w for w in waits if w.youngest and w.valu < 20]
    print(f"\nwaits that cover an LDS read: {sum(1 for w in waits if w.youngest)}; with fewer than 20 VALU instructions behind the read: {len(exposed)}", file=out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--source", default="pv_wave_kernel.hip")
    ap.add_argument("--instance", default=HEADLINE, help="substring of the mangled kernel name")
    ap.add_argument("--csrc", default=None, help="directory to compile <source> in (default: phaze_amd/csrc)")
    ap.add_argument("--asm", default=None, help="read this assembly file instead of compiling")
    ap.add_argument("-D", action="append", default=[], help="extra macro definitions")
    a = ap.parse_args()
    text = open(a.asm).read() if a.asm else compile_asm(a.source, a.csrc, ["-D" + d for d in a.D])
    report(text, a.instance)
