#!/usr/bin/env python3
"""What the compiler adds around the arithmetic of a frame loop: hazard pads and register copies, read off the assembly (no GPU needed).

    python tools/isa_copies.py                                    # the four fp32-first pitchFactor >= 1 instances of pv_wave_kernel.hip
    python tools/isa_copies.py --csrc <dir with another copy of the kernel sources>        # e.g. the parent commit's, for a before / after pair
    python tools/isa_copies.py --instance pv_wave_kernel_1024ILi2ELb0ELb0ELb1ELb1E --lines plain

The kernel file is compiled as tools/lds_wait_points.py compiles it and the frame loop of an instance is found the same way.  The loop is cut into basic
blocks and ONE path per rotation mode of the scatter is walked from the loop's head to its back edge, by the rule of tools/isa_path_walk.py: an exec-mask
skip (s_cbranch_execz) falls through -- the masked block runs, as it does when any lane is active --, s_cbranch_execnz is taken.  Every other conditional
branch is wave-uniform; of its two ways the walk keeps those that stay on the class-A path: no block with a call (s_swappc_b64: the shift-table rebuild,
the out-of-line forward transforms) and no block with fp64 arithmetic (the inline fp64-first transform).  Of the paths left, the scatter phase -- the code
between the loop's two `s_setprio 3` -- tells the rotation mode: each mode has its own copy of the nine Y stores (ds_write_b64), and by the VALU work in
front of them the copies are `plain` (frames with t = 0 mod N: none), `flip` (t = N/2: sign flips) and `rotate` (the general rotation; at hop >= 512 the
code exists but no frame takes it).  Per mode the LONGEST path is reported: the one that skips nothing but what the rule excludes.

Counted along a path:
  * pads: s_nop, as the sum of wait states (s_nop n = n + 1)
  * v->v: v_mov_b32 / v_mov_b64 from a VGPR (not DPP moves: those move data across lanes)
  * s->v: v_mov_b32 / v_mov_b64 from an SGPR (a wave-uniform value re-materialised in a vector register; inline constants and literals are not counted)
  * VALU: every v_* instruction
"""
import argparse
import os
import re
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lds_wait_points as W  # noqa: E402

INSTANCES = {128: "pv_wave_kernel_1024ILi1ELb0ELb0ELb1ELb1E", 256: "pv_wave_kernel_1024ILi2ELb0ELb0ELb1ELb1E",
             512: "pv_wave_kernel_1024ILi4ELb0ELb0ELb1ELb1E", 1024: "pv_wave_kernel_1024ILi8ELb0ELb0ELb1ELb1E"}
MODES = ("plain", "flip", "rotate")
FIELDS = ("pads", "vv", "sv", "valu")
Counts = namedtuple("Counts", FIELDS)


def _is_mov(op):
    return re.fullmatch(r"v_mov_b(32|64)(_e32|_e64)?", op) is not None


def count(seq):
    """Counts of a sequence of lds_wait_points.Ins."""
    pads = vv = sv = valu = 0
    for i in seq:
        if i.op == "s_nop":
            pads += int(i.text.split()[1], 0) + 1
        elif i.op.startswith("v_"):
            valu += 1
            if _is_mov(i.op):
                src = i.text.split(",")[-1].strip()
                if re.fullmatch(r"v\d+|v\[\d+:\d+\]", src):
                    vv += 1
                elif re.fullmatch(r"s\d+|s\[\d+:\d+\]", src):
                    sv += 1
    return Counts(pads, vv, sv, valu)


def blocks(ins, first, last):
    """The loop ins[first..last] as basic blocks: [(first index, last index)], cut in front of labels and behind branches."""
    cuts = {first}
    for k in range(first, last + 1):
        if ins[k].text.endswith(":"):
            cuts.add(k)
        if ins[k].op.startswith(("s_cbranch", "s_branch")) and k + 1 <= last:
            cuts.add(k + 1)
    starts = sorted(cuts)
    return [(a, (starts[n + 1] - 1) if n + 1 < len(starts) else last) for n, a in enumerate(starts)]


def _forbidden(ins, a, b):
    return any(i.op == "s_swappc_b64" or (i.op.startswith("v_") and "_f64" in i.op and not i.op.startswith("v_cvt")) for i in ins[a:b + 1])


def paths(ins, first, last):
    """Every path (list of block numbers) from the loop's head to its back edge under the walking rule of the module text."""
    bl = blocks(ins, first, last)
    at = {a: n for n, (a, b) in enumerate(bl)}
    label = {i.text[:-1]: k for k, i in enumerate(ins) if i.text.endswith(":")}
    bad = [_forbidden(ins, a, b) for a, b in bl]
    found = []

    def walk(n, trail):
        assert len(found) < 100000, "too many paths"
        if bad[n]:
            return
        trail = trail + [n]
        a, b = bl[n]
        t = ins[b]
        nxt = []
        if t.op.startswith(("s_cbranch", "s_branch")):
            tgt = label.get(t.text.split()[-1])
            back = tgt == first
            inside = tgt is not None and first < tgt <= last
            if t.op == "s_branch" or t.op == "s_cbranch_execnz":
                if back:
                    found.append(trail)
                    return
                nxt = [tgt] if inside else []                   # (a branch out of the loop ends the chain: not a frame's path)
            elif t.op == "s_cbranch_execz":
                nxt = [b + 1]
            else:
                if back:
                    found.append(trail)
                elif inside:
                    nxt.append(tgt)
                nxt.append(b + 1)
        else:
            nxt = [b + 1]
        for k in nxt:
            if k <= last and k in at:
                walk(at[k], trail)

    sys.setrecursionlimit(10000)
    walk(0, [])
    return bl, found


def scatter_of(ins, seq_idx):
    """(indices of the first ten Y stores, VALU count) of a path's scatter phase; None for a path without the phase."""
    marks = [k for k in seq_idx if ins[k].op == "s_setprio" and ins[k].text.split()[1] == "3"]
    if len(marks) != 2:
        return None
    a, b = seq_idx.index(marks[0]), seq_idx.index(marks[1])
    stores = tuple(k for k in seq_idx[a:b] if ins[k].op == "ds_write_b64")[:10]     # bin 512's zero and the nine sources; behind them the NaN frames' poison
    return stores, sum(1 for k in seq_idx[a:b] if ins[k].op.startswith("v_"))


def frame_paths(asm, instance):
    """{mode: (Counts, [Ins along the path])} of one instance's frame loop."""
    ins = W.instructions(W.kernel_body(asm, instance))
    first, last = W.frame_loop(ins)
    bl, found = paths(ins, first, last)
    best = {}                                                    # Y stores of the scatter phase -> (the phase's VALU count, the longest path through them)
    for p in found:
        idx = [k for n in p for k in range(bl[n][0], bl[n][1] + 1)]
        s = scatter_of(ins, idx)
        if s is None or len(s[0]) < 10:                          # (the dispatch of the three modes is a chain of flag tests: a walk through it that enters none is no frame's path)
            continue
        if s[0] not in best or len(idx) > len(best[s[0]][1]):
            best[s[0]] = (s[1], idx)
    assert len(best) == len(MODES), (instance, len(best))
    ranked = sorted(best.values(), key=lambda v: v[0])           # plain < flip < rotate by the work of the scatter
    return {m: (count([ins[k] for k in idx]), [ins[k] for k in idx]) for m, (_, idx) in zip(MODES, ranked)}


def table(asm, instances=INSTANCES, out=sys.stdout):
    print("| hop | mode | pads (wait states) | v->v moves | s->v moves | VALU |", file=out)
    print("|---:|---|---:|---:|---:|---:|", file=out)
    for hop in sorted(instances):
        best = frame_paths(asm, instances[hop])
        for m in MODES:
            c = best[m][0]
            print(f"| {hop} | {m} | {c.pads} | {c.vv} | {c.sv} | {c.valu} |", file=out)


def read_table(path):
    """{(hop, mode): Counts} of a table written by table()."""
    got = {}
    with open(path) as f:
        for line in f:
            m = re.fullmatch(r"\|\s*(\d+)\s*\|\s*(\w+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*", line)
            if m:
                got[(int(m.group(1)), m.group(2))] = Counts(*(int(x) for x in m.groups()[2:]))
    return got


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--source", default="pv_wave_kernel.hip")
    ap.add_argument("--instance", default=None, help="substring of one mangled kernel name (default: the four fp32-first pitchFactor >= 1 instances)")
    ap.add_argument("--csrc", default=None, help="directory to compile <source> in (default: phaze_amd/csrc)")
    ap.add_argument("--asm", default=None, help="read this assembly file instead of compiling")
    ap.add_argument("--lines", default=None, choices=MODES, help="print the instructions of this mode's path (with --instance)")
    ap.add_argument("-D", action="append", default=[], help="extra macro definitions")
    a = ap.parse_args()
    text = open(a.asm).read() if a.asm else W.compile_asm(a.source, a.csrc, ["-D" + d for d in a.D])
    if a.instance and a.lines:
        for i in frame_paths(text, a.instance)[a.lines][1]:
            print(i.line, i.text)
    else:
        table(text, {0: a.instance} if a.instance else INSTANCES)
