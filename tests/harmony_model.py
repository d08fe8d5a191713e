"""CPU model of harmony voices on the overlap-add path (Harmony / pv_harmony_*, pv_harmony_ratios): plain numpy.  TEST INFRASTRUCTURE ONLY, and the
normative definition (DESIGN.md "Harmony voices"); the reference has no counterpart.

A call has V voices, 1 <= V <= 8.  Voice v is a far-grain table of tests/tsm_model.py and y_v = TM.process(x, table_v): one num / den per voice.  gains[v, c]
is a finite float32.  For channel c and output n, in float32: acc = 0; for v ascending, voice v is skipped where gains[v, c] == 0 or no grain of voice v
covers n with a non-zero weight; else acc = acc + f32(gains[v, c] * f32(y_v[n])), the product rounded on its own.  out[c, n] = acc.
  tiles    a call's outputs go in tiles of 1024 as TM.tiles.  Per tile every voice has its own grain range and source range [lo_v, hi_v) (TM.tiles on the
           voice's table); the tile stages the HULL [min lo_v, max hi_v) over the voices that have a grain on the tile, once for all voices.  The hull's
           extent must not exceed TM.span(max_period, max_rate), even when every voice alone would fit.
  ratios   harmony_ratios: PM.tune_ratios's one-pole r_j, shared by the voices; voice v lies degrees[v] ALLOWED notes away from the note ns the lead is
           corrected onto, i semitones, and its ratio is clamp(2^(r_j + i / 12), 1/2, 2); i = 0 for degree 0 and for unvoiced or empty records."""
import math

import numpy as np

import f0_model as FM
import tsm_model as TM

MAX_VOICES = 8
MAX_DEGREE = 24
TILE = TM.TILE


def mix(ys, covered, gains):
    """The float32 fold: ys float32[V, nch, nout] per-voice outputs, covered bool[V, nout], gains float32[V, nch] -> float32[nch, nout]."""
    ys = np.asarray(ys, np.float32)
    gains = np.asarray(gains, np.float32)
    acc = np.zeros(ys.shape[1:], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in range(ys.shape[0]):
            prod = (gains[v][:, None] * ys[v]).astype(np.float32)                      # rounded on its own
            take = (gains[v] != 0.0)[:, None] & np.asarray(covered[v], bool)[None, :]
            acc = np.where(take, (acc + prod).astype(np.float32), acc)
    return acc


def _gains(gains, nv, nch):
    g = np.asarray(gains, np.float32)
    if g.ndim == 1:
        g = np.repeat(g[:, None], nch, axis=1)
    if g.shape != (nv, nch) or not np.all(np.isfinite(g)):
        raise ValueError("gains: finite, [V] or [V, nch]")
    return g


def process(x, tables, gains, out_first=0, nout=None, ptable=None, htable=None, bound=False, outs=None):
    """x: float32[nch, nin], tables: a list of far-grain tables, gains [V] or [V, nch] -> float32[nch, nout]: TM.process per voice in fp64, rounded to
    float32, then mix().  The model's own per-voice outputs are not the kernel's bits (TM.process is fp64), so against the GPU use bound=True: returns
    (y fp64, tol, poisoned) with y = sum_v g_v y_v in fp64 over the voices that are not skipped and
        tol = sum |g_v| tol_v + (V + 1) 2^-24 sum |g_v| (|y_v| + tol_v) + sum of the voices' subnormal slack,
    tol_v TM.process's derived bound: the kernel's y_v is within tol_v of the model's, every product and every add of the fold rounds once (at most
    2^-24 relative each, V adds and one product per voice, on partial sums of at most sum |g_v| (|y_v| + tol_v)), and a product in the subnormal range
    is within 2^-150 absolute: V 2^-149 covers products and adds.  poisoned: where a voice that is not skipped has a non-finite sample under a tap.
    outs: the list of TM.process(x, table_v, ..., bound=True) per voice, when the caller has it already."""
    x = np.asarray(x, np.float32)
    if x.ndim == 1:
        x = x[None, :]
    nch, nin = x.shape
    nout = nin - out_first if nout is None else nout
    nv = len(tables)
    if not 1 <= nv <= MAX_VOICES:
        raise ValueError("1 to 8 voices")
    g = _gains(gains, nv, nch)
    if outs is None:
        outs = [TM.process(x, t, out_first, nout, ptable, htable, bound=True) for t in tables]
    covered = [o[1][0] > 0 for o in outs]                                              # tol > 0 exactly where a grain covers the output
    if not bound:
        return mix([o[0].astype(np.float32) for o in outs], covered, g)
    y = np.zeros((nch, nout)); tol = np.zeros((nch, nout)); mag = np.zeros((nch, nout))
    poisoned = np.zeros((nch, nout), bool)
    for v, (yv, tv, pv) in enumerate(outs):
        take = (g[v] != 0.0)[:, None] & covered[v][None, :]
        a = np.abs(g[v].astype(np.float64))[:, None]
        y += np.where(take, g[v].astype(np.float64)[:, None] * yv, 0.0)
        tol += np.where(take, a * tv, 0.0)
        mag += np.where(take, a * (np.abs(yv) + tv), 0.0)
        poisoned |= take & pv
    tol = tol + (nv + 1) * 2.0 ** -24 * mag + nv * 2.0 ** -149
    return y, tol, poisoned


def tiles(tables, max_period, out_first, nout):
    """(hull int64[ntiles, 2] {src0, src_count}, ranges int64[ntiles, V, 2] {g_first, g_end} as indices into the concatenated table) as the host uploads
    them: TM.tiles per voice, and the hull over the voices with a grain on the tile ({0, 0} when none has one)."""
    per = [TM.tiles(t, max_period, out_first, nout) for t in tables]
    first = np.concatenate([[0], np.cumsum([np.asarray(t).reshape(-1, 4).shape[0] for t in tables])])
    ntiles = per[0].shape[0]
    hull = np.zeros((ntiles, 2), np.int64)
    ranges = np.zeros((ntiles, len(tables), 2), np.int64)
    for k in range(ntiles):
        live = [p[k] for p in per if p[k, 3] > 0]
        if live:
            lo = min(int(p[2]) for p in live)
            hi = max(int(p[2] + p[3]) for p in live)
            hull[k] = [lo, hi - lo]
        for v, p in enumerate(per):
            ranges[k, v] = [first[v] + p[k, 0], first[v] + p[k, 1]]
    return hull, ranges


def check_span(tables, max_period, max_rate, out_first, nout):
    """None when the hull of every tile of the call fits the span, else (tile, lowest voice with a grain on it, that voice's first grain of the tile
    counted within the voice, the hull's extent)."""
    cap = TM.span(max_period, max_rate)
    hull, _ = tiles(tables, max_period, out_first, nout)
    for k, (_, cnt) in enumerate(hull.tolist()):
        if cnt > cap:
            for v, t in enumerate(tables):
                p = TM.tiles(t, max_period, out_first, nout)[k]
                if p[3] > 0:
                    return k, v, int(p[0]), cnt
    return None


def check_voices(tables, max_period):
    """None when every voice's table is well formed, else (voice, index of its first bad grain, why)."""
    for v, t in enumerate(tables):
        bad = TM.check_grains(t, max_period)
        if bad is not None:
            return (v,) + bad
    return None


def _allowed(mask, note):
    return bool((mask >> (note % 12)) & 1)


def interval(ns, degree, scale_mask):
    """Semitones from the allowed note ns to the one |degree| allowed notes above (below, for a negative degree)."""
    m, left = ns, abs(degree)
    while left > 0:
        m += 1 if degree > 0 else -1
        if _allowed(scale_mask, m):
            left -= 1
    return m - ns


def harmony_ratios(records, sample_rate, degrees, scale_mask=0xFFF, strength=1.0, retune=1.0, a4=440.0):
    """float64[V, nrec] of pv_harmony_ratios."""
    degrees = [int(k) for k in degrees]
    if (not 1 <= scale_mask <= 0xFFF or not 0.0 <= strength <= 1.0 or not 0.0 < retune <= 1.0 or not sample_rate > 0.0 or not a4 > 0.0
            or not 1 <= len(degrees) <= MAX_VOICES or any(abs(k) > MAX_DEGREE for k in degrees)):
        raise ValueError("bad argument")
    recs = np.asarray(records, np.int32).reshape(-1, 4)
    out = np.zeros((len(degrees), recs.shape[0]), np.float64)
    r = 0.0
    for j, rec in enumerate(recs):
        p, t, ns = FM.period(rec), 0.0, None
        if p > 0.0:
            n = 69.0 + 12.0 * math.log2(sample_rate / p / a4)
            ns = FM.nearest_allowed(n, scale_mask)
            t = strength * (float(ns) - n) / 12.0
        r += retune * (t - r)
        for v, k in enumerate(degrees):
            i = interval(ns, k, scale_mask) if ns is not None else 0
            out[v, j] = min(max(2.0 ** (r + i / 12.0), 0.5), 2.0)
    return out
