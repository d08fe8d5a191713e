"""CPU model of per-take plans on the overlap-add path (Takes / pv_takes_*): plain numpy on top of tests/tsm_model.py.  TEST INFRASTRUCTURE ONLY, and the
normative definition (DESIGN.md "Takes"); the reference has no counterpart.

A call has K takes, each with its own input, far-grain table, first output and output count.  Take k's output is tsm_model.process on take k alone.
  tiles    take k's outputs go in tiles of 1024 from its own out_first on: tsm_model.tiles per take, concatenated in (take, tile) order.  A record is
           {take, first, g_first, g_end, src0, src_count, cls, 0}: first = 1024 j for the take's tile j, the grain range counts within the take's table.
  class    cls = min(4, 163840 div lds_bytes(s)), s = max(128, src_count rounded up to 64): how many workgroups that stage s samples the LDS of a
           compute unit holds.  lds_bytes(s) is tsm_model.lds_bytes's formula for a launch that stages s samples.  Where the rounded s would not fit
           the LDS at all, s is src_count itself and the class is 1 (launch_span).
  order    the tile ids sorted by class, (take, tile) order kept within a class (a stable sort): one launch per non-empty class."""
import numpy as np

import psola_model as PM
import tsm_model as TM
import vari_model as VM

TILE = TM.TILE
CLASSES = 4
MAX_TAKES = 65536
_TABLE_WORDS = ((VM.prototype().size + 3) & ~3) + ((PM.WINDOW + 3) & ~3)       # P and Hn


def lds_bytes(s):
    """Dynamic LDS of a launch that stages s samples per tile: tsm_model.lds_bytes with the span given."""
    return 4 * (((s + (s >> 6) + 4) & ~3) + _TABLE_WORDS)


def launch_span(src_count):
    """Samples a launch stages when its longest tile reads src_count: the count rounded up to 64, at least 128.  A configuration's span need not be a
    multiple of 64, so within 63 samples of the largest span that fits the LDS the rounded count would not fit: there it is the count itself, which fits
    because the span does."""
    s = max(128, (src_count + 63) & ~63)
    return src_count if lds_bytes(s) > TM.LDS_BYTES else s


def cls(src_count):
    """1 .. 4 for every count a configuration accepts."""
    return max(1, min(CLASSES, TM.LDS_BYTES // lds_bytes(launch_span(src_count))))


def process(xs, tables, out_firsts, nouts, **kw):
    """A list of fp64[nch, nout_k]: tsm_model.process per take."""
    return [TM.process(x, g, f, n, **kw) for x, g, f, n in zip(xs, tables, out_firsts, nouts)]


def tiles(tables, max_period, out_firsts, nouts):
    """int64[ntiles, 8] {take, first, g_first, g_end, src0, src_count, cls, 0} in (take, tile) order."""
    out = []
    for k, (g, f, n) in enumerate(zip(tables, out_firsts, nouts)):
        for j, (a, b, s0, cnt) in enumerate(TM.tiles(g, max_period, f, n).tolist()):
            out.append([k, j * TILE, a, b, s0, cnt, cls(cnt), 0])
    return np.array(out, np.int64).reshape(-1, 8)


def check_span(tables, max_period, max_rate, out_firsts, nouts):
    """None when every tile of every take fits the span, else (take, tile, its first grain, its extent)."""
    for k, (g, f, n) in enumerate(zip(tables, out_firsts, nouts)):
        bad = TM.check_span(g, max_period, max_rate, f, n)
        if bad is not None:
            return (k,) + tuple(bad)
    return None


def order(t):
    """The tile ids by class, stable."""
    t = np.asarray(t).reshape(-1, 8)
    return np.argsort(t[:, 6], kind="stable")
