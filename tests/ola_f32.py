"""A plain float32 restatement of the kernel arithmetic of pv_psola.h / pv_tsm.h in numpy.  TEST INFRASTRUCTURE ONLY.

tests/psola_model.py and tests/tsm_model.py define the result in fp64 and bound the kernel's distance from it; this file does what the kernels do,
operation for operation in the stated order, every intermediate a float32:
  window   f = f32(rem) * (1.0f / f32(L)), h = fmaf(f, Hn[q + 1] - Hn[q], Hn[q]); a grain with h == 0 is skipped;
  sample   phi == 0: xt = x[n - D].  Else a = s = 0, for i = 0 .. 63 ascending a = fmaf(w_i, x_i, a), s = s + w_i, then xt = a / s;
  output   num = den = 0, for the grains ascending num = fmaf(h, xt, num), den = den + h; y = num / den, +0.0 where no grain covers the output.
So it shows without a GPU that a faithful float32 implementation meets the gates of tests/test_gpu_ola_ranges.py, and (flush=True) that one which treats
subnormal numbers as zero does not.

fmaf(a, b, c) is emulated as float32(float64(a) * float64(b) + float64(c)).  The product of two float32 is exact in fp64; the sum is rounded to fp64 and then
to float32, a DOUBLE ROUNDING: where the fp64 sum lands exactly on the midpoint of two float32 neighbours although the exact one does not, the result is one
float32 spacing off a true fused multiply-add.  That moves a result by at most one further rounding, which the bounds absorb; it is why this file is compared
with the models within their bound and never bit for bit with a device.

flush=True zeroes every subnormal operand and every subnormal result of an arithmetic operation (sign kept), as a kernel compiled with flushed denormals
does.  Tables in the far notation of tsm_model; TM.from_psola gives them for a psola table."""
import numpy as np

import psola_model as PM
import tsm_model as TM
import vari_model as VM

Q = PM.Q
TAPS = PM.TAPS
TINY = np.float32(2.0 ** -126)                                               # the smallest normal float32


def _ftz(v, flush):
    """v with its subnormal entries replaced by zeros of their sign when `flush`."""
    if not flush:
        return v
    v = np.asarray(v, np.float32)
    return np.where(np.abs(v) < TINY, np.copysign(np.float32(0.0), v), v).astype(np.float32)


def _fma(a, b, c, flush):
    a, b, c = _ftz(a, flush), _ftz(b, flush), _ftz(c, flush)
    r = (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
    return _ftz(r, flush)


def _op(fn, a, b, flush):
    r = fn(_ftz(np.asarray(a, np.float32), flush), _ftz(np.asarray(b, np.float32), flush))
    assert r.dtype == np.float32
    return _ftz(r, flush)


def process(x, grains, out_first=0, nout=None, ptable=None, htable=None, flush=False, stats=None, taps=True):
    """x: float32[nch, nin], far grains int[ngrains, 4] -> float32[nch, nout], outputs out_first .. out_first + nout - 1.  stats: a dict that receives
    min_h (the smallest non-zero window weight), min_tap (the smallest non-zero |w_i| used), max_sum_abs_w (the largest sum |w_i| of a fractional grain); taps=False
    fills it without running the taps (the output is then meaningless)."""
    x = np.asarray(x, np.float32)
    if x.ndim == 1:
        x = x[None, :]
    nch, nin = x.shape
    nout = nin - out_first if nout is None else nout
    P = VM.prototype() if ptable is None else np.asarray(ptable, np.float32)
    Hn = PM.window() if htable is None else np.asarray(htable, np.float32)
    assert P.dtype == np.float32 and Hn.dtype == np.float32
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    one = np.float32(1.0)

    def gather(idx):
        if nin == 0:
            return np.zeros((nch,) + idx.shape, np.float32)
        ok = (idx >= 0) & (idx < nin)
        return np.where(ok, x[:, np.clip(idx, 0, nin - 1)], np.float32(0.0)).astype(np.float32)

    num = np.zeros((nch, nout), np.float32)
    den = np.zeros(nout, np.float32)
    covered = np.zeros(nout, bool)
    min_h, min_tap, max_saw = np.inf, np.inf, 0.0
    for t, w_, D, L in g.tolist():
        tf, phi = w_ & (Q - 1), w_ >> 8
        lo, hi = max(t - L + 1, out_first), min(t + L, out_first + nout - 1)
        if lo > hi:
            continue
        n = np.arange(lo, hi + 1, dtype=np.int64)
        ua = np.abs(Q * (n - t) - tf)
        n, ua = n[ua < Q * L], ua[ua < Q * L]
        u4 = 4 * ua
        q = np.minimum(u4 // L, 1024)
        rem = u4 - (u4 // L) * L
        f = _op(np.multiply, rem.astype(np.float32), _op(np.divide, one, np.float32(L), flush), flush)
        h = _fma(f, _op(np.subtract, Hn[q + 1], Hn[q], flush), Hn[q], flush)
        nz = h != 0
        if not nz.any():
            continue
        n, h = n[nz], h[nz]
        min_h = min(min_h, float(np.min(np.abs(h))))
        sl = n - out_first
        if phi == 0:
            xt = gather(n - D)
        else:
            theta = Q - phi
            w = P[np.abs(Q * (np.arange(TAPS) - (TAPS // 2 - 1)) - theta)]
            min_tap = min(min_tap, float(np.min(np.abs(w[w != 0]))))
            max_saw = max(max_saw, float(np.sum(np.abs(w.astype(np.float64)))))
            a = np.zeros((nch, n.size), np.float32)
            s = np.float32(0.0)
            b = n - D - 1 - (TAPS // 2 - 1)
            xv = gather(b[:, None] + np.arange(TAPS)[None, :]) if taps else None                # [nch, len, 64]
            for i in range(TAPS if taps else 0):
                a = _fma(w[i], xv[:, :, i], a, flush)
                s = _op(np.add, s, w[i], flush)
            xt = _op(np.divide, a, s, flush) if taps else a
        num[:, sl] = _fma(h, xt, num[:, sl], flush)
        den[sl] = _op(np.add, den[sl], h, flush)
        covered[sl] = True
    y = np.zeros((nch, nout), np.float32)
    y[:, covered] = _op(np.divide, num[:, covered], den[covered], flush)
    if stats is not None:
        stats.update(min_h=min_h, min_tap=min_tap, max_sum_abs_w=max_saw)
    return y


def scaling_conditions(tables):
    """The conditions under which scaling the input by 2^k scales every intermediate of the kernel exactly, from the restatement and the model over
    `tables`, an iterable of (x float32[nch, nin], far grains, nout): (smallest, largest, k_top).
      smallest  smallest non-zero |h| * smallest non-zero |w_i| * smallest non-zero |x|: above 2^-126 after scaling, no product of a tap or of a grain
                falls into the subnormal range, where the spacing no longer scales;
      largest   max_phi sum |w_i| * max den * max |x|, which bounds |a|, |xt| (|s| >= 1 is asserted) and |num|;
      k_top     the largest k with largest * 2^k < 2^128."""
    min_h = min_tap = min_x = np.inf
    saw = den_max = max_x = 0.0
    for x, g, nout in tables:
        st = {}
        process(x, g, 0, nout, stats=st, taps=False)
        _, _, _, _, den = TM.process(x, g, 0, nout, bound=True, subnormal="derived")
        P = VM.prototype()
        for phi in sorted(set((np.asarray(g).reshape(-1, 4)[:, 1] >> 8).tolist()) - {0}):
            w = P[np.abs(Q * (np.arange(TAPS) - (TAPS // 2 - 1)) - (Q - phi))].astype(np.float64)
            assert abs(w.sum()) >= 1.0
        ax = np.abs(np.asarray(x, np.float64))
        min_h, min_tap, min_x = min(min_h, st["min_h"]), min(min_tap, st["min_tap"]), min(min_x, float(ax[ax > 0].min()))
        saw, den_max, max_x = max(saw, st["max_sum_abs_w"]), max(den_max, float(den.max())), max(max_x, float(ax.max()))
    smallest, largest = min_h * min_tap * min_x, saw * den_max * max_x
    k_top = int(np.floor(128 - np.log2(largest)))
    while largest * 2.0 ** k_top >= 2.0 ** 128:
        k_top -= 1
    return dict(min_h=min_h, min_tap=min_tap, min_x=min_x, smallest=smallest, sum_abs_w=saw, den_max=den_max, max_x=max_x, largest=largest, k_top=k_top)
