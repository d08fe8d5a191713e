"""CPU model of mirrored grains on the overlap-add path (Mirror / pv_mirror_*, pv_mirror_plan): plain numpy, fp64.  TEST INFRASTRUCTURE ONLY, and the
normative definition (DESIGN.md "Mirrored grains"); the reference has no counterpart.

A grain is four int32 {t, w, D, L} with w = tf + 256 phi + 65536 m, tf and phi in 0 .. 255, m in {0, 1}.  With m = 0 it is the far grain of
tests/tsm_model.py word for word: output n reads the input at the real position n - D - phi / 256.  With m = 1 the grain is MIRRORED: output n reads
the input at D - n - phi / 256, so the grain plays its stretch of the input backwards.  Window and output rules do not change; the sample rule is the
forward one with n - D replaced by D - n and nothing else: phi == 0 reads x[D - n] itself, else theta = 256 - phi, b = D - n - 1 and the taps
i = 0 .. 63 read x[b - 31 + i] with weight P[|256 (i - 31) - theta|], a = fmaf(w_i, x_i, a), s += w_i for i ascending, xt = a / s.
  check    0 <= w < 131072; for m = 1, D > -2^30 (any larger int32: D is a sum of two positions below 2^30); for m = 0, |D| < 2^30; the rest is
           tsm_model.check_grains.
  tiles    the grain range [a, b) of a tile is tsm_model's walk (t and L only).  A forward grain's source range is tsm_model's; a mirrored grain that
           reaches the tile [j0, j1) has lo = D - min(j1, t + L) - 33 and hi = D - max(j0, t - L) + 32.  src0 = min lo, src_count = max hi - min lo over
           both kinds; every tap of a covered output lies in [lo + 1, hi - 1].
The planner is tsm_model.tsm_plan with one more rule: in an unvoiced stretch every second use of an analysis mark is mirrored about that mark."""
import math

import numpy as np

import epoch_model as EM
import f0_model as FM
import psola_model as PM
import tsm_model as TM
import vari_model as VM

Q = TM.Q
TAPS = TM.TAPS
TILE = TM.TILE
MAX_PERIOD = TM.MAX_PERIOD
MAX_POSITION = TM.MAX_POSITION
MIRROR = Q * Q                                                             # bit 16 of w
span = TM.span
lds_bytes = TM.lds_bytes


def mirrored(grains):
    """bool[ngrains]: bit 16 of w."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    return (g[:, 1] & MIRROR) != 0


def check_grains(grains, max_period):
    """None when the table is well formed, else (index of the first bad grain, why): TM.check_grains with the direction bit."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    prev = 0
    for k, (t, w, D, L) in enumerate(g.tolist()):
        if not (0 <= t < MAX_POSITION and 0 <= w < 2 * MIRROR):
            return k, "centre"
        if not 2 <= L <= max_period:
            return k, "half length"
        if (D <= -MAX_POSITION or D >= 1 << 31) if w & MIRROR else abs(D) >= MAX_POSITION:
            return k, "shift"
        if t * Q + (w & (Q - 1)) < prev:
            return k, "out of order"
        prev = t * Q + (w & (Q - 1))
    return None


def tiles(grains, max_period, out_first, nout):
    """int64[ntiles, 4] {g_first, g_end, src0, src_count} of the call's tiles (src_count = hi - lo, 0 for a tile without grains)."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    ng = g.shape[0]
    t, D, L = g[:, 0], g[:, 2], g[:, 3]
    m = (g[:, 1] & MIRROR) != 0
    out = []
    lo = hi = 0
    for k in range((nout + TILE - 1) // TILE):
        j0 = out_first + k * TILE
        j1 = j0 + min(TILE, nout - k * TILE)
        while lo < ng and t[lo] < j0 - max_period - 1:
            lo += 1
        hi = max(hi, lo)
        while hi < ng and t[hi] < j1 + max_period:
            hi += 1
        a, b = lo, hi
        while a < b and t[a] + 1 + L[a] <= j0:
            a += 1
        while b > a and t[b - 1] - L[b - 1] >= j1:
            b -= 1
        s = slice(a, b)
        reach = (t[s] + L[s] >= j0) & (t[s] - L[s] < j1)
        if reach.any():
            first, last = np.maximum(j0, t[s] - L[s]), np.minimum(j1, t[s] + L[s])
            from_ = np.where(m[s], D[s] - last - 33, first - D[s] - 33)
            to = np.where(m[s], D[s] - first + 32, last - D[s] + 32)
            s0, s1 = int(np.min(from_[reach])), int(np.max(to[reach]))
            out.append([a, b, s0, s1 - s0])
        else:
            out.append([a, b, 0, 0])
    return np.array(out, np.int64).reshape(-1, 4)


def check_span(grains, max_period, max_rate, out_first, nout):
    """None when every tile of the call fits the span, else (tile, its first grain, its extent)."""
    cap = span(max_period, max_rate)
    for k, (a, b, s0, cnt) in enumerate(tiles(grains, max_period, out_first, nout).tolist()):
        if cnt > cap:
            return k, a, cnt
    return None


def process(x, grains, out_first=0, nout=None, ptable=None, htable=None, bound=False, subnormal=None):
    """x: float32[nch, nin], grains int[ngrains, 4] -> fp64[nch, nout], outputs out_first .. out_first + nout - 1.  TM.process operation for operation
    (a table with every m = 0 gives its bits), with the addresses of a mirrored grain running downwards.  bound=True returns (y, tol, poisoned) as
    TM.process does: the derived bound of tests/test_gpu_psola.py holds unchanged, since the direction enters the addresses only, never a rounded
    value.  subnormal="derived" as TM.process."""
    x = np.asarray(x, np.float32)
    if x.ndim == 1:
        x = x[None, :]
    nch, nin = x.shape
    nout = nin - out_first if nout is None else nout
    P = (VM.prototype() if ptable is None else np.asarray(ptable, np.float32)).astype(np.float64)
    Hn = PM.window() if htable is None else np.asarray(htable, np.float32)
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    bad = ~np.isfinite(x)
    clean = np.where(bad, np.float32(0.0), x).astype(np.float64)

    def gather(idx):
        """(samples fp64, non-finite flags) at the positions idx, zeros and False outside [0, nin)."""
        if nin == 0:
            return np.zeros((nch,) + idx.shape), np.zeros((nch,) + idx.shape, bool)
        ok = (idx >= 0) & (idx < nin)
        c = np.clip(idx, 0, nin - 1)
        return np.where(ok, clean[:, c], 0.0), bad[:, c] & ok

    num = np.zeros((nch, nout)); den = np.zeros(nout)
    A = np.zeros((nch, nout)); S = np.zeros(nout); E = np.zeros((nch, nout)); G = np.zeros(nout, np.int64)
    Z = np.zeros(nout)                                                    # sum |h_g| (64 / |d_g| + 1) over the fractional grains
    poisoned = np.zeros((nch, nout), bool)
    u = 2.0 ** -24
    i = np.arange(TAPS, dtype=np.int64)
    for t, w_, D, L in g.tolist():
        tf, phi, mir = w_ & (Q - 1), (w_ >> 8) & (Q - 1), (w_ >> 16) & 1
        lo, hi = max(t - L + 1, out_first), min(t + L, out_first + nout - 1)
        if lo > hi:
            continue
        n = np.arange(lo, hi + 1, dtype=np.int64)
        h, fd, nz = PM.grain_weights(n, t, tf, L, Hn)
        if not nz.any():
            continue
        n, h, fd = n[nz], h[nz], fd[nz]
        sl = n - out_first
        at = D - n if mir else n - D                                        # the whole part of the read position: the only place the direction enters
        if phi == 0:
            xt, hit = gather(at)
            e = np.zeros_like(xt)
        else:
            w = P[np.abs(Q * (i - (TAPS // 2 - 1)) - (Q - phi))]
            xv, hits = gather((at - 1 - (TAPS // 2 - 1))[:, None] + i[None, :])         # [nch, len, 64]
            Dg = w.sum()
            xt = (xv * w).sum(axis=2) / Dg
            e = u * (TAPS * ((np.abs(xv) * np.abs(w)).sum(axis=2) + np.abs(xt) * np.abs(w).sum()) / abs(Dg) + np.abs(xt))
            hit = hits.any(axis=2)
        m = np.abs(h) + fd
        num[:, sl] += h * xt
        den[sl] += h
        A[:, sl] += m * np.abs(xt)
        S[sl] += m
        E[:, sl] += np.abs(h) * e
        if phi != 0:
            Z[sl] += np.abs(h) * (TAPS / abs(Dg) + 1.0)
        G[sl] += 1
        poisoned[:, sl] |= hit
    cov = G > 0
    y = np.zeros((nch, nout))
    y[:, cov] = num[:, cov] / den[cov]
    if not bound:
        return y
    tol = np.zeros((nch, nout))
    Gc = (G[cov] + 3).astype(np.float64)
    rel = ((u * Gc * (A[:, cov] + np.abs(y[:, cov]) * S[cov]) + E[:, cov]) / den[cov] + u * np.abs(y[:, cov])) * (1.0 + 2.0 ** -10)
    if subnormal is None:
        tol[:, cov] = rel + 2.0 ** -149 * (1.0 + (Gc + TAPS) / den[cov])
        return y, tol, poisoned
    if subnormal != "derived":
        raise ValueError("subnormal: None or 'derived'")
    tol[:, cov] = rel + 2.0 ** -150 * ((Z[cov] + G[cov]) / den[cov] + 2.0)
    return y, tol, poisoned, G, den


# ---- the planner ------------------------------------------------------------------------------------------------------------------------------

def mirror_plan(records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios=None, rates=None, epochs=None, min_strength=0,
                lock=EM.DEFAULT_LOCK, mirror=True, offset=None, details=False):
    """(int32[ngrains, 4] grains, output_len) of pv_mirror_plan: TM.tsm_plan, restated here statement for statement, with the direction of every grain.
    mirror=False: tsm_plan's grains bit for bit.  mirror=True: the walk, the marks, T, V, c, L and output_len do not change; a grain held at (T, A) is a
    REUSE when a grain was held before it, that grain's analysis mark is this very A (the same fp64 value: the walk did not advance) and the record at A
    is unvoiced or there are no records; a reuse takes the opposite direction of the grain before it, every other grain is forward.  A mirrored grain
    reads about its own mark (input A - (tau - T) lands at output tau): sq = floor(256 (T + A) + 1/2), D = (sq + 255) >> 8, phi = 256 D - sq,
    w = tf + 256 phi + 65536.  details=True returns also, per grain, its analysis mark A (float64) and whether the record at A is voiced."""
    records = np.asarray(records, np.int32).reshape(-1, 4)
    nrec = records.shape[0]
    if (f0_hop < 1 or min_period < 2 or max_period < min_period or max_period > MAX_PERIOD or not min_period <= unvoiced_period <= max_period
            or not 0 <= input_len < MAX_POSITION or not 0.0 < lock <= 1.0 or not 0 <= min_strength <= EM.S_ONE):
        raise ValueError("bad argument")
    if ratios is not None:
        ratios = np.asarray(ratios, np.float64)
        if ratios.shape != (nrec,) or not np.all((ratios >= 0.5) & (ratios <= 2.0)):
            raise ValueError("bad ratios")
    if rates is not None:
        rates = np.asarray(rates, np.float64)
        if rates.shape != (nrec,) or not np.all((rates > 0.0) & np.isfinite(rates)):
            raise ValueError("bad rates")
    if epochs is not None:
        epochs = np.asarray(epochs, np.int32).reshape(-1, 4).astype(np.int64)
        if epochs.shape[0] != nrec:
            raise ValueError("bad epochs")
    f0p = [FM.period(r) for r in records]
    cap = float(2 * max_period - 4) if max_period > 2 else 1.0

    def rec(tau):
        if nrec == 0:
            return -1
        return min(max((math.floor(tau) - f0_center + f0_hop // 2) // f0_hop, 0), nrec - 1)

    def voiced(tau):
        j = rec(tau)
        return j >= 0 and f0p[j] > 0.0

    def period(tau):
        j = rec(tau)
        q = f0p[j] if j >= 0 else 0.0
        if not q > 0.0:
            return float(unvoiced_period)
        return min(max(q, float(min_period)), float(max_period))

    def ratio(tau):
        j = rec(tau)
        if j < 0 or ratios is None or not f0p[j] > 0.0:
            return 1.0
        return float(ratios[j])

    def rate(tau):
        j = rec(tau)
        if j < 0 or rates is None:
            return 1.0
        return min(max(float(rates[j]), 0.25), 4.0)

    def step(tau):
        return min(period(tau) / ratio(tau), cap)

    def snap(c, prev):
        j = rec(c)
        if epochs is None or j < 0 or not f0p[j] > 0.0 or epochs[j, 1] <= 0 or epochs[j, 3] < min_strength:
            return c
        P = period(c)
        E = float(j * f0_hop + int(epochs[j, 0]))
        s = E + math.floor((c - E) / P + 0.5) * P
        if prev is not None and s - prev < P / 2.0:
            s = s + P
        if prev is not None and voiced(prev) and abs(s - c) <= P / 4.0:
            s = c + lock * (s - c)
        return s

    grains, marks = [], []
    length = float(input_len)
    A = snap(0.0, None) if offset is None else float(offset)
    An = snap(A + period(A), A)
    T = Tprev = 0.0
    V = Vprev = 0.0
    held = None                                                          # (T, A, gap before, V, mirrored)

    def emit(h, gap_after):
        hT, hA, hgap, _, hm = h
        L = math.floor(period(hA) + 0.5)
        L = max(L, math.floor(max(hgap, gap_after) / 2.0) + 2, 2)
        L = min(L, max_period)
        c = math.floor(256.0 * hT + 0.5)
        if (c >> 8) >= MAX_POSITION:
            raise ValueError("the output passes 2^30")
        marks.append((hA, voiced(hA)))
        if hm:
            sq = math.floor(256.0 * (hT + hA) + 0.5)
            D = (sq + 255) >> 8
            if D >= 1 << 31:
                raise ValueError("a mirrored grain's D passes 2^31")
            grains.append([c >> 8, (c & 255) + 256 * (256 * D - sq) + MIRROR, D, L])
        else:
            dq = math.floor(256.0 * (hT - hA) + 0.5)
            grains.append([c >> 8, (c & 255) + 256 * (dq & 255), dq >> 8, L])

    while V < length:
        while abs(An - V) < abs(A - V):
            A = An
            An = snap(A + period(A), A)
        if held is not None and not voiced(V) and not voiced(A) and A < length:
            Tn = A + np.rint((T + (A - V)) - A)
            if A >= Vprev + 1.0 and Tn >= Tprev + 1.0 and Tn - Tprev <= cap:
                T, V = float(Tn), A
        if held is not None:
            emit(held, T - held[0])
        reuse = bool(mirror) and held is not None and held[1] == A and not voiced(A)
        held = (T, A, T - held[0] if held is not None else 0.0, V, reuse and not held[4])
        Tprev, Vprev = T, V
        s = step(V)
        T = T + s
        V = V + rate(V) * s
    output_len = 0
    if held is not None:
        emit(held, T - held[0])
        output_len = math.floor(held[0] + (length - held[3]) / rate(held[3]) + 0.5)
    g = np.array(grains, np.int64).astype(np.int32).reshape(-1, 4)
    if details:
        return g, int(output_len), np.array([a for a, _ in marks], np.float64), np.array([v for _, v in marks], bool)
    return g, int(output_len)


def buzz(y, lo=32, hi=1100, edge=2000):
    """(the largest normalised autocorrelation of y[edge : len - edge] over the lags lo .. hi, its lag, the figure of every lag: r[k - lo] is lag k's)."""
    z = np.asarray(y, np.float64)[edge:len(y) - edge]
    z = z - z.mean()
    e = float(np.dot(z, z))
    r = np.array([np.dot(z[:-k], z[k:]) / e for k in range(lo, hi + 1)])
    k = int(np.argmax(r))
    return float(r[k]), lo + k, r
