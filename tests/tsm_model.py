"""CPU model of time-scale modification on the overlap-add path (Tsm / pv_tsm_*, pv_tsm_plan): plain numpy, fp64.  TEST INFRASTRUCTURE ONLY, and the
normative definition (DESIGN.md "Time-scale modification"); the reference has no counterpart.

A far grain is four int32 {t, w, D, L} with w = tf + 256 phi, tf and phi in 0 .. 255: a Hann window of half length L centred at output position
t + tf / 256; output n of the grain reads the input at the real position n - D - phi / 256.  D is any whole number with |D| < 2^30: it is the
`dq div 256` of tests/psola_model.py and phi its `dq mod 256`, so a grain may read the input far from where it writes.  Window, sample and output
rules are psola_model's word for word (the same Hn and P, phi == 0 reads x[n - D] itself, else theta = 256 - phi, b = n - D - 1 and 64 taps, num and
den in grain order, x is 0 outside [0, nin)): on a table with |256 D + phi| <= 256 max_period, process() here is PM.process after from_psola().
  tiles    a call's outputs [out_first, out_first + nout) go in tiles of 1024, tile k = [j0, j1) from j0 = out_first + 1024 k.  Its grains are the range
           [a, b) of psola's two-pointer walk, and its source range is lo = min (max(j0, t - L) - D - 33), hi = max (min(j1, t + L) - D + 32) over the
           grains of [a, b) with t + L >= j0 and t - L < j1; every tap of a covered output lies in [lo, hi).  The extent hi - lo must not exceed
           span(max_period, max_rate) = max_rate (1024 + 2 max_period) + 4 max_period + 64.
The planner is tests/epoch_model.py epoch_plan with a read position V beside the synthesis position T; with every rate 1 its grains are epoch_plan's."""
import math

import numpy as np

import epoch_model as EM
import f0_model as FM
import psola_model as PM
import vari_model as VM

Q = PM.Q
TAPS = PM.TAPS
TILE = 1024
MAX_PERIOD = PM.MAX_PERIOD
MAX_POSITION = PM.MAX_POSITION
MAX_RATE = 4
LDS_BYTES = 160 * 1024


def span(max_period, max_rate):
    """Samples a tile may stage."""
    return max_rate * (TILE + 2 * max_period) + 4 * max_period + TAPS


def lds_bytes(max_period, max_rate):
    """Dynamic LDS of a launch: the padded span, P and Hn."""
    s = span(max_period, max_rate)
    return 4 * (((s + (s >> 6) + 4) & ~3) + ((VM.prototype().size + 3) & ~3) + ((PM.WINDOW + 3) & ~3))


def from_psola(grains):
    """psola grains {t, tf, dq, L} -> far grains {t, tf + 256 (dq mod 256), dq div 256, L}."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    return np.stack([g[:, 0], g[:, 1] + Q * (g[:, 2] & (Q - 1)), g[:, 2] >> 8, g[:, 3]], axis=1).astype(np.int32).reshape(-1, 4)


def is_near(grains, max_period):
    """Whether every grain satisfies |256 D + phi| <= 256 max_period: then to_psola() gives pv_psola_process's table."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    return bool(np.all(np.abs(Q * g[:, 2] + (g[:, 1] >> 8)) <= Q * max_period))


def to_psola(grains):
    """Far grains -> psola grains {t, tf, 256 D + phi, L} (meaningful for a near table)."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    return np.stack([g[:, 0], g[:, 1] & (Q - 1), Q * g[:, 2] + (g[:, 1] >> 8), g[:, 3]], axis=1).astype(np.int32).reshape(-1, 4)


def check_grains(grains, max_period):
    """None when the table is well formed, else (index of the first bad grain, why): PM.check_grains in the far notation."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    prev = 0
    for k, (t, w, D, L) in enumerate(g.tolist()):
        if not (0 <= t < MAX_POSITION and 0 <= w < Q * Q):
            return k, "centre"
        if not 2 <= L <= max_period:
            return k, "half length"
        if abs(D) >= MAX_POSITION:
            return k, "shift"
        if t * Q + (w & (Q - 1)) < prev:
            return k, "out of order"
        prev = t * Q + (w & (Q - 1))
    return None


def tiles(grains, max_period, out_first, nout):
    """int64[ntiles, 4] {g_first, g_end, src0, src_count} of the call's tiles, as the host uploads them (src_count = hi - lo, 0 for a tile without grains)."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    ng = g.shape[0]
    t, D, L = g[:, 0], g[:, 2], g[:, 3]
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
            s0 = int(np.min((np.maximum(j0, t[s] - L[s]) - D[s] - 33)[reach]))
            s1 = int(np.max((np.minimum(j1, t[s] + L[s]) - D[s] + 32)[reach]))
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
    """x: float32[nch, nin], far grains int[ngrains, 4] -> fp64[nch, nout], outputs out_first .. out_first + nout - 1.  PM.process operation for
    operation (so that a near table gives its bits), with the input gathered at any distance.  bound=True returns (y, tol, poisoned) as PM.process does:
    the derived bound of tests/test_gpu_psola.py holds for this arithmetic unchanged, since D enters the addresses only.  subnormal="derived" replaces
    the last term of tol, 2^-149 (1 + (G + 67) / D), by 2^-150 ((Z + G) / D + 2), Z = sum |h_g| (64 / |d_g| + 1) over the fractional grains, and returns
    (y, tol, poisoned, G, den): PM.process derives it (every rounding in the subnormal range is within 2^-150 absolute; 64 fused multiply-adds and a division
    per fractional grain, G fused multiply-adds into the numerator, the final division, one unit for the second order).  The default stays bit for bit."""
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
        tf, phi = w_ & (Q - 1), w_ >> 8
        lo, hi = max(t - L + 1, out_first), min(t + L, out_first + nout - 1)
        if lo > hi:
            continue
        n = np.arange(lo, hi + 1, dtype=np.int64)
        h, fd, nz = PM.grain_weights(n, t, tf, L, Hn)
        if not nz.any():
            continue
        n, h, fd = n[nz], h[nz], fd[nz]
        sl = n - out_first
        if phi == 0:
            xt, hit = gather(n - D)
            e = np.zeros_like(xt)
        else:
            w = P[np.abs(Q * (i - (TAPS // 2 - 1)) - (Q - phi))]
            xv, hits = gather((n - D - 1 - (TAPS // 2 - 1))[:, None] + i[None, :])      # [nch, len, 64]
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

def tsm_plan(records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios=None, rates=None, epochs=None, min_strength=0,
             lock=EM.DEFAULT_LOCK, offset=None):
    """(int32[ngrains, 4] far grains, output_len) of pv_tsm_plan: EM.epoch_plan with a read position V beside the synthesis position T.  rates:
    float64[nrec], the input samples consumed per output sample while V lies on record j (finite and positive, held within [1/4, 4]; None: 1).
    offset: the first analysis mark in place of snap(0, none) (the envelope tests put it on a pulse; the C planner has none)."""
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

    grains = []
    length = float(input_len)
    A = snap(0.0, None) if offset is None else float(offset)
    An = snap(A + period(A), A)
    T = Tprev = 0.0
    V = Vprev = 0.0
    held = None                                                          # (T, A, gap before, V)

    def emit(h, gap_after):
        hT, hA, hgap, _ = h
        L = math.floor(period(hA) + 0.5)
        L = max(L, math.floor(max(hgap, gap_after) / 2.0) + 2, 2)
        L = min(L, max_period)
        c = math.floor(256.0 * hT + 0.5)
        dq = math.floor(256.0 * (hT - hA) + 0.5)
        if (c >> 8) >= MAX_POSITION:
            raise ValueError("the output passes 2^30")
        grains.append([c >> 8, (c & 255) + 256 * (dq & 255), dq >> 8, L])

    while V < length:
        while abs(An - V) < abs(A - V):
            A = An
            An = snap(A + period(A), A)
        # unvoiced material passes at whole-sample shifts: the read position goes onto the analysis mark and the synthesis mark moves with it,
        # rounded to a whole distance from the mark; never unless the read position gets at least one sample past the mark before it
        if held is not None and not voiced(V) and not voiced(A) and A < length:
            Tn = A + np.rint((T + (A - V)) - A)
            if A >= Vprev + 1.0 and Tn >= Tprev + 1.0 and Tn - Tprev <= cap:
                T, V = float(Tn), A
        if held is not None:
            emit(held, T - held[0])
        held = (T, A, T - held[0] if held is not None else 0.0, V)
        Tprev, Vprev = T, V
        s = step(V)
        T = T + s
        V = V + rate(V) * s
    output_len = 0
    if held is not None:
        emit(held, T - held[0])
        output_len = math.floor(held[0] + (length - held[3]) / rate(held[3]) + 0.5)
    return np.array(grains, np.int32).reshape(-1, 4), int(output_len)
