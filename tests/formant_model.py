"""CPU model of warped grains on the overlap-add path (Formant / pv_formant_*, pv_formant_plan): plain numpy, fp64.  TEST INFRASTRUCTURE ONLY, and the
normative definition (DESIGN.md "Formant shifting"); the reference has no counterpart.

A grain is four int32 {t, w, D, L} with w = tf + 256 phi + 131072 z, tf and phi in 0 .. 255, bit 16 zero.  z, bits 17 .. 26, is the step s in 1/256:
z = 0 means s = 256, else 128 <= z <= 512 and s = z; z = 256 is treated exactly as z = 0.  With s = 256 the grain is the far grain of tests/tsm_model.py
word for word.  With s != 256 it is WARPED: output n reads the input at the real position (t + tf / 256 - D - phi / 256) + (s / 256) (n - t - tf / 256).
In exact integers: u = 256 (n - t) - tf, v = 256 (tf - phi) + s u, m = (t - D) + floor(v / 65536), r = v mod 65536; den = max(256, s), W = 32 for
s <= 256 and 64 otherwise; tap i = 0 .. 2 W - 1 reads x[m - W + 1 + i] with d = |(i - W + 1) 65536 - r|, q = d div den, rem = d mod den, w_i = 0 when
q >= 8192, else P[q] + (rem / den) (P[q + 1] - P[q]); a = fmaf(w_i, x_i, a) and sum += w_i for i ascending, xt = a / sum; a tap whose weight is exactly
0 (in the kernel's f32 arithmetic, as tests/vari_model.py nonzero_weights) touches neither sum whatever its sample holds.  Window and output rules do not
change.
  check    0 <= t < 2^30 ("centre"); 0 <= w < 2^27, bit 16 zero, z = 0 or 128 <= z <= 512 ("step"); the rest is tsm_model.check_grains.
  tiles    the grain range [a, b) of a tile is tsm_model's walk (t and L only).  An unwarped grain's source range is tsm_model's; a warped grain that
           reaches the tile [j0, j1) has lo = M(max(j0, t - L)) - W - 1 and hi = M(min(j1, t + L)) + W + 1, M(n) the m of output n.  src0 = min lo,
           src_count = max hi - min lo over both kinds; every tap of a covered output lies in [lo + 1, hi - 1].
  span     max_rate (1024 + 2 max_period) + 6 max_period + 192.
The planner is tsm_model.tsm_plan with one more row, warps: a step per f0 record."""
import math

import numpy as np

import epoch_model as EM
import f0_model as FM
import psola_model as PM
import tsm_model as TM
import vari_model as VM

Q = TM.Q
TAPS = TM.TAPS
WARPED_TAPS = 128
TILE = TM.TILE
MAX_PERIOD = TM.MAX_PERIOD
MAX_POSITION = TM.MAX_POSITION
LDS_BYTES = TM.LDS_BYTES
MIRROR = Q * Q                                                             # bit 16 of w: must be 0
STEP = 1 << 17                                                             # z = w div 131072
W_END = 1 << 27
MIN_STEP, MAX_STEP = 128, 512
ONE = 1 << 16                                                              # positions per sample on the warped side


def span(max_period, max_rate):
    """Samples a tile may stage."""
    return max_rate * (TILE + 2 * max_period) + 6 * max_period + 192


def lds_bytes(max_period, max_rate):
    """Dynamic LDS of a launch: the padded span, P and Hn."""
    s = span(max_period, max_rate)
    return 4 * (((s + (s >> 6) + 4) & ~3) + ((VM.prototype().size + 3) & ~3) + ((PM.WINDOW + 3) & ~3))


def fits(max_period, max_rate):
    """Whether pv_formant_create accepts the pair (the LDS rule)."""
    return lds_bytes(max_period, max_rate) <= LDS_BYTES


def steps(grains):
    """int64[ngrains]: the step s of every grain (256 for z = 0)."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    z = (g[:, 1] >> 17) & 1023
    return np.where(z == 0, Q, z)


def warped(grains):
    """bool[ngrains]: s != 256."""
    return steps(grains) != Q


def check_grains(grains, max_period):
    """None when the table is well formed, else (index of the first bad grain, why)."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    prev = 0
    for k, (t, w, D, L) in enumerate(g.tolist()):
        if not 0 <= t < MAX_POSITION:
            return k, "centre"
        z = w >> 17
        if not 0 <= w < W_END or w & MIRROR or (z != 0 and not MIN_STEP <= z <= MAX_STEP):
            return k, "step"
        if not 2 <= L <= max_period:
            return k, "half length"
        if abs(D) >= MAX_POSITION:
            return k, "shift"
        if t * Q + (w & (Q - 1)) < prev:
            return k, "out of order"
        prev = t * Q + (w & (Q - 1))
    return None


def _m(t, tf, phi, D, s, n):
    """(m, r) of output n of a warped grain: the read position is m + r / 65536."""
    v = Q * (tf - phi) + s * (Q * (n - t) - tf)
    return (t - D) + (v >> 16), v & (ONE - 1)


def tiles(grains, max_period, out_first, nout):
    """int64[ntiles, 4] {g_first, g_end, src0, src_count} of the call's tiles (src_count = hi - lo, 0 for a tile without grains)."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    ng = g.shape[0]
    t, D, L = g[:, 0], g[:, 2], g[:, 3]
    tf, phi, s = g[:, 1] & (Q - 1), (g[:, 1] >> 8) & (Q - 1), steps(g)
    W = np.where(s < Q, TAPS // 2, WARPED_TAPS // 2)
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
        c = slice(a, b)
        reach = (t[c] + L[c] >= j0) & (t[c] - L[c] < j1)
        if reach.any():
            first, last = np.maximum(j0, t[c] - L[c]), np.minimum(j1, t[c] + L[c])
            from_ = np.where(s[c] == Q, first - D[c] - 33, _m(t[c], tf[c], phi[c], D[c], s[c], first)[0] - W[c] - 1)
            to = np.where(s[c] == Q, last - D[c] + 32, _m(t[c], tf[c], phi[c], D[c], s[c], last)[0] + W[c] + 1)
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


def warped_weights(s, r, P32):
    """For the fractions r (int64[len]) of a grain of step s: (w fp64[len, 2 W], |f d| fp64, nonzero bool, W).  `nonzero` is w != 0 IN THE KERNEL'S ARITHMETIC,
    w = fmaf(f32(rem) * (1.0f / f32(den)), P[q + 1] - P[q], P[q]), evaluated in fp64 from the f32 operands as VM.nonzero_weights does."""
    den = max(Q, s)
    W = TAPS // 2 if s < Q else WARPED_TAPS // 2
    i = np.arange(2 * W, dtype=np.int64)[None, :]
    d = np.abs((i - W + 1) * ONE - np.asarray(r, np.int64)[:, None])
    q = np.minimum(d // den, VM.HALF_WIDTH * Q)
    rem = d % den
    P = P32.astype(np.float64)
    dP = P[q + 1] - P[q]
    f = rem.astype(np.float64) / den
    w = P[q] + f * dP
    f32 = rem.astype(np.float32) * (np.float32(1.0) / np.float32(den))
    d32 = P32[q + 1] - P32[q]
    assert f32.dtype == np.float32 and d32.dtype == np.float32
    nz = f32.astype(np.float64) * d32.astype(np.float64) + P[q] != 0.0
    return np.where(nz, w, 0.0), np.where(nz, np.abs(f * dP), 0.0), nz, W


def process(x, grains, out_first=0, nout=None, ptable=None, htable=None, bound=False, subnormal=None):
    """x: float32[nch, nin], grains int[ngrains, 4] -> fp64[nch, nout], outputs out_first .. out_first + nout - 1.  TM.process operation for operation
    (a table with no warped grain gives its bits), with the sample of a warped grain formed by the rule above.  bound=True returns (y, tol, poisoned) as
    TM.process does.  The derived bound of tests/test_gpu_psola.py holds with one term changed, the error e_g of a grain's sample: for a warped grain
    the weights are interpolated (three roundings on f d and one on the result: |w^ - w| <= 3 u m, m = |w| + |f d|, tests/test_gpu_vari.py), and Tloc <= 128
    non-zero taps go into each accumulator, so |xt^ - xt| <= e_g = u [(Tloc + 3) (a_g + |xt| s_g) / |d_g| + |xt|] with a_g = sum m |x|, s_g = sum m,
    d_g = sum w (tests/test_gpu_formant.py states it).  subnormal="derived" as TM.process, with Tloc in the place of 64."""
    x = np.asarray(x, np.float32)
    if x.ndim == 1:
        x = x[None, :]
    nch, nin = x.shape
    nout = nin - out_first if nout is None else nout
    P32 = VM.prototype() if ptable is None else np.asarray(ptable, np.float32)
    P = P32.astype(np.float64)
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
    Z = np.zeros(nout)                                                    # sum |h_g| (Tloc / |d_g| + 1) over the fractional and the warped grains
    poisoned = np.zeros((nch, nout), bool)
    u = 2.0 ** -24
    i = np.arange(TAPS, dtype=np.int64)
    most = TAPS                                                            # the most taps of any grain of the table
    for t, w_, D, L in g.tolist():
        tf, phi, z = w_ & (Q - 1), (w_ >> 8) & (Q - 1), w_ >> 17
        s = Q if z == 0 else z
        lo, hi = max(t - L + 1, out_first), min(t + L, out_first + nout - 1)
        if lo > hi:
            continue
        n = np.arange(lo, hi + 1, dtype=np.int64)
        h, fd, nz = PM.grain_weights(n, t, tf, L, Hn)
        if not nz.any():
            continue
        n, h, fd = n[nz], h[nz], fd[nz]
        sl = n - out_first
        zterm = None
        if s != Q:
            m, r = _m(t, tf, phi, D, s, n)
            w, wfd, wnz, W = warped_weights(s, r, P32)
            most = max(most, 2 * W)
            xv, hits = gather((m - W + 1)[:, None] + np.arange(2 * W, dtype=np.int64)[None, :])       # [nch, len, 2 W]
            Dg = w.sum(axis=1)                                                                         # per output: every lane has its own weights
            xt = (xv * w).sum(axis=2) / Dg
            mw = np.abs(w) + wfd
            Tloc = wnz.sum(axis=1)
            e = u * ((Tloc + 3) * ((np.abs(xv) * mw).sum(axis=2) + np.abs(xt) * mw.sum(axis=1)) / np.abs(Dg) + np.abs(xt))
            hit = (hits & wnz[None, :, :]).any(axis=2)
            zterm = np.abs(h) * ((Tloc + 3) / np.abs(Dg) + 1.0)
        elif phi == 0:
            xt, hit = gather(n - D)
            e = np.zeros_like(xt)
        else:
            w = P[np.abs(Q * (i - (TAPS // 2 - 1)) - (Q - phi))]
            xv, hits = gather((n - D - 1 - (TAPS // 2 - 1))[:, None] + i[None, :])      # [nch, len, 64]
            Dg = w.sum()
            xt = (xv * w).sum(axis=2) / Dg
            e = u * (TAPS * ((np.abs(xv) * np.abs(w)).sum(axis=2) + np.abs(xt) * np.abs(w).sum()) / abs(Dg) + np.abs(xt))
            hit = hits.any(axis=2)
            zterm = np.abs(h) * (TAPS / abs(Dg) + 1.0)
        mm = np.abs(h) + fd
        num[:, sl] += h * xt
        den[sl] += h
        A[:, sl] += mm * np.abs(xt)
        S[sl] += mm
        E[:, sl] += np.abs(h) * e
        if zterm is not None:
            Z[sl] += zterm
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
        tol[:, cov] = rel + 2.0 ** -149 * (1.0 + (Gc + most) / den[cov])
        return y, tol, poisoned
    if subnormal != "derived":
        raise ValueError("subnormal: None or 'derived'")
    tol[:, cov] = rel + 2.0 ** -150 * ((Z[cov] + G[cov]) / den[cov] + 2.0)
    return y, tol, poisoned, G, den


# ---- the planner ------------------------------------------------------------------------------------------------------------------------------

def formant_plan(records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios=None, rates=None, warps=None, epochs=None,
                 min_strength=0, lock=EM.DEFAULT_LOCK, offset=None):
    """(int32[ngrains, 4] grains, output_len) of pv_formant_plan: TM.tsm_plan, restated here statement for statement, with a step per grain.
    warps=None: tsm_plan's grains bit for bit.  Else float64[nrec] within [1/2, 2]: the grain held for the analysis mark A takes alpha = warps[rec(A)],
    voiced or not; s = floor(256 alpha + 1/2), z = 0 when s == 256 and s otherwise, and its half length starts from floor(period(A) / (s / 256.0) + 1/2)
    in place of floor(period(A) + 1/2); tsm_plan's floors then apply unchanged.  Marks, read position, D, phi and output_len do not depend on warps."""
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
    if warps is not None:
        warps = np.asarray(warps, np.float64)
        if warps.shape != (nrec,) or not np.all((warps >= 0.5) & (warps <= 2.0)):
            raise ValueError("bad warps")
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

    def warp(tau):
        j = rec(tau)
        if j < 0 or warps is None:
            return Q
        return math.floor(256.0 * float(warps[j]) + 0.5)

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
        s = warp(hA)
        L = math.floor(period(hA) / (s / 256.0) + 0.5)
        L = max(L, math.floor(max(hgap, gap_after) / 2.0) + 2, 2)
        L = min(L, max_period)
        c = math.floor(256.0 * hT + 0.5)
        dq = math.floor(256.0 * (hT - hA) + 0.5)
        if (c >> 8) >= MAX_POSITION:
            raise ValueError("the output passes 2^30")
        grains.append([c >> 8, (c & 255) + 256 * (dq & 255) + (0 if s == Q else STEP * s), dq >> 8, L])

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
        held = (T, A, T - held[0] if held is not None else 0.0, V)
        Tprev, Vprev = T, V
        s = step(V)
        T = T + s
        V = V + rate(V) * s
    output_len = 0
    if held is not None:
        emit(held, T - held[0])
        output_len = math.floor(held[0] + (length - held[3]) / rate(held[3]) + 0.5)
    return np.array(grains, np.int64).astype(np.int32).reshape(-1, 4), int(output_len)
