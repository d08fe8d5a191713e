"""CPU model of full-grain harmony voices on the overlap-add path (Choir / pv_choir_*, pv_choir_plan): plain numpy, fp64.  TEST INFRASTRUCTURE ONLY, and
the normative definition (DESIGN.md "Choir"); the reference has no counterpart.

A grain is four int32 {t, w, D, L} with w = tf + 256 phi + 65536 m + 131072 z, 0 <= w < 2^27, tf and phi in 0 .. 255.  m is the direction bit of
tests/mirror_model.py, z the step of tests/formant_model.py (z = 0 means s = 256, else 128 <= z <= 512 and s = z; z = 256 is treated exactly as z = 0).
  m = 0, s = 256   the far grain of tests/tsm_model.py, word for word.
  m = 1, s = 256   the mirrored grain of tests/mirror_model.py, word for word: output n reads D - n - phi / 256.
  m = 0, s != 256  the warped grain of tests/formant_model.py, word for word.
  m = 1, s != 256  MIRRORED AND WARPED: output n reads the real position (D - t - tf / 256 - phi / 256) - (s / 256) (n - t - tf / 256).  In exact integers:
                   u = 256 (n - t) - tf, v = -256 (tf + phi) - s u, mm = (D - t) + floor(v / 65536), r = v mod 65536; from (mm, r) on the sample rule is
                   formant_model's, unchanged: den = max(256, s), W = 32 for s <= 256 and 64 otherwise, tap i = 0 .. 2 W - 1 reads x[mm - W + 1 + i] with
                   d = |(i - W + 1) 65536 - r| and the interpolated weight of that model; i ascending; a zero weight touches neither sum.
  check    0 <= t < 2^30 ("centre"); 0 <= w < 2^27 and z = 0 or 128 <= z <= 512 ("step"); 2 <= L <= max_period ("half length"); D > -2^30 always and
           D < 2^30 for a forward grain ("shift"); centres non-decreasing on 256 t + tf ("out of order").
  tiles    per voice the grain range [a, b) of a tile is tsm_model's walk (t and L only).  With first = max(j0, t - L) and last = min(j1, t + L) the source
           range of a grain that reaches the tile [j0, j1) is tsm_model's, mirror_model's or formant_model's for the first three kinds, and
           lo = M'(last) - W - 1, hi = M'(first) + W + 1 for a mirrored warped one, M'(n) the mm of output n (it does not increase with n): every tap of a
           covered output lies in [lo + 2, hi - 1].  A call stages the hull over the voices, as tests/harmony_model.py.
  span     formant_model's: max_rate (1024 + 2 max_period) + 6 max_period + 192, with its LDS rule.
  mix      harmony_model's float32 fold, word for word, on the per-voice outputs.
The planner is mirror_model.mirror_plan with formant_model.formant_plan's row warps."""
import math

import numpy as np

import epoch_model as EM
import f0_model as FM
import formant_model as FoM
import harmony_model as HM
import psola_model as PM
import tsm_model as TM
import vari_model as VM

Q = TM.Q
TAPS = TM.TAPS
WARPED_TAPS = FoM.WARPED_TAPS
TILE = TM.TILE
MAX_PERIOD = TM.MAX_PERIOD
MAX_POSITION = TM.MAX_POSITION
MAX_VOICES = HM.MAX_VOICES
MIRROR = Q * Q                                                             # bit 16 of w
STEP = 1 << 17                                                             # z = w div 131072
W_END = 1 << 27
MIN_STEP, MAX_STEP = 128, 512
ONE = 1 << 16                                                              # positions per sample on the warped side
span = FoM.span
lds_bytes = FoM.lds_bytes
fits = FoM.fits
mix = HM.mix


def steps(grains):
    """int64[ngrains]: the step s of every grain (256 for z = 0)."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    z = (g[:, 1] >> 17) & 1023
    return np.where(z == 0, Q, z)


def warped(grains):
    """bool[ngrains]: s != 256."""
    return steps(grains) != Q


def mirrored(grains):
    """bool[ngrains]: bit 16 of w."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    return (g[:, 1] & MIRROR) != 0


def check_grains(grains, max_period):
    """None when ONE voice's table is well formed, else (index of the first bad grain, why)."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    prev = 0
    for k, (t, w, D, L) in enumerate(g.tolist()):
        if not 0 <= t < MAX_POSITION:
            return k, "centre"
        z = w >> 17
        if not 0 <= w < W_END or (z != 0 and not MIN_STEP <= z <= MAX_STEP):
            return k, "step"
        if not 2 <= L <= max_period:
            return k, "half length"
        if (D <= -MAX_POSITION or D >= 1 << 31) if w & MIRROR else abs(D) >= MAX_POSITION:
            return k, "shift"
        if t * Q + (w & (Q - 1)) < prev:
            return k, "out of order"
        prev = t * Q + (w & (Q - 1))
    return None


def check_voices(tables, max_period):
    """None when every voice's table is well formed, else (voice, index of its first bad grain, why)."""
    for v, t in enumerate(tables):
        bad = check_grains(t, max_period)
        if bad is not None:
            return (v,) + bad
    return None


def _m(t, tf, phi, D, s, mir, n):
    """(m, r) of output n of a warped grain, forward (formant_model's) or mirrored (mm of the contract): the read position is m + r / 65536."""
    su = s * (Q * (n - t) - tf)
    v = np.where(mir, -Q * (tf + phi) - su, Q * (tf - phi) + su)
    return np.where(mir, D - t, t - D) + (v >> 16), v & (ONE - 1)


def tiles(grains, max_period, out_first, nout):
    """int64[ntiles, 4] {g_first, g_end, src0, src_count} of the tiles of ONE voice's table (src_count = hi - lo, 0 for a tile without grains)."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    ng = g.shape[0]
    t, D, L = g[:, 0], g[:, 2], g[:, 3]
    tf, phi, s, mir = g[:, 1] & (Q - 1), (g[:, 1] >> 8) & (Q - 1), steps(g), mirrored(g)
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
            low, high = np.where(mir[c], last, first), np.where(mir[c], first, last)      # the output that reads lowest, and the one that reads highest
            plain_from = np.where(mir[c], D[c] - last, first - D[c]) - 33
            plain_to = np.where(mir[c], D[c] - first, last - D[c]) + 32
            from_ = np.where(s[c] == Q, plain_from, _m(t[c], tf[c], phi[c], D[c], s[c], mir[c], low)[0] - W[c] - 1)
            to = np.where(s[c] == Q, plain_to, _m(t[c], tf[c], phi[c], D[c], s[c], mir[c], high)[0] + W[c] + 1)
            s0, s1 = int(np.min(from_[reach])), int(np.max(to[reach]))
            out.append([a, b, s0, s1 - s0])
        else:
            out.append([a, b, 0, 0])
    return np.array(out, np.int64).reshape(-1, 4)


def hull(tables, max_period, out_first, nout):
    """(hull int64[ntiles, 2] {src0, src_count}, ranges int64[ntiles, V, 2] {g_first, g_end} as indices into the concatenated table) as the host uploads
    them: tiles() per voice, and the hull over the voices with a grain on the tile ({0, 0} when none has one).  harmony_model.tiles with full grains."""
    per = [tiles(t, max_period, out_first, nout) for t in tables]
    first = np.concatenate([[0], np.cumsum([np.asarray(t).reshape(-1, 4).shape[0] for t in tables])])
    ntiles = per[0].shape[0]
    out = np.zeros((ntiles, 2), np.int64)
    ranges = np.zeros((ntiles, len(tables), 2), np.int64)
    for k in range(ntiles):
        live = [p[k] for p in per if p[k, 3] > 0]
        if live:
            lo = min(int(p[2]) for p in live)
            hi = max(int(p[2] + p[3]) for p in live)
            out[k] = [lo, hi - lo]
        for v, p in enumerate(per):
            ranges[k, v] = [first[v] + p[k, 0], first[v] + p[k, 1]]
    return out, ranges


def check_span(tables, max_period, max_rate, out_first, nout):
    """None when the hull of every tile of the call fits the span, else (tile, lowest voice with a grain on it, that voice's first grain of the tile counted
    within the voice, the hull's extent)."""
    cap = span(max_period, max_rate)
    per = [tiles(t, max_period, out_first, nout) for t in tables]
    for k, (_, cnt) in enumerate(hull(tables, max_period, out_first, nout)[0].tolist()):
        if cnt > cap:
            for v, p in enumerate(per):
                if p[k, 3] > 0:
                    return k, v, int(p[k, 0]), cnt
    return None


def voice(x, grains, out_first=0, nout=None, ptable=None, htable=None, bound=False, subnormal=None):
    """One voice.  x: float32[nch, nin], grains int[ngrains, 4] -> fp64[nch, nout], outputs out_first .. out_first + nout - 1: formant_model.process operation
    for operation (a table without mirrored grains gives its bits, one without warped grains mirror_model.process's), with the whole part of the read
    position running downwards under a mirrored grain.  bound=True returns (y, tol, poisoned) as those do; the derived bound is formant_model's, since the
    direction enters the addresses and the fraction r only, never the way a value is rounded.  subnormal="derived" as there."""
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
        tf, phi, mir, z = w_ & (Q - 1), (w_ >> 8) & (Q - 1), (w_ >> 16) & 1, w_ >> 17
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
            m, r = _m(t, tf, phi, D, s, bool(mir), n)
            w, wfd, wnz, W = FoM.warped_weights(s, r, P32)
            most = max(most, 2 * W)
            xv, hits = gather((m - W + 1)[:, None] + np.arange(2 * W, dtype=np.int64)[None, :])       # [nch, len, 2 W]
            Dg = w.sum(axis=1)                                                                         # per output: every lane has its own weights
            xt = (xv * w).sum(axis=2) / Dg
            mw = np.abs(w) + wfd
            Tloc = wnz.sum(axis=1)
            e = u * ((Tloc + 3) * ((np.abs(xv) * mw).sum(axis=2) + np.abs(xt) * mw.sum(axis=1)) / np.abs(Dg) + np.abs(xt))
            hit = (hits & wnz[None, :, :]).any(axis=2)
            zterm = np.abs(h) * ((Tloc + 3) / np.abs(Dg) + 1.0)
        else:
            at = D - n if mir else n - D                                    # the whole part of the read position: the only place the direction enters
            if phi == 0:
                xt, hit = gather(at)
                e = np.zeros_like(xt)
            else:
                w = P[np.abs(Q * (i - (TAPS // 2 - 1)) - (Q - phi))]
                xv, hits = gather((at - 1 - (TAPS // 2 - 1))[:, None] + i[None, :])     # [nch, len, 64]
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


def process(x, tables, gains, out_first=0, nout=None, ptable=None, htable=None, bound=False, outs=None):
    """x: float32[nch, nin], tables: a list of grain tables, gains [V] or [V, nch] -> float32[nch, nout]: harmony_model.process, word for word, on voice()
    in the place of tsm_model.process (per voice in fp64, rounded to float32, then mix()).  bound=True returns (y fp64, tol, poisoned) with harmony_model's
    fold bound on voice()'s derived bounds.  outs: the list of voice(x, table_v, ..., bound=True), when the caller has it already."""
    x = np.asarray(x, np.float32)
    if x.ndim == 1:
        x = x[None, :]
    nch, nin = x.shape
    nout = nin - out_first if nout is None else nout
    nv = len(tables)
    if not 1 <= nv <= MAX_VOICES:
        raise ValueError("1 to 8 voices")
    g = HM._gains(gains, nv, nch)
    if outs is None:
        outs = [voice(x, t, out_first, nout, ptable, htable, bound=True) for t in tables]
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


# ---- the planner ------------------------------------------------------------------------------------------------------------------------------

def choir_plan(records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios=None, rates=None, warps=None, epochs=None,
               min_strength=0, lock=EM.DEFAULT_LOCK, mirror=True, offset=None, details=False):
    """(int32[ngrains, 4] grains, output_len) of pv_choir_plan: mirror_model.mirror_plan, restated here statement for statement, with
    formant_model.formant_plan's row warps.  warps=None: mirror_plan's grains bit for bit; mirror=False: formant_plan's.  With both, the grain held for the
    analysis mark A takes s = floor(256 warps[rec(A)] + 1/2), z = 0 when s == 256 and s otherwise, and its half length starts from
    floor(period(A) / (s / 256.0) + 1/2); the direction, D and phi of a reuse are mirror_plan's, so a mirrored warped grain reads A at its centre and
    (s / 256) L either side of it.  details=True returns also, per grain, its analysis mark A (float64) and whether the record at A is voiced."""
    records = np.asarray(records, np.int32).reshape(-1, 4)
    nrec = records.shape[0]
    if (f0_hop < 1 or min_period < 2 or max_period < min_period or max_period > MAX_PERIOD or not min_period <= unvoiced_period <= max_period
            or not 0 <= input_len < MAX_POSITION or not 0.0 < lock <= 1.0 or not 0 <= min_strength <= EM.S_ONE):
        raise ValueError("bad argument")
    if mirror not in (0, 1, False, True):
        raise ValueError("bad mirror")
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

    grains, marks = [], []
    length = float(input_len)
    A = snap(0.0, None) if offset is None else float(offset)
    An = snap(A + period(A), A)
    T = Tprev = 0.0
    V = Vprev = 0.0
    held = None                                                          # (T, A, gap before, V, mirrored)

    def emit(h, gap_after):
        hT, hA, hgap, _, hm = h
        s = warp(hA)
        L = math.floor(period(hA) / (s / 256.0) + 0.5)
        L = max(L, math.floor(max(hgap, gap_after) / 2.0) + 2, 2)
        L = min(L, max_period)
        c = math.floor(256.0 * hT + 0.5)
        if (c >> 8) >= MAX_POSITION:
            raise ValueError("the output passes 2^30")
        marks.append((hA, voiced(hA)))
        zz = 0 if s == Q else STEP * s
        if hm:
            sq = math.floor(256.0 * (hT + hA) + 0.5)
            D = (sq + 255) >> 8
            if D >= 1 << 31:
                raise ValueError("a mirrored grain's D passes 2^31")
            grains.append([c >> 8, (c & 255) + 256 * (256 * D - sq) + MIRROR + zz, D, L])
        else:
            dq = math.floor(256.0 * (hT - hA) + 0.5)
            grains.append([c >> 8, (c & 255) + 256 * (dq & 255) + zz, dq >> 8, L])

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
