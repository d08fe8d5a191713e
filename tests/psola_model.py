"""CPU model of the pitch-synchronous overlap-add path (Psola / pv_psola_*, pv_psola_plan, pv_psola_ratios): plain numpy, fp64.  TEST INFRASTRUCTURE
ONLY, and the normative definition (DESIGN.md "Pitch-synchronous correction"); the reference has no counterpart, it is a pitch shifter only.

A grain is four int32 {t, tf, dq, L}: a Hann window of half length L centred at output position t + tf / 256 over the input shifted by dq / 256
samples.  For output n and grain g, Q = 256:
  window   ua = |256 (n - t) - tf|; weight 0 when ua >= 256 L; else q = (4 ua) div L, rem = (4 ua) mod L, f = rem / L,
           h = Hn[q] + f (Hn[q + 1] - Hn[q]); Hn[q] = f32((1 + cos(pi q / 1024)) / 2), q = 0 .. 1023, Hn[1024] = Hn[1025] = 0;
  sample   D = dq div 256, phi = dq mod 256 (floored).  phi == 0: xt = x[n - D].  Else theta = 256 - phi, b = n - D - 1, taps i = 0 .. 63 read
           x[b - 31 + i] with weight w_i = P[|256 (i - 31) - theta|] (P: the prototype of tests/vari_model.py, entries as they are),
           xt = (sum w_i x_i) / (sum w_i); x is 0 outside [0, nin);
  output   y[n] = (sum_g h_g xt_g) / (sum_g h_g) over the grains with h != 0, 0 where there is none.
The model forms weights and sums in fp64 from the f32 tables (the integers are exact either way); the kernel's f32 roundings are what the GPU
tests bound.  The planner and the ratios are exact restatements: the C code is compared with `==`."""
import math

import numpy as np

import f0_model as FM
import vari_model as VM

Q = 256
TAPS = 64
WINDOW = 1026
MAX_PERIOD = 4096
MAX_POSITION = 1 << 30


def window():
    """Hn f32[1026]."""
    H = np.zeros(WINDOW, np.float32)
    H[:1024] = (0.5 * (1.0 + np.cos(np.pi * np.arange(1024) / 1024.0))).astype(np.float32)
    return H


def check_grains(grains, max_period):
    """None when pv_psola_process accepts the table, else (index of the first bad grain, why)."""
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    prev = 0
    for k, (t, tf, dq, L) in enumerate(g.tolist()):
        if not (0 <= t < MAX_POSITION and 0 <= tf < Q):
            return k, "centre"
        if not 2 <= L <= max_period:
            return k, "half length"
        if abs(dq) > Q * max_period:
            return k, "shift"
        if t * Q + tf < prev:
            return k, "out of order"
        prev = t * Q + tf
    return None


def grain_weights(n, t, tf, L, Hn):
    """For int64 outputs n: (h fp64, |f d| fp64, nonzero bool) of one grain.  `nonzero` is h != 0 IN THE KERNEL'S ARITHMETIC,
    h = fmaf(f32(rem) * (1.0f / f32(L)), Hn[q + 1] - Hn[q], Hn[q]), evaluated in fp64 from the f32 operands as tests/vari_model.py nonzero_weights does."""
    ua = np.abs(Q * (n - t) - tf)
    inside = ua < Q * L
    u4 = np.where(inside, 4 * ua, 0)
    q = np.minimum(u4 // L, 1024)
    rem = u4 % L
    H64 = Hn.astype(np.float64)
    d = H64[q + 1] - H64[q]
    f = rem.astype(np.float64) / L
    h = np.where(inside, H64[q] + f * d, 0.0)
    f32 = rem.astype(np.float32) * (np.float32(1.0) / np.float32(L))
    d32 = Hn[q + 1] - Hn[q]
    assert f32.dtype == np.float32 and d32.dtype == np.float32
    nz = inside & (f32.astype(np.float64) * d32.astype(np.float64) + H64[q] != 0.0)
    return h, np.where(inside, np.abs(f * d), 0.0), nz


def process(x, grains, out_first=0, nout=None, ptable=None, htable=None, bound=False, subnormal=None):
    """x: float32[nch, nin], grains int[ngrains, 4] -> fp64[nch, nout], outputs out_first .. out_first + nout - 1.
    A non-finite sample counts as 0 in y; bound=True returns (y, tol, poisoned): tol the derived bound on |y_kernel - y| per sample
    (tests/test_gpu_psola.py states it) and poisoned the outputs that the kernel gives a non-finite value: those with a non-finite sample under a tap of
    a grain with h != 0.

    The last term of tol covers roundings in the subnormal range.  The default, 2^-149 (1 + (G + 67) / D), is kept bit for bit; it is smaller than
    the worst case below wherever D > about 2.2, which no test at O(1) amplitudes can see.  subnormal="derived" replaces it and returns
    (y, tol, poisoned, G, den), G the number of grains covering an output and den = D = sum h_g.  DERIVATION.  A float32 result in the subnormal
    range is within 2^-150 absolute of the exact one (half the spacing 2^-149) instead of within u relative, so every rounding is within
    u |r| + 2^-150 and the absolute parts add up beside the relative bound.  The window weight h and the weight sum s of the taps are normal (h is 0
    or above 2^-50, |s| = |d_g| about 1): only the signal path counts.  Per fractional grain, 64 fused multiply-adds into `a` give 64 2^-150, the
    division a / s turns that into 64 2^-150 / |d_g| and rounds once more: |xt^ - xt| gains (64 / |d_g| + 1) 2^-150; a whole-sample grain reads the
    sample itself and gains nothing.  The numerator takes G fused multiply-adds, G 2^-150, and carries sum |h_g| (64 / |d_g| + 1) 2^-150 =: Z 2^-150
    from the grains; the quotient divides both by D and rounds once:
        2^-150 ((Z + G) / D + 1)    to first order,
    and one more unit of 2^-150 covers the second order (an absolute error scaled by the relative errors of h^, s^ and the weight sum, a factor
    below 1 + (G + 70) u).  With every grain fractional and |d_g| >= 1, Z <= 65 D and the term is at most 2^-150 (G / D + 67), the hand count of
    the same roundings; this one takes |d_g| from the table instead of assuming it and charges whole-sample grains nothing, so it is never larger."""
    x = np.asarray(x, np.float32)
    if x.ndim == 1:
        x = x[None, :]
    nch, nin = x.shape
    nout = nin - out_first if nout is None else nout
    P = (VM.prototype() if ptable is None else np.asarray(ptable, np.float32)).astype(np.float64)
    Hn = window() if htable is None else np.asarray(htable, np.float32)
    g = np.asarray(grains, np.int64).reshape(-1, 4)
    pad = MAX_PERIOD + TAPS + 1
    bad = ~np.isfinite(x)
    buf = np.zeros((nch, nin + 2 * pad), np.float64)                      # buf[:, pad + i] = x[:, i], zeros outside
    buf[:, pad:pad + nin] = np.where(bad, np.float32(0.0), x)
    badbuf = np.zeros((nch, nin + 2 * pad), bool)
    badbuf[:, pad:pad + nin] = bad
    num = np.zeros((nch, nout)); den = np.zeros(nout)
    A = np.zeros((nch, nout)); S = np.zeros(nout); E = np.zeros((nch, nout)); G = np.zeros(nout, np.int64)
    Z = np.zeros(nout)                                                    # sum |h_g| (64 / |d_g| + 1) over the fractional grains
    poisoned = np.zeros((nch, nout), bool)
    u = 2.0 ** -24
    i = np.arange(TAPS, dtype=np.int64)
    for t, tf, dq, L in g.tolist():
        lo, hi = max(t - L + 1, out_first), min(t + L, out_first + nout - 1)
        if lo > hi:
            continue
        n = np.arange(lo, hi + 1, dtype=np.int64)
        h, fd, nz = grain_weights(n, t, tf, L, Hn)
        if not nz.any():
            continue
        n, h, fd = n[nz], h[nz], fd[nz]
        sl = n - out_first
        D, phi = dq >> 8, dq & (Q - 1)                                    # floored
        if phi == 0:
            idx = pad + n - D
            xt = buf[:, idx]
            e = np.zeros_like(xt)
            hit = badbuf[:, idx]
        else:
            w = P[np.abs(Q * (i - (TAPS // 2 - 1)) - (Q - phi))]
            idx = pad + (n - D - 1 - (TAPS // 2 - 1))[:, None] + i[None, :]
            xv = buf[:, idx]                                              # [nch, len, 64]
            Dg = w.sum()
            xt = (xv * w).sum(axis=2) / Dg
            # 64 fused multiply-adds and 64 additions into f32 accumulators, then one division
            e = u * (TAPS * ((np.abs(xv) * np.abs(w)).sum(axis=2) + np.abs(xt) * np.abs(w).sum()) / abs(Dg) + np.abs(xt))
            hit = badbuf[:, idx].any(axis=2)
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

def tune_ratios(records, sample_rate, scale_mask=0xFFF, strength=1.0, retune=1.0, a4=440.0):
    """float64[nrec] of pv_psola_ratios: pv_tune_plan's target rule, the one-pole per record, 2^r held within [1/2, 2]."""
    if not 1 <= scale_mask <= 0xFFF or not 0.0 <= strength <= 1.0 or not 0.0 < retune <= 1.0 or not sample_rate > 0.0 or not a4 > 0.0:
        raise ValueError("bad argument")
    out, r = [], 0.0
    for rec in np.asarray(records, np.int32).reshape(-1, 4):
        p, t = FM.period(rec), 0.0
        if p > 0.0:
            n = 69.0 + 12.0 * math.log2(sample_rate / p / a4)
            t = strength * (float(FM.nearest_allowed(n, scale_mask)) - n) / 12.0
        r += retune * (t - r)
        out.append(min(max(2.0 ** r, 0.5), 2.0))
    return np.array(out, np.float64)


def psola_plan(records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios=None, offset=0.0):
    """int32[ngrains, 4] of pv_psola_plan.  offset: A_0, the first analysis mark (the C planner has 0; the envelope tests sweep it)."""
    records = np.asarray(records, np.int32).reshape(-1, 4)
    nrec = records.shape[0]
    if (f0_hop < 1 or min_period < 2 or max_period < min_period or max_period > MAX_PERIOD or not min_period <= unvoiced_period <= max_period
            or not 0 <= input_len < MAX_POSITION):
        raise ValueError("bad argument")
    if ratios is not None:
        ratios = np.asarray(ratios, np.float64)
        if ratios.shape != (nrec,) or not np.all((ratios >= 0.5) & (ratios <= 2.0)):
            raise ValueError("bad ratios")
    periods = [FM.period(r) for r in records]
    cap = float(2 * max_period - 4) if max_period > 2 else 1.0

    def rec(tau):
        if nrec == 0:
            return -1
        return min(max((math.floor(tau) - f0_center + f0_hop // 2) // f0_hop, 0), nrec - 1)

    def voiced(tau):
        j = rec(tau)
        return j >= 0 and periods[j] > 0.0

    def period(tau):
        j = rec(tau)
        q = periods[j] if j >= 0 else 0.0
        if not q > 0.0:
            return float(unvoiced_period)
        return min(max(q, float(min_period)), float(max_period))

    def ratio(tau):
        j = rec(tau)
        if j < 0 or ratios is None or not periods[j] > 0.0:
            return 1.0
        return float(ratios[j])

    def step(tau):
        return min(period(tau) / ratio(tau), cap)

    grains = []
    length = float(input_len)
    A = float(offset)
    An = A + period(A)
    T = Tprev = 0.0
    held = None                                                          # (T, A, gap before)

    def emit(h, gap_after):
        hT, hA, hgap = h
        L = math.floor(period(hA) + 0.5)
        L = max(L, math.floor(max(hgap, gap_after) / 2.0) + 2, 2)
        L = min(L, max_period)
        c = math.floor(256.0 * hT + 0.5)
        grains.append([c >> 8, c & 255, math.floor(256.0 * (hT - hA) + 0.5), L])

    while T < length:
        while abs(An - T) < abs(A - T):
            A = An
            An = A + period(A)
        if held is not None and not voiced(T) and not voiced(A) and A < length and A >= Tprev + 1.0 and A - Tprev <= cap:
            T = A
        if held is not None:
            emit(held, T - held[0])
        held = (T, A, T - held[0] if held is not None else 0.0)
        Tprev = T
        T = T + step(T)
    if held is not None:
        emit(held, T - held[0])
    return np.array(grains, np.int32).reshape(-1, 4)


def records_of(periods):
    """int32[n, 4] records whose FM.period is exactly the given value: p > 0 voiced (integer part and a parabola for the fraction in 1/1024 steps),
    0 empty, p < 0 unvoiced with best lag -p."""
    out = []
    for p in periods:
        if p == 0:
            out.append([0, 0, 0, 0])
        elif p < 0:
            out.append([int(p), 9000, 8000, 9000])
        else:
            tau = int(round(p))
            k = int(round((p - tau) * 1024))                              # the fraction k / 1024 in [-1/2, 1/2]: 0.5 (cm - cp) / (cm - 2 c0 + cp)
            out.append([tau, 512 + k, 0, 512 - k])
    return np.array(out, np.int32).reshape(-1, 4)


# ---- test signals ----------------------------------------------------------------------------------------------------------------------------

FORMANTS = ((1200.0, 80.0), (2600.0, 120.0))                              # centre and bandwidth in Hz


def _resonator_response(freq, sample_rate):
    """|H| of the two resonators in cascade at the frequencies `freq` (Hz): the envelope of voice()."""
    z = np.exp(-2j * np.pi * np.asarray(freq, np.float64) / sample_rate)
    H = np.ones_like(z)
    for fc, bw in FORMANTS:
        r = math.exp(-math.pi * bw / sample_rate)
        H = H / (1.0 - 2.0 * r * math.cos(2.0 * math.pi * fc / sample_rate) * z + r * r * z * z)
    return np.abs(H)


def voice(period, n, sample_rate=FM.SAMPLE_RATE, phase=0.0, amplitude=0.9):
    """float32[n]: a band-limited pulse train of the given period in samples (harmonics below 0.45 sample_rate, equal amplitude, a pulse at
    t = phase * period) through the two resonators, in closed form as its steady state: a sum of harmonics."""
    t = np.arange(n, dtype=np.float64) - phase * period
    ks = np.arange(1, int(0.45 * period) + 1)
    amp = _resonator_response(ks * sample_rate / period, sample_rate)
    z = np.exp(-2j * np.pi * ks / period)
    H = np.ones_like(z)
    for fc, bw in FORMANTS:
        r = math.exp(-math.pi * bw / sample_rate)
        H = H / (1.0 - 2.0 * r * math.cos(2.0 * math.pi * fc / sample_rate) * z + r * r * z * z)
    y = np.zeros(n)
    for k, a, ph in zip(ks, amp, np.angle(H)):
        y += a * np.cos(2.0 * np.pi * k * t / period + ph)
    return (amplitude * y / np.max(np.abs(y))).astype(np.float32)


def harmonic_amplitudes(y, period, lo, hi):
    """Least-squares amplitudes of the harmonics k / period of y[lo:hi] (fp64), k = 1 .. floor(0.45 period): (frequencies in cycles per sample,
    amplitudes, relative residual)."""
    seg = np.asarray(y, np.float64)[lo:hi]
    t = np.arange(lo, hi, dtype=np.float64)
    ks = np.arange(1, int(0.45 * period) + 1)
    ph = 2.0 * np.pi * np.outer(t, ks) / period
    M = np.concatenate([np.cos(ph), np.sin(ph), np.ones((t.size, 1))], axis=1)
    coef, *_ = np.linalg.lstsq(M, seg, rcond=None)
    res = float(np.linalg.norm(M @ coef - seg) / np.linalg.norm(seg))
    return ks / period, np.hypot(coef[:ks.size], coef[ks.size:2 * ks.size]), res
