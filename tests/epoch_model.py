"""CPU model of the epoch records (EpochTracker / pv_epoch_track) and of the epoch-aligned planner (pv_epoch_plan): numpy int64 and fp64.  TEST
INFRASTRUCTURE ONLY, and the normative definition (DESIGN.md "Pitch-synchronous correction", "Epoch marks"); the reference has no counterpart.

A record is four int32 {pos, K, w, s}, an exact integer function of the frame's `window` samples and of p, the period in 1/256 sample:
  scale    as tests/f0_model.py, one bit narrower: A = max |x| = f 2^e, q_i = rint(x_i 2^(10 - e)), |q_i| <= 1024; silence, a non-finite sample or a
           p outside [256 * 8, 256 * max_period] give {0, 0, 0, 0}
  sizes    w = max(2, p >> 10), Pc = (p + 255) >> 8, S(a, b) = sum_{a <= i < b} q_i^2
  rise     D[n] = S(n, n + w) - S(n - w, n), mass M[n] = S(n - w, n + w), for w <= n <= window - w
  comb     K = #{k >= 0: w + Pc - 1 + ((k p) >> 8) <= window - w}, C(phi) = sum_{k < K} D[w + phi + ((k p) >> 8)], phi = 0 .. Pc - 1
  record   {w + phi*, K, w, (max(C(phi*), 0) 2^14) div Mtot}, phi* the first argmax, Mtot = sum_{k < K} M[w + phi* + ((k p) >> 8)], 0 when Mtot == 0
The planner is tests/psola_model.py psola_plan with the analysis marks pulled onto the lattice that a record's position and the period span."""
import math

import numpy as np

import f0_model as FM
import psola_model as PM

S_ONE = 1 << 14
MIN_PERIOD = 8
MAX_PERIOD = 2048
MAX_WINDOW = 8192
DEFAULT_LOCK = 0.125


def quantise(frame):
    """int64 q of one frame (float32[window]), or None for silence or a non-finite sample."""
    x = np.asarray(frame, np.float32)
    if not np.all(np.isfinite(x)):
        return None
    A = np.float32(np.max(np.abs(x)))
    if A == 0:
        return None
    _, e = np.frexp(A)                                                  # A = f 2^e, f in [0.5, 1)
    return np.rint(np.ldexp(x, 10 - int(e))).astype(np.int64)           # exact scaling, ties to even


def record(frame, p, max_period):
    """The record of one frame (float32[window]) at the period p / 256."""
    p = int(p)
    q = quantise(frame)
    if q is None or not 256 * MIN_PERIOD <= p <= 256 * max_period:
        return [0, 0, 0, 0]
    window = q.size
    w, Pc = max(2, p >> 10), (p + 255) >> 8
    cs = np.concatenate([[0], np.cumsum(q * q)])                        # cs[i] = S(0, i)
    n = np.arange(w, window - w + 1)
    D = np.zeros(window + 1, np.int64)
    M = np.zeros(window + 1, np.int64)
    D[n] = cs[n + w] - 2 * cs[n] + cs[n - w]
    M[n] = cs[n + w] - cs[n - w]
    K = 0
    while w + Pc - 1 + ((K * p) >> 8) <= window - w:
        K += 1
    assert K >= 1
    teeth = (np.arange(K, dtype=np.int64) * p) >> 8
    C = np.array([int(np.sum(D[w + phi + teeth])) for phi in range(Pc)], np.int64)
    phi = int(np.argmax(C))                                             # the first argmax
    Mtot = int(np.sum(M[w + phi + teeth]))
    s = (max(int(C[phi]), 0) * S_ONE) // Mtot if Mtot else 0
    assert 0 <= s <= S_ONE
    return [w + phi, K, w, s]


def frames(n, window, hop):
    return max((n - window) // hop + 1, 0)


def track(x, window, hop, max_period, periods256, nframes=None):
    """int32[nframes, 4] records of one channel x; frame m reads x[m hop : m hop + window] and periods256[m]."""
    x = np.asarray(x, np.float32)
    nframes = min(frames(x.size, window, hop), len(periods256)) if nframes is None else nframes
    return np.array([record(x[m * hop:m * hop + window], periods256[m], max_period) for m in range(nframes)], np.int32).reshape(nframes, 4)


def periods(records):
    """int32[nrec] of pv_epoch_periods: floor(256 * period + 1/2) per f0 record, 0 where it is unvoiced or empty."""
    return np.array([math.floor(256.0 * FM.period(r) + 0.5) for r in np.asarray(records, np.int32).reshape(-1, 4)], np.int32)


def epoch_plan(records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios=None, epochs=None, min_strength=0, lock=DEFAULT_LOCK):
    """int32[ngrains, 4] of pv_epoch_plan: PM.psola_plan with A_0 = snap(0, none), A_(i+1) = snap(A_i + P(A_i), A_i).  epochs: int32[nrec, 4], record j
    the epoch record of f0 record j with its position relative to j * f0_hop, or None (then the grains are PM.psola_plan's)."""
    records = np.asarray(records, np.int32).reshape(-1, 4)
    nrec = records.shape[0]
    if (f0_hop < 1 or min_period < 2 or max_period < min_period or max_period > PM.MAX_PERIOD or not min_period <= unvoiced_period <= max_period
            or not 0 <= input_len < PM.MAX_POSITION or not 0.0 < lock <= 1.0 or not 0 <= min_strength <= S_ONE):
        raise ValueError("bad argument")
    if ratios is not None:
        ratios = np.asarray(ratios, np.float64)
        if ratios.shape != (nrec,) or not np.all((ratios >= 0.5) & (ratios <= 2.0)):
            raise ValueError("bad ratios")
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
    A = snap(0.0, None)
    An = snap(A + period(A), A)
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
            An = snap(A + period(A), A)
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
