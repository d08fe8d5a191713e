"""Parity at level: the yardstick, the corpus and the float32 restatement behind tests/test_level_model.py (CPU) and tests/test_gpu_level_parity.py (GPU).

TEST INFRASTRUCTURE, no GPU.  The stream gates of the parity tests (rms(y - yo) over a whole stream, all channels together, <= 2e-7) are loud-weighted: a quiet
channel, a quiet passage or one hop can be wrong without moving them.  Here every output hop of every channel is held at its own level.

The level of a hop.  Frame m of a channel is the Hann-windowed input x[(m + 1) hop - N, (m + 1) hop) (zeros before the stream starts); the oracle adds its R = N / hop
segments into output hops m .. m + R - 1 (oracle/pv_oracle.c, pvo_process2: the frame is added, the first hop of the accumulator leaves, the rest moves up).  So the
frames that reach output hop h are F(h) = {h - R + 1 .. h} (those that exist), and

    L(c, h) = max over m in F(h) of rms(window * frame m of channel c)         in float64, from the test's own input.

The fp32 error of a frame's shift and inverse scales with that frame's level, the f32 rounding of the reference's overlap-add accumulator with the loudest frame still in it:
L is the yardstick for both.  Hop metric: rms(y - yo over the hop) / L <= K_rms and max|y - yo| / L <= K_max, every channel, every hop; where L == 0 every frame that
reaches the hop is digital silence and both hops must be exactly 0.

K_rms and K_max are never fitted to a kernel.  `restate` below is a plain float32 restatement of the oracle's operation (f32 window, f32 radix-2 FFT, the oracle's own
peak set so that no decision can flip, f32 complex product with an f32 root of unity, f32 inverse, window and overlap-add); its own worst rms / L and max / L against the
oracle over the corpus are pinned below (tests/test_level_model.py reproduces them), and the GPU gate is GATE_FACTOR times those figures: a hand-tuned kernel and a naive
restatement order their roundings differently, the factor covers that and no more (the standing practice of tests/test_gpu_pitch.py and tests/test_vari_model.py).
"""
import functools

import numpy as np

import gpu_algo_model as G
import oracle_lib
import signals as S

EPS32 = 2.0 ** -24
GATE_FACTOR = 4.0
STREAM_RMS_GATE = 2e-7                     # the stream gate of tests/test_gpu_parity.py (REGRESSION_RMS), for the planted-perturbation check

# The restatement's own worst figures against the oracle, per FFT size: (rms / L, max / L) over every hop of every channel of the corpus below (eight runs: fade, burst,
# quiet_mid, quiet_first, quiet_last, scaled_up, scaled_down, loud_partial), pitch rows 1.5, 0.8 and the 0.5 -> 2.0 sweep, at the hop sizes of SHAPES.
# Measured 2026-10-19 by tests/test_level_model.py::test_restatement_figures_are_pinned_and_reproduced, plus 3 % and rounded up to two digits; the test asserts the restatement stays
# under them and within a factor 1.25 above (so a pin cannot go stale on the loose side either).
RESTATEMENT_FIGURES = {
    64: (1.1e-7, 2.9e-7),        # measured 1.026e-07, 2.787e-07
    256: (1.0e-7, 3.5e-7),       # measured 9.696e-08, 3.315e-07
    1024: (9.8e-8, 4.9e-7),      # measured 9.453e-08, 4.736e-07
    2048: (1.4e-7, 5.7e-7),      # measured 1.346e-07, 5.519e-07   (hop 128; hop 512 lies below)
    4096: (9.9e-8, 1.1e-6),      # measured 9.526e-08, 1.024e-06   (hop 512; hop 1024 lies below)
    8192: (8.8e-8, 7.9e-7),      # measured 8.500e-08, 7.662e-07
}

# (N, hop) of the GPU test's shapes (tests/test_gpu_level_parity.py adds the flags)
SHAPES = [(1024, 256), (2048, 512), (2048, 128), (4096, 1024), (8192, 2048), (4096, 512), (256, 64), (64, 16)]
PITCH_ROWS = ("1.5", "0.8", "sweep")
NCH = 3


def gate(N):
    """(K_rms, K_max) the kernels are held to at FFT size N."""
    r, m = RESTATEMENT_FIGURES[N]
    return GATE_FACTOR * r, GATE_FACTOR * m


def nhops(N):
    return 48 if N <= 2048 else 16


def pitch_row(name, T):
    if name == "sweep":                                              # 0.5 -> 2.0 over the stream (the sweep of tests/test_gpu_forward_first.py, one period)
        return (0.5 + 1.5 * np.arange(T) / (T - 1)).astype(np.float32)
    return np.full(T, float(name), np.float32)


# ---- the corpus: signals with dynamics, all from the tonal-plus-noise material of tests/signals.py (peaks exist at every level) ----

def _material(T, hop, stream):
    return np.stack([S.make_signal("tonal", c, T * hop, stream=stream).astype(np.float64) for c in range(NCH)])


def _fade_gain(n):
    """0 dB at both ends, -140 dB in the middle, a parabola in dB: -140 (1 - (2u - 1)^2), u = position in the stream.  A straight V in dB would, at 48 hops, spend
    fewer hops below the guarded range's low end (about -117 dB) than ONE frame of N / hop = 16 is long, and no frame of such a run would ever cross it; the parabola
    falls fast where nothing happens (11.7 dB per hop at the ends of a 48-hop stream), crosses the low end at 4 to 5 dB per hop and lingers at the bottom."""
    u = np.arange(n, dtype=np.float64) / (n - 1)
    return 10.0 ** (-140.0 * (1.0 - (2.0 * u - 1.0) ** 2) / 20.0)


def burst_hops(N, hop):
    """3 loud hops + 2R silent ones + at least 5 of the quiet tone: longer than the shape's T where R is large."""
    return max(nhops(N), 3 + 2 * (N // hop) + 5)


@functools.lru_cache(maxsize=None)
def corpus(N, hop):
    """name -> float32[NCH, T * hop].  Peak levels lie within 1e-9 .. 1e9 (0.45 * 2^-20 = 4e-7 .. 0.45 * 2^20 = 5e5)."""
    T, R = nhops(N), N // hop
    out = {}
    fade = _material(T, hop, 11) * _fade_gain(T * hop)
    out["fade"] = fade
    Tb = burst_hops(N, hop)
    b = _material(Tb, hop, 12)
    b[:, 3 * hop:(3 + 2 * R) * hop] = 0.0
    b[:, (3 + 2 * R) * hop:] *= 1e-5                                    # the -100 dB tone
    out["burst"] = b
    q = _material(T, hop, 13)
    gains = {"quiet_mid": (1.0, 1e-5, 1e-3), "quiet_first": (1e-5, 1.0, 1e-3), "quiet_last": (1e-3, 1.0, 1e-5)}
    for name, g in gains.items():                                       # 0 dB, -100 dB and -60 dB in one launch; the quiet one first, in the middle and last
        out[name] = q * np.asarray(g)[:, None]
    out["scaled_up"] = fade * 2.0 ** 20
    out["scaled_down"] = fade * 2.0 ** -20
    i = np.arange(T * hop, dtype=np.float64)
    amp = 0.5
    out["loud_partial"] = np.stack([amp * np.sin(2 * np.pi * (0.0731 + 0.011 * c) * i)
                                    + S.lcg_noise(3000 + c, T * hop, amp * 10.0 ** (-110.0 / 20.0)).astype(np.float64) for c in range(NCH)])
    out = {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- the yardstick ----

def frames_of(x, N, hop, dtype=np.float32):
    """[..., T, N]: frame m = x[(m + 1) hop - N, (m + 1) hop), zeros before the start (the oracle's input buffer after m + 1 quanta)."""
    x = np.asarray(x)
    T = x.shape[-1] // hop
    xp = np.concatenate([np.zeros(x.shape[:-1] + (N - hop,), x.dtype), x], axis=-1)
    idx = np.arange(T)[:, None] * hop + np.arange(N)[None, :]
    return xp[..., idx].astype(dtype)


def hop_levels(x, N, hop):
    """L[c, h], float64."""
    R = N // hop
    w = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N))
    f = frames_of(x, N, hop, np.float64) * w
    fr = np.sqrt(np.mean(f * f, axis=-1))                                # [nch, T]
    L = fr.copy()
    for j in range(1, R):
        L[:, j:] = np.maximum(L[:, j:], fr[:, :-j])
    return L


def hop_metrics(y, yo, L, hop):
    """(rms / L, max / L), each [nch, T].  A hop with L == 0 gives 0 where y and yo are both exactly 0 over it and inf otherwise."""
    nch, T = L.shape
    d = (np.asarray(y, np.float64) - np.asarray(yo, np.float64)).reshape(nch, T, hop)
    r, m = np.sqrt(np.mean(d * d, axis=-1)), np.max(np.abs(d), axis=-1)
    zero = L == 0
    nz = np.any(np.asarray(y).reshape(nch, T, hop) != 0, axis=-1) | np.any(np.asarray(yo).reshape(nch, T, hop) != 0, axis=-1)
    bad = ~(np.isfinite(r) & np.isfinite(m))
    with np.errstate(divide="ignore", invalid="ignore"):
        rr, mm = r / L, m / L
    rr[zero], mm[zero] = np.where(nz[zero], np.inf, 0.0), np.where(nz[zero], np.inf, 0.0)
    rr[bad], mm[bad] = np.inf, np.inf
    return rr, mm


def hop_failures(y, yo, L, hop, k_rms, k_max):
    """[(channel, hop, rms / L, max / L)] of the hops that miss the gate; worst (rms / L, max / L) over all hops."""
    rr, mm = hop_metrics(y, yo, L, hop)
    bad = np.argwhere((rr > k_rms) | (mm > k_max))
    return [(int(c), int(h), float(rr[c, h]), float(mm[c, h])) for c, h in bad], (float(rr.max()), float(mm.max()))


# ---- the oracle, hop by hop (output and peak sets) ----

@functools.lru_cache(maxsize=None)
def oracle_run(N, hop, signal, row, with_peaks=False):
    """(yo float32[NCH, n], peaks[c][m] or None) of corpus signal `signal` under pitch row `row`.  Channels are independent in the reference: one mono oracle each
    where the peak sets are wanted (Oracle.debug() taps the last channel processed)."""
    x = corpus(N, hop)[signal]
    T = x.shape[1] // hop
    p = pitch_row(row, T)
    if not with_peaks:
        yo = oracle_lib.Oracle(N, hop, x.shape[0]).process_planar(x, p)
        yo.setflags(write=False)
        return yo, None
    yo = np.zeros_like(x)
    peaks = []
    for c in range(x.shape[0]):
        o = oracle_lib.Oracle(N, hop, 1)
        pk = []
        for m in range(T):
            yo[c, m * hop:(m + 1) * hop] = o.process([x[c, m * hop:(m + 1) * hop]], p[m])[0]
            pk.append(o.debug()["peaks"].astype(np.int64))
        o.close()
        peaks.append(pk)
    yo.setflags(write=False)
    return yo, peaks


# ---- the float32 restatement ----

@functools.lru_cache(maxsize=None)
def _bitrev(N):
    bits = N.bit_length() - 1
    r = np.zeros(N, np.int64)
    for b in range(bits):
        r |= ((np.arange(N) >> b) & 1) << (bits - 1 - b)
    return r


def fft32(z, inverse=False):
    """Radix-2 decimation-in-time FFT over the last axis in numpy complex64 arithmetic (np.fft may compute in double and is not used).  Twiddles are the float64
    values rounded to float32.  No 1 / N."""
    N = z.shape[-1]
    lead = z.shape[:-1]
    a = np.ascontiguousarray(np.asarray(z, np.complex64)[..., _bitrev(N)])
    half = 1
    sign = 2.0 if inverse else -2.0
    while half < N:
        tw = np.exp(sign * 1j * np.pi * np.arange(half) / (2 * half)).astype(np.complex64)
        a = a.reshape(lead + (N // (2 * half), 2, half))
        e, o = a[..., 0, :], a[..., 1, :] * tw
        a = np.stack([e + o, e - o], axis=-2)
        assert a.dtype == np.complex64
        half *= 2
    return a.reshape(lead + (N,))


def residue32(xw):
    """gpu_algo_model.residue_upper (what fft.js's real transform leaves in bins N/2+1 .. N-1, which the reference reads when it shifts down), in complex64, over
    the last axis of a batch of frames.  tests/test_level_model.py holds it bit for bit against residue_upper."""
    N = xw.shape[-1]
    power = N.bit_length() - 1
    buf = np.zeros(xw.shape, np.complex64)
    x = np.asarray(xw, np.float32)
    if power % 2 == 0:
        base, nd = 4, (power - 2) // 2
        t = np.arange(N // 8, N // 4)
        off = np.array([G.digit_reverse4(int(v), nd) for v in t], np.int64)
        a, b, c, d = x[..., off], x[..., off + N // 4], x[..., off + N // 2], x[..., off + 3 * N // 4]
        t0, t1, t2, t3 = a + c, a - c, b + d, b - d
        buf.real[..., 4 * t], buf.real[..., 4 * t + 1], buf.real[..., 4 * t + 2], buf.real[..., 4 * t + 3] = t0 + t2, t1, t0 - t2, t1
        buf.imag[..., 4 * t + 1], buf.imag[..., 4 * t + 3] = -t3, t3
    else:
        base, nd = 2, (power - 1) // 2
        t = np.arange(N // 4, N // 2)
        off = np.array([G.digit_reverse4(int(v), nd) for v in t], np.int64)
        a, b = x[..., off], x[..., off + N // 2]
        buf.real[..., 2 * t], buf.real[..., 2 * t + 1] = a + b, a - b
    M = base * 4
    while M <= N // 4:
        q = M // 4
        i = np.arange(0, q // 2 + 1)
        w = np.exp(-2j * np.pi * i / M).astype(np.complex64)
        for o in range(N // 2, N, M):
            A, B, C, D = buf[..., o + i], buf[..., o + q + i] * w, buf[..., o + 2 * q + i] * w * w, buf[..., o + 3 * q + i] * w * w * w
            T0, T1, T2, T3 = A + C, A - C, B + D, B - D
            FA, FB = T0 + T2, T1 - 1j * T3
            FC0 = T0[..., 0] - T2[..., 0]
            SA, SB = np.conj(T1 + 1j * T3), np.conj(T0 - T2)
            buf[..., o + i] = FA
            buf[..., o + q + i] = FB
            buf[..., o + 2 * q] = FC0
            if len(i) > 2:
                inner = i[1:-1]
                buf[..., o + q - inner] = SA[..., 1:-1]
                buf[..., o + 2 * q - inner] = SB[..., 1:-1]
        M *= 4
    assert buf.dtype == np.complex64
    return buf


def shift32(src, peaks, pitch, t, N):
    """shiftPeaks (oracle/pv_oracle.c shift_peaks) on a float32 spectrum src[N] with the GIVEN peak set: region-of-influence walk as index arithmetic, the rotation
    cos / sin(omega t) as the exact N-th root of unity rounded to float32, a complex64 product, contributions summed in float32 in the reference's order."""
    H = N // 2 + 1
    Y = np.zeros(H, np.complex64)
    pk = np.asarray(peaks, np.int64)
    if pk.size == 0:
        return Y
    pf = np.float64(np.float32(pitch))
    psh = G.js_round(pk.astype(np.float64) * pf)
    dead = psh > H
    live = int(np.argmax(dead)) if dead.any() else pk.size                # pv:127-129: `break` at the first peak shifted beyond the spectrum
    if live == 0:
        return Y
    gap = pk[1:] - pk[:-1]
    starts = np.concatenate([[0], pk[1:] - gap // 2])
    ends = np.concatenate([pk[:-1] + (gap + 1) // 2, [N]])
    b = np.arange(0, ends[live - 1])
    own = np.searchsorted(starts, b, side="right") - 1
    bin_sh = psh[own] + (b - pk[own])
    ok = (bin_sh < H) & (bin_sh >= 0)
    b, tgt = b[ok], bin_sh[ok].astype(np.int64)
    ridx = ((tgt - b) % N) * (int(t) % N) % N
    rot = np.exp(2j * np.pi * ridx / N).astype(np.complex64)
    contrib = src[b] * rot
    assert contrib.dtype == np.complex64
    np.add.at(Y, tgt, contrib)
    return Y


def restate(N, hop, x, pitch, peaks):
    """The whole operation in float32: x float32[nch, T * hop], pitch float32[T], peaks[c][m] from the oracle -> float32[nch, T * hop]."""
    nch, n = x.shape
    T, R, H = n // hop, N // hop, N // 2 + 1
    w = G.hann(N)                                                        # the reference's window: float64 formula rounded to float32
    xw = frames_of(x, N, hop, np.float32) * w                            # [nch, T, N]
    assert xw.dtype == np.float32
    X = fft32(xw.astype(np.complex64))
    if np.any(~(pitch >= 1)):
        X[..., H:] = residue32(xw)[..., H:]
    else:
        X[..., H:] = 0
    Y = np.zeros((nch, T, N), np.complex64)
    for c in range(nch):
        for m in range(T):
            Y[c, m, :H] = shift32(X[c, m], peaks[c][m], pitch[m], m * hop, N)
    k = np.arange(1, N // 2)
    Y[..., N - k] = np.conj(Y[..., k])                                   # bundle:69-76
    fr = fft32(Y, inverse=True).real / np.float32(N)
    fr = fr * w / np.float32(R)
    assert fr.dtype == np.float32
    y = np.zeros((nch, n), np.float32)
    acc = np.zeros((nch, N), np.float32)
    for m in range(T):
        acc = acc + fr[:, m]
        y[:, m * hop:(m + 1) * hop] = acc[:, :hop]
        acc = np.concatenate([acc[:, hop:], np.zeros((nch, hop), np.float32)], axis=1)
    return y


# ---- the shifted spectrum, bin by bin ----

def frame_taps(N, T):
    """The frames (hops) whose spectra are compared bin by bin: a loud, a guarded-range-crossing and the quietest frame of `fade`, three settled frames of `loud_partial`."""
    return {"fade": (6, 20, 24) if T == 48 else (2, 7, 8), "loud_partial": (5, 6, 11)}


@functools.lru_cache(maxsize=None)
def oracle_taps(N, hop, signal, pitch, ch=0):
    """{m: (X complex128[N], Y complex128[N/2+1], peaks)} of channel `ch` of corpus signal `signal` at constant pitch factor `pitch`, for the frames of frame_taps."""
    x = corpus(N, hop)[signal][ch]
    T = nhops(N)
    want = frame_taps(N, T)[signal]
    o = oracle_lib.Oracle(N, hop, 1)
    out = {}
    for m in range(max(want) + 1):
        o.process([x[m * hop:(m + 1) * hop]], pitch)
        if m in want:
            d = o.debug()
            out[m] = (d["X"][0::2] + 1j * d["X"][1::2], (d["Y"][0::2] + 1j * d["Y"][1::2])[:N // 2 + 1], d["peaks"].astype(np.int64))
    o.close()
    return out


def residue_term(N, Xfull):
    """Absolute error allowed to ONE above-Nyquist source value, which the kernels rebuild in fp32 (the reference holds it in fp64): log4(N) radix-4
    stages, each one complex product with an f32 twiddle ((1 + sqrt 5) eps) and two additions (2 eps) on values no larger than the largest the residue ends with."""
    return (3.0 + np.sqrt(5.0)) * 0.5 * np.log2(N) * EPS32 * float(np.max(np.abs(Xfull[N // 2 + 1:])))


def spectrum_bound(A, n, n_res, N, Xfull, fp32_forward=False):
    """|Yg[k] - Yr[k]| <= C(n) 2^-24 A[k] (+ the terms of the sources that are not fp64), A[k] = sum of |X[src]| over the n[k] source bins that land on k.

    C from the operations the model (gpu_algo_model.shift_spectrum, pv_device_common.h rotate_route) names, eps = 2^-24, first order:
      * X[src] rounded to f32, componentwise:                          eps |X|
      * the root of unity rounded to f32 (modulus error <= eps):       eps |X|
      * the complex product in f32, four products and two sums
        (Brent, Percival & Zimmermann 2007; 2 eps with an FMA):        sqrt(5) eps |X|
        -> each contribution is off by at most (2 + sqrt 5) eps |X[src]|, together (2 + sqrt 5) eps A[k];
      * n - 1 float32 additions, each partial sum at most A[k]:         (n - 1) eps A[k]   (the first contribution is stored);
      * the reference side is fp64 (its cos / sin argument omega * t reaches 1e5 rad: 1e-11, absorbed in the rounding up of sqrt 5 = 2.2360... to 2.25).
    C(n) = n + 3.25.  A bin with A[k] == 0 receives nothing and must be exactly 0.
    Sources above Nyquist (f < 1) are the fp32 residue: + residue_term each.  fp32_forward: class-A frames of the default N = 1024 / 2048 kernels take X from the fp32
    transform, |A32 - A64| <= E_b = 4 eps max|X| per bin (pv_guard.h): + E_b per contribution."""
    H = N // 2 + 1
    bound = (n + 3.25) * EPS32 * A + n_res * residue_term(N, Xfull)
    if fp32_forward:
        bound = bound + n * 4.0 * EPS32 * float(np.max(np.abs(Xfull[:H])))
    return bound
