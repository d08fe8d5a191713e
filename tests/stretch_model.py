"""CPU model of the phase-locked time stretch (TimeStretch / pv_stretch_*): plain numpy, fp64 transforms, integer phase state.  TEST INFRASTRUCTURE ONLY.

Written from the algorithm text in DESIGN.md ("Time stretch"), frame by frame:
  window (periodic Hann, f32) -> fp64 forward DFT -> f32 squared magnitudes -> findPeaks -> regions of influence (shiftPeaks at f = 1) ->
  fixed-point analysis phase q (u32 turns) -> per-bin phase advance psi += adv (u32, mod 2^32) -> identity phase locking (every bin rotated by
  its peak's angle psi[P] - q[P]) -> fp64 Hermitian inverse, Re, f32, Hann -> overlap-add at the synthesis hop, each frame scaled by hs / N.
Nothing here is taken from the reference: the reference has no time stretch.
"""
import numpy as np

TWO32 = 1 << 32
MASK = np.uint64(0xFFFFFFFF)


def hann_f32(N):
    i = np.arange(N, dtype=np.float64)
    return (0.5 * (1.0 - np.cos(2.0 * np.pi * i / N))).astype(np.float32)


def find_peaks(mag):
    """phase-vocoder.js findPeaks: strict maximum over +-2 bins, i in [2, H - 2).  (The reference's skip of two bins after a peak never hides one: a
    peak's two right neighbours are below it, so neither can be a strict maximum over a span that holds it.)"""
    H = mag.shape[0]
    if H < 5:
        return []
    c = mag[2:H - 2]
    pk = ~((mag[1:H - 3] >= c) | (mag[0:H - 4] >= c) | (mag[3:H - 1] >= c) | (mag[4:H] >= c))
    return (np.nonzero(pk)[0] + 2).tolist()


def doubtful_frame(mag, ulps=2):
    """True when a findPeaks comparison of the frame lies within `ulps` f32 ulps of a tie, or a magnitude is NaN: another correctly rounded transform
    may find other peaks there.  (Introspection for the tests; the model's output does not depend on it.)"""
    mag = np.asarray(mag, np.float32)
    if np.any(np.isnan(mag)):
        return True
    H = mag.shape[0]
    if H < 5:
        return False
    for a, b in ((mag[1:H - 2], mag[2:H - 1]), (mag[0:H - 2], mag[2:H])):        # the (k, k +- 1) and (k, k +- 2) pairs of k in [2, H - 2)
        tol = ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))
        if np.any(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= tol):
            return True
    return False


def regions(peaks, H):
    """P[k]: the peak whose region of influence (shiftPeaks at f = 1) holds bin k; -1 everywhere when there is no peak."""
    P = np.full(H, -1, np.int64)
    n = len(peaks)
    for i, p in enumerate(peaks):
        start = 0 if i == 0 else p - (p - peaks[i - 1]) // 2
        end = H if i == n - 1 else p + -((p - peaks[i + 1]) // 2)      # ceil((p_{i+1} - p) / 2)
        P[start:end] = p
    return P


def phase_q(X):
    """round-to-nearest-even(atan2(Im, Re) / 2 pi * 2^32) mod 2^32; atan2(0, 0) = 0; a bin that is not finite, or a non-finite angle, gives 0
    (the angle of an infinite bin depends on where a transform's arithmetic meets inf - inf)."""
    with np.errstate(invalid="ignore"):
        ang = np.arctan2(X.imag, X.real)
    ang = np.where((X.real == 0) & (X.imag == 0), 0.0, ang)
    ok = np.isfinite(ang) & np.isfinite(X.real) & np.isfinite(X.imag)
    v = np.rint(np.where(ok, ang, 0.0) * (2.0 ** 31 / np.pi)).astype(np.int64)
    return (v & 0xFFFFFFFF).astype(np.uint32)


def phase_advance(q, phi, k, N, ha, hs):
    """adv = hs k 2^32/N + floor((2 d hs + ha) / (2 ha)) mod 2^32, d = (int32)(q - phi - ha k 2^32/N).  All integer (int64 / uint64)."""
    k = np.asarray(k, dtype=np.int64)
    step = TWO32 // N
    e = (np.int64(ha) * k * step) & 0xFFFFFFFF
    d = (q.astype(np.int64) - phi.astype(np.int64) - e) & 0xFFFFFFFF
    d = np.where(d >= 1 << 31, d - TWO32, d)                                           # (int32): the principal value
    adv = np.int64(hs) * k * step + np.floor_divide(2 * d * hs + ha, 2 * ha)           # floor division (numpy // on int64 floors)
    return (adv & 0xFFFFFFFF).astype(np.uint32)


class StretchModel:
    """One pv_stretch handle with `nch` channel slots."""

    def __init__(self, N, ha, hs, nch=1, track_doubt=False):
        if N < 2 or N & (N - 1):
            raise ValueError("FFT size must be a power of two and bigger than 1")
        if not (1 <= ha <= N) or not (1 <= hs <= N // 2):
            raise ValueError("analysis hop in 1..N, synthesis hop in 1..N/2")
        self.N, self.ha, self.hs, self.H = N, ha, hs, N // 2 + 1
        self.hann = hann_f32(N)
        self.scale = np.float32(hs / N)                  # 1 / R_s (exact when hs divides N)
        self.k = np.arange(self.H, dtype=np.int64)
        self.hist = np.zeros((nch, N - ha), np.float32)
        self.acc = np.zeros((nch, N - hs), np.float32)
        self.phi = np.zeros((nch, self.H), np.uint32)
        self.psi = np.zeros((nch, self.H), np.uint32)
        self.last = None                                 # introspection: the last frame's X, mag, q, peaks, adv (see frame)
        self.track_doubt = track_doubt
        self.doubtful = [[] for _ in range(nch)]         # per channel, per frame (track_doubt only): doubtful_frame(mag)
        self.cond_min = np.full((nch, self.H), np.inf)   # per channel (track_doubt only): min over frames of |X_k| / max |X|

    def frame(self, c, block):
        """One frame of channel c: `ha` new samples in, `hs` samples out."""
        N, ha, hs = self.N, self.ha, self.hs
        x = np.concatenate([self.hist[c], np.asarray(block, np.float32)])[-N:]
        self.hist[c] = x[ha:] if ha < N else x[:0]
        xw = x * self.hann                                                              # f32
        X = np.fft.rfft(xw.astype(np.float64))
        mag = (X.real * X.real + X.imag * X.imag).astype(np.float32)
        P = regions(find_peaks(mag), self.H)
        q = phase_q(X)
        adv = phase_advance(q, self.phi[c], self.k, N, ha, hs)
        self.psi[c] = ((self.psi[c].astype(np.uint64) + adv) & MASK).astype(np.uint32)
        self.phi[c] = q
        self.last = {"X": X, "mag": mag, "q": q, "peaks": P, "adv": adv}
        if self.track_doubt:
            self.doubtful[c].append(doubtful_frame(mag))
            ax = np.abs(X)
            self.cond_min[c] = np.minimum(self.cond_min[c], ax / ax.max() if ax.max() > 0 else 0.0)
        if P[0] < 0:
            Y = np.zeros(self.H, np.complex128)                                         # no peaks: silence, as the pitch shifter
        else:
            s = (self.psi[c][P].astype(np.int64) - q[P].astype(np.int64)) & 0xFFFFFFFF
            s = np.where(s >= 1 << 31, s - TWO32, s)
            th = 2.0 * np.pi * s.astype(np.float64) / TWO32
            Y = X * (np.cos(th) + 1j * np.sin(th))
        fr = np.fft.irfft(Y, N).astype(np.float32) * self.hann                          # Re of the Hermitian inverse (1/N), f32, Hann
        full = np.concatenate([self.acc[c], np.zeros(hs, np.float32)]) + fr * self.scale
        self.acc[c] = full[hs:]
        return full[:hs]

    def process(self, x):
        """x: float32[nch, nframes * ha] -> float32[nch, nframes * hs] (channel slots 0..nch-1)."""
        x = np.asarray(x, np.float32)
        nch, n = x.shape
        T = n // self.ha
        assert T * self.ha == n
        y = np.zeros((nch, T * self.hs), np.float32)
        for c in range(nch):
            for m in range(T):
                y[c, m * self.hs:(m + 1) * self.hs] = self.frame(c, x[c, m * self.ha:(m + 1) * self.ha])
        return y
