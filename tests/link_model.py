"""CPU model of linked channels on the time stretch (TimeStretch(channels_per_group=G) / pv_link_channels).  TEST INFRASTRUCTURE ONLY.

Written from DESIGN.md "Linked channels" on the functions of stretch_model.py and tempo_model.py.  Slots [g G, (g + 1) G) are group g.  Per group and
frame: the mix u = ((x_0 + x_1) + x_2) + ... (f32, slot order, over the carried history and the input alike) runs the mono phase path -- Hann, fp64
forward, f32 magnitudes, findPeaks, regions P, q, psi += adv, phi = q -- and every channel c of the group rotates its own spectrum X_c by the mix's
angle psi[P] - q[P], then inverts (fp64, Re, f32), windows, scales by hs / N and overlap-adds into its own accumulator.  So the group's phi / psi are
those of a mono StretchModel fed u, and G = 1 is StretchModel.
"""
import numpy as np

from stretch_model import MASK, TWO32, doubtful_frame, find_peaks, hann_f32, phase_advance, phase_q, regions
from tempo_model import hop_rows, positions


def mix(x, G):
    """float32[nch / G, n]: the f32 sum of each group's channels in slot order, one rounding per add."""
    x = np.asarray(x, np.float32)
    assert x.shape[0] % G == 0, (x.shape, G)
    u = x[0::G].copy()
    for i in range(1, G):
        u = (u + x[i::G]).astype(np.float32)
    return u


class LinkModel:
    """One pv_stretch handle with `nch` channel slots linked in groups of G, analysis hop floor `floor` (the fixed hop of `process`)."""

    def __init__(self, N, floor, hs, nch, G, track_doubt=False):
        if N < 2 or N & (N - 1):
            raise ValueError("FFT size must be a power of two and bigger than 1")
        if not (1 <= floor <= N) or not (1 <= hs <= N // 2):
            raise ValueError("analysis hop in 1..N, synthesis hop in 1..N/2")
        if G < 1 or nch % G:
            raise ValueError("nch must be a whole number of groups of G >= 1")
        self.N, self.floor, self.hs, self.H, self.G = N, floor, hs, N // 2 + 1, G
        self.hann = hann_f32(N)
        self.scale = np.float32(hs / N)
        self.k = np.arange(self.H, dtype=np.int64)
        self.hist = [np.zeros(N - floor, np.float32) for _ in range(nch)]
        self.acc = np.zeros((nch, N - hs), np.float32)
        self.phi = np.zeros((nch // G, self.H), np.uint32)      # per GROUP
        self.psi = np.zeros((nch // G, self.H), np.uint32)
        self.track_doubt = track_doubt
        self.doubtful = [[] for _ in range(nch // G)]            # per group, per frame (track_doubt only): doubtful_frame of the mix's magnitudes
        self.peakless = [[] for _ in range(nch // G)]            # per group, per frame: the mix had no peak (every channel of the group silent)

    def group_frame(self, g, blocks):
        """One frame of group g: blocks[i] (the same length, the frame's hop) are channel g G + i's new samples; returns G blocks of hs outputs."""
        N, hs, G = self.N, self.hs, self.G
        h = len(blocks[0])
        if not self.floor <= h <= N:
            raise ValueError(f"hop {h} outside [{self.floor}, {N}]")
        xs = []
        for i in range(G):
            c = g * G + i
            assert len(blocks[i]) == h
            full = np.concatenate([self.hist[c], np.asarray(blocks[i], np.float32)])
            xs.append(full[full.size - N:])
            self.hist[c] = full[full.size - (N - self.floor):]
        u = xs[0]
        for i in range(1, G):
            u = (u + xs[i]).astype(np.float32)
        # the group's phase path: the mono path on u
        Xu = np.fft.rfft((u * self.hann).astype(np.float64))
        mag = (Xu.real * Xu.real + Xu.imag * Xu.imag).astype(np.float32)
        P = regions(find_peaks(mag), self.H)
        q = phase_q(Xu)
        adv = phase_advance(q, self.phi[g], self.k, N, h, hs)
        self.psi[g] = ((self.psi[g].astype(np.uint64) + adv) & MASK).astype(np.uint32)
        self.phi[g] = q
        self.peakless[g].append(bool(P[0] < 0))
        if self.track_doubt:
            self.doubtful[g].append(doubtful_frame(mag))
        if P[0] >= 0:
            s = (self.psi[g][P].astype(np.int64) - q[P].astype(np.int64)) & 0xFFFFFFFF
            s = np.where(s >= 1 << 31, s - TWO32, s)
            th = 2.0 * np.pi * s.astype(np.float64) / TWO32
            rot = np.cos(th) + 1j * np.sin(th)
        out = []
        for i in range(G):
            c = g * G + i
            if P[0] < 0:
                Y = np.zeros(self.H, np.complex128)                                     # no peak in the mix: silence in every channel
            else:
                Y = np.fft.rfft((xs[i] * self.hann).astype(np.float64)) * rot
            fr = np.fft.irfft(Y, N).astype(np.float32) * self.hann
            full = np.concatenate([self.acc[c], np.zeros(hs, np.float32)]) + fr * self.scale
            self.acc[c] = full[hs:]
            out.append(full[:hs])
        return out

    def process_hops(self, x, hops):
        """x: float32[nch, >= every row's total]; hops: int[nframes] or int[nch, nframes] (rows equal within a group) -> float32[nch, nframes hs]."""
        x = np.asarray(x, np.float32)
        nch = x.shape[0]
        rows = hop_rows(hops, nch)
        T = rows.shape[1]
        y = np.zeros((nch, T * self.hs), np.float32)
        for g in range(nch // self.G):
            c0 = g * self.G
            for i in range(1, self.G):
                assert np.array_equal(rows[c0 + i], rows[c0]), "schedule rows differ within a group"
            S = positions(rows[c0])
            assert S[-1] <= x.shape[1], (S[-1], x.shape)
            for m in range(T):
                outs = self.group_frame(g, [x[c0 + i, S[m]:S[m + 1]] for i in range(self.G)])
                for i in range(self.G):
                    y[c0 + i, m * self.hs:(m + 1) * self.hs] = outs[i]
        return y

    def process(self, x):
        """The fixed-hop call: x float32[nch, nframes * floor] -> float32[nch, nframes * hs]."""
        x = np.asarray(x, np.float32)
        T = x.shape[1] // self.floor
        assert T * self.floor == x.shape[1]
        return self.process_hops(x, np.full(T, self.floor, np.int64))


def phase_fit(y, N, ha, hs, freqs):
    """Per partial, the fitted phase (rad) of each channel of y over the steady range (tones.tone_fit's basis, g(n) cos / sin): float64[nch, len(freqs)]."""
    import tones as TN
    y = np.asarray(y, np.float64)
    lo, hi = TN.steady_range(N, ha, hs, y.shape[1])
    g = TN.envelope(N, hs, y.shape[1])[lo:hi]
    k = np.arange(lo, hi, dtype=np.float64)
    cols = []
    for f in freqs:
        w = 2.0 * np.pi * f / N
        cols += [g * np.cos(w * k), g * np.sin(w * k)]
    B = np.stack(cols, axis=1)
    out = np.zeros((y.shape[0], len(freqs)))
    for c in range(y.shape[0]):
        coef, *_ = np.linalg.lstsq(B, y[c, lo:hi], rcond=None)
        out[c] = np.arctan2(-coef[1::2], coef[0::2])                 # A cos(w k + p) = A cos p cos(w k) - A sin p sin(w k)
    return out


def wrap(a):
    """Angles to (-pi, pi]."""
    return (np.asarray(a, np.float64) + np.pi) % (2 * np.pi) - np.pi


def stereo_partials(N, freqs, amps, phases, n):
    """float32[len(amps), n]: channel c = sum_i amps[c][i] cos(2 pi freqs[i] k / N + phases[c][i])."""
    import tones as TN
    return np.stack([TN.partials(N, freqs, a, p, n) for a, p in zip(amps, phases)])
