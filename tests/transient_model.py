"""CPU model of phase resets, onset strength, the onset rule and the transient planner (TimeStretch.process_hops(..., resets),
TimeStretch.onset_strength, phaze_amd.onsets_from_strength, phaze_amd.transient_plan).  TEST INFRASTRUCTURE ONLY.

Written from DESIGN.md "Phase resets" on the functions of stretch_model.py: TempoModel / LinkModel's frame with one line added,

    psi_m = r_m ? q_m : psi_{m-1} + adv_m        (phi_m = q_m either way; every bin of the frame)

for slots linked in groups of G (G = 1: every slot on its own, TempoModel).  A reset frame rotates by psi[P] - q[P] = 0: its output is
Hann * IDFT(X) * hs / N, and it is still silent when it has no peak.  Nothing here is taken from the reference: the reference has no time stretch.
"""
import numpy as np

import tones as TN
from stretch_model import MASK, TWO32, doubtful_frame, find_peaks, hann_f32, phase_advance, phase_q, regions
from tempo_model import hop_rows, positions


def flag_rows(resets, nch, T):
    """bool[nch, T] from None (no reset), a shared row (1-D) or per-channel rows (2-D)."""
    if resets is None:
        return np.zeros((nch, T), bool)
    r = np.asarray(resets)
    assert np.all((r == 0) | (r == 1)), "reset flags are 0 / 1"
    r = r.astype(bool)
    if r.ndim == 1:
        return np.broadcast_to(r, (nch, r.size))
    assert r.shape == (nch, T), r.shape
    return r


class TransientModel:
    """One pv_stretch handle with `nch` channel slots in groups of G, analysis hop floor `floor`, run with per-frame hops and reset flags."""

    def __init__(self, N, floor, hs, nch=1, G=1, track_doubt=False):
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
        self.doubtful = [[] for _ in range(nch // G)]            # per group, per frame (track_doubt only): doubtful_frame of the group's magnitudes
        self.last = None                                         # introspection: the last frame's X (of the mix), mag, q, peaks

    def group_frame(self, g, blocks, reset=False):
        """One frame of group g: blocks[i] (the same length, the frame's hop) are slot g G + i's new samples; returns G blocks of hs outputs."""
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
        Xu = np.fft.rfft((u * self.hann).astype(np.float64))
        mag = (Xu.real * Xu.real + Xu.imag * Xu.imag).astype(np.float32)
        P = regions(find_peaks(mag), self.H)
        q = phase_q(Xu)
        if reset:
            self.psi[g] = q.copy()                                                      # the reset line: psi := q
        else:
            adv = phase_advance(q, self.phi[g], self.k, N, h, hs)
            self.psi[g] = ((self.psi[g].astype(np.uint64) + adv) & MASK).astype(np.uint32)
        self.phi[g] = q
        self.last = {"X": Xu, "mag": mag, "q": q, "peaks": P}
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
                Y = np.zeros(self.H, np.complex128)                                     # no peak: silence, reset or not
            else:
                Y = (Xu if G == 1 else np.fft.rfft((xs[i] * self.hann).astype(np.float64))) * rot
            fr = np.fft.irfft(Y, N).astype(np.float32) * self.hann
            full = np.concatenate([self.acc[c], np.zeros(hs, np.float32)]) + fr * self.scale
            self.acc[c] = full[hs:]
            out.append(full[:hs])
        return out

    def process_hops(self, x, hops, resets=None):
        """x: float32[nch, >= every row's total]; hops: int[T] or int[nch, T]; resets: None, 0/1[T] or 0/1[nch, T] (rows equal within a group)
        -> float32[nch, T hs]."""
        x = np.asarray(x, np.float32)
        nch = x.shape[0]
        rows = hop_rows(hops, nch)
        T = rows.shape[1]
        flags = flag_rows(resets, nch, T)
        y = np.zeros((nch, T * self.hs), np.float32)
        for g in range(nch // self.G):
            c0 = g * self.G
            for i in range(1, self.G):
                assert np.array_equal(rows[c0 + i], rows[c0]) and np.array_equal(flags[c0 + i], flags[c0]), "rows differ within a group"
            S = positions(rows[c0])
            assert S[-1] <= x.shape[1], (S[-1], x.shape)
            for m in range(T):
                outs = self.group_frame(g, [x[c0 + i, S[m]:S[m + 1]] for i in range(self.G)], bool(flags[c0, m]))
                for i in range(self.G):
                    y[c0 + i, m * self.hs:(m + 1) * self.hs] = outs[i]
        return y


# ---- identity in a hold ---------------------------------------------------------------------------------------------------------------------

def hold_schedule(N, ha, hs, pre, J):
    """(hops, resets, r): `pre` frames at ha, then frames r .. r + J at hs with the reset at r = pre, then `pre` frames at ha again."""
    hops = np.array([ha] * pre + [hs] * (J + 1) + [ha] * pre, np.int64)
    resets = np.zeros(hops.size, np.uint8)
    resets[pre] = 1
    return hops, resets, pre


def hold_identity(y, x, hops, N, hs, r, J):
    """Relative RMS of y - g(n) x[n + delta] over the output samples that only frames r .. r + J write, [(r - 1) hs + N, (r + J + 1) hs).  There
    frame m >= r contributes (hs / N) w^2(n - m hs) x[S[m + 1] - N + n - m hs], and with hops = hs from r on S[m + 1] = S[r + 1] + (m - r) hs: the
    input index is n + delta, delta = S[r + 1] - N - r hs, the same for every frame.  g is tones.envelope (every frame that covers n lies in the hold)."""
    S = positions(hops)
    lo, hi = (r - 1) * hs + N, (r + J + 1) * hs
    assert hi - lo >= hs, ("the hold is too short to own any output", lo, hi)
    delta = int(S[r + 1]) - N - r * hs
    n = np.arange(lo, hi)
    assert n[0] + delta >= 0
    want = TN.envelope(N, hs, hi)[lo:hi] * np.asarray(x, np.float64)[n + delta]
    got = np.asarray(y, np.float64)[lo:hi]
    return float(np.sqrt(np.mean((got - want) ** 2)) / np.sqrt(np.mean(want ** 2)))


# (N, ha, hs): halo = (N - 1) // hs of 2, 3, 6, 2, and from (512, 128, 16) on 31, 255, 3, 3, 127, 1, 1; ha = N (no carried history), hs = N / 2, hs = 1
HOLD_SHAPES = [(1024, 256, 384), (1024, 256, 320), (2048, 512, 300), (256, 100, 97), (512, 128, 16), (256, 8, 1), (4096, 1024, 1280),
               (8192, 2048, 2560), (8192, 1024, 64), (2048, 2048, 1024), (1024, 256, 512)]


def hold_base(N, ha, hs):
    """(J, pre) of the shortest hold case: 2 ceil(N / hs) + 4 held frames after the reset, ceil(N / ha) + 3 frames at ha on either side."""
    return 2 * -(-N // hs) + 4, -(-N // ha) + 3


# ---- a linked pair of tones ------------------------------------------------------------------------------------------------------------------

PAIR_AMPS, PAIR_PHASES = (0.5, 0.2), (0.4, 2.1)


def tone_pair_input(N, floor, hs, freq, kind="random", seed=0):
    """(hops, float32[2, sum hops]): one partial at `freq` bins in two channels with amplitudes PAIR_AMPS and phases PAIR_PHASES under a schedule
    floor .. N, long enough for 8 N of steady output (tempo_model.tone_schedule_input).  A linked pair keeps the phase difference 2.1 - 0.4."""
    from tempo_model import schedule
    lo, _ = TN.steady_range(N, floor, hs, 0)
    T = -(-(lo + 9 * N) // hs)
    hops = schedule(kind, floor, N, T, seed)
    n = int(hops.sum())
    return hops, np.stack([TN.partials(N, [freq], [a], [p], n) for a, p in zip(PAIR_AMPS, PAIR_PHASES)])


# ---- onset strength -------------------------------------------------------------------------------------------------------------------------

def frame_mags(u, N, ha):
    """float32[T, H]: mag of frame m of the buffer u (one row), window = the N samples that end at (m + 1) ha, zeros before the buffer."""
    u = np.asarray(u, np.float32)
    T = u.size // ha
    w = hann_f32(N)
    s = np.concatenate([np.zeros(N, np.float32), u])
    out = np.zeros((T, N // 2 + 1), np.float32)
    for m in range(T):
        X = np.fft.rfft((s[(m + 1) * ha:(m + 1) * ha + N] * w).astype(np.float64))
        out[m] = (X.real * X.real + X.imag * X.imag).astype(np.float32)
    return out


def onset_strength(u, N, ha, ulps=2):
    """(c int64[T], doubt int64[T]): c_m = #{k in [1, H - 1): mag_m[k] > 4 mag_{m-1}[k] and mag_m[k] > 2^-20 max_k mag_m}, frame -1 all zeros;
    doubt_m = the number of those bins where either comparison lies within `ulps` f32 ulps of a tie (another correctly rounded transform may count
    them the other way)."""
    mag = frame_mags(u, N, ha)
    T, H = mag.shape
    prev = np.concatenate([np.zeros((1, H), np.float32), mag[:-1]])
    a = mag[:, 1:H - 1]
    b = (np.float32(4.0) * prev[:, 1:H - 1]).astype(np.float32)
    fl = (mag.max(axis=1, keepdims=True) * np.float32(2.0 ** -20)).astype(np.float32) * np.ones_like(a)
    c = np.count_nonzero((a > b) & (a > fl), axis=1)

    def near(p, q):
        return np.abs(p.astype(np.float64) - q.astype(np.float64)) <= ulps * np.spacing(np.maximum(np.abs(p), np.abs(q)))
    # a bin near one tie can change the count only if the other comparison holds or is itself near a tie; all-zero bins (0 > 0) are no tie
    live = (a > 0) | (b > 0)
    doubt = np.count_nonzero(live & ((near(a, b) & ((a > fl) | near(a, fl))) | (near(a, fl) & ((a > b) | near(a, b)))), axis=1)
    return c.astype(np.int64), doubt.astype(np.int64)


def onsets_from_strength(c, N, ha, tau=0.4):
    """int64 positions m ha of the frames with c_m >= tau (H - 2) whose predecessor is below it (c_{-1} = 0)."""
    thr = tau * float(N // 2 - 1)
    above = np.asarray(c, np.float64) >= thr
    first = above & ~np.concatenate([[False], above[:-1]])
    return np.nonzero(first)[0].astype(np.int64) * ha


# ---- the planner ----------------------------------------------------------------------------------------------------------------------------

def transient_plan(onsets, n, N, ha, floor, hs, lead=None, release=None):
    """(hops int64[T], resets uint8[T], held bool[T]) by the rule of DESIGN.md "Phase resets" (pv_transient_plan)."""
    if hs < floor:
        raise ValueError("synthesis hop below the floor: a hold needs hop == hs to be legal")
    L = N // 8 if lead is None else int(lead)
    rel = N // 2 if release is None else int(release)
    if not 0 <= rel <= N:
        raise ValueError("release in 0 .. N")
    if not 0 <= L <= N // 2 or not floor <= ha <= N:
        raise ValueError("lead in 0 .. N/2, nominal hop in [floor, N]")
    onsets = np.asarray(onsets, np.int64)
    kappa = max(1, ha // 8)
    S, m, held_prev = 0, 0, False
    hops, resets, holds = [], [], []
    while True:
        tried = hs if held_prev else ha
        lo, hi = S + tried - N + L, S + tried - L
        held = bool(np.any((onsets >= lo - rel) & (onsets < hi)))          # the span [onset, onset + release] meets [lo, hi)
        hop = hs if held else min(max(ha - min(max(S - m * ha, -kappa), kappa), floor), N)
        if S + hop > n:
            break
        hops.append(hop)
        resets.append(1 if held and not held_prev else 0)
        holds.append(held)
        S, m, held_prev = S + hop, m + 1, held
    return np.array(hops, np.int64), np.array(resets, np.uint8), np.array(holds, bool)


# ---- test signals ---------------------------------------------------------------------------------------------------------------------------

BURST_DECAY = 120
# The background noise of the burst classes and the stationary-noise class: 30 dB below the bursts' initial RMS (1.0).  A burst's energy is
# BURST_DECAY / 2 = 60, so against the burst's power averaged over one frame of 1024 samples this is -18 dB: the level at which the measured D of the
# onsets (>= 0.92 / 0.70 / 0.75 at 1024/256, 2048/256, 4096/1024) is the design table's.  At sigma 0.1 (-20 dB re the initial RMS) D is 0.70 .. 0.76 at
# 1024/256 but 0.30 .. 0.34 at 2048/256 and 0.33 .. 0.49 at 4096/1024: below tau = 0.4, such bursts are missed (DESIGN.md "Phase resets").
NOISE_SIGMA = 10.0 ** -1.5


def bursts(n, onsets, seed=0, decay=BURST_DECAY, amp=1.0):
    """float64[n]: Gaussian noise bursts starting at `onsets`, each with envelope amp exp(-t / decay)."""
    rng = np.random.default_rng(seed)
    y = np.zeros(n)
    for o in onsets:
        t = np.arange(min(n - o, 12 * decay))
        y[o:o + t.size] += amp * rng.standard_normal(t.size) * np.exp(-t / decay)
    return y


def background(kind, n, N, seed=0):
    """float64[n]: 'silence', 'tones' (five partials of amplitude 0.1), 'noise' (Gaussian, sigma NOISE_SIGMA), 'vibrato' (the tones
    with an 8 rad phase vibrato at 5 cycles per 65536 samples)."""
    rng = np.random.default_rng(seed + 1000)
    k = np.arange(n, dtype=np.float64)
    if kind == "silence":
        return np.zeros(n)
    if kind == "noise":
        return NOISE_SIGMA * rng.standard_normal(n)
    freqs = np.array([0.031, 0.072, 0.113, 0.197, 0.301]) * N                 # in bins of N: N-independent frequencies in cycles per sample
    ph = rng.uniform(0, 2 * np.pi, freqs.size)
    vib = 8.0 * np.sin(2 * np.pi * 5 * k / 65536.0) if kind == "vibrato" else 0.0
    if kind in ("tones", "vibrato"):
        return sum(0.1 * np.cos(2 * np.pi * f / N * k + p + vib) for f, p in zip(freqs, ph))
    raise ValueError(kind)


# the five signal classes of the onset rule: (background, has bursts)
SIGNAL_CLASSES = {"bursts_tones": ("tones", True), "bursts_noise": ("noise", True), "bursts_silence": ("silence", True), "noise": ("noise", False),
                  "vibrato": ("vibrato", False)}


def class_signal(name, n, N, onsets, seed=0):
    bg, has = SIGNAL_CLASSES[name]
    y = background(bg, n, N, seed)
    if has:
        y = y + bursts(n, onsets, seed)
    return y.astype(np.float32)


def energy_spread(e, lo, hi):
    """Energy spread of the segment e[lo:hi] (a signal), in samples: the square root of the energy-weighted variance of the sample index."""
    p = np.asarray(e[lo:hi], np.float64) ** 2
    t = np.arange(p.size)
    c = np.sum(t * p) / np.sum(p)
    return float(np.sqrt(np.sum((t - c) ** 2 * p) / np.sum(p)))
