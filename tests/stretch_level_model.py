"""Parity at level for the time stretch: the yardstick, the corpus, the cases and the float32 restatement behind tests/test_stretch_level_model.py (CPU) and
tests/test_gpu_stretch_level.py (GPU).  TEST INFRASTRUCTURE, no GPU.  The counterpart of tests/level_model.py (the pitch shifter), whose metric it reuses.

The gates of tests/test_gpu_stretch_edges.py (relative RMS over a whole channel <= 5e-7, worst block RMS relative to the WHOLE reference's RMS <= 4e-6) are loud-weighted
and every signal they see is stationary and of order one: a passage 100 dB under a channel's loudest can be 1 % wrong without moving either.  Here every output block of
hs samples of every channel is held at its own level.

The level of a block.  Frame m of a channel is the Hann-windowed input x[S[m + 1] - N, S[m + 1]), S the prefix sum of the hops (S[m] = m ha at the fixed hop,
tempo_model.positions(hops) on a schedule; zeros before the stream).  The frame is overlap-added into output blocks m .. m + halo, halo = (N - 1) // hs.  So

    L(c, b) = max over m in [b - halo, b] of rms(window * frame m of channel c)         in float64, from the test's own input,

per channel also in a linked group (every channel inverts its own spectrum).  Block metric: rms(y - ref over the block) / L <= K_rms and max|y - ref| / L <= K_max; where
L == 0 both blocks are exactly 0 (level_model.hop_metrics with hop = hs).

K_rms and K_max are never fitted to a kernel.  `restate` is a plain float32 restatement of the SYNTHESIS half of the reference models (stretch_model.py, tempo_model.py,
link_model.py, transient_model.py): it drives the fp64 model frame by frame and takes the model's own X, peak regions P, q and psi, so that no decision can flip; then an
f32 rotation (cos / sin of 2 pi (psi[P] - q[P]) / 2^32 rounded to f32), a complex64 product, level_model.fft32 as the inverse with an f32 1 / N, and f32 window, hs / N
scale and accumulator.  Its own worst rms / L and max / L against the models over the corpus are pinned below per FFT size (tests/test_stretch_level_model.py reproduces
them); the GPU gate is level_model.GATE_FACTOR times those.
"""
import functools
import types

import numpy as np

import level_model as LM
import signals as S
from link_model import LinkModel, mix
from stretch_model import TWO32, StretchModel, hann_f32
from tempo_model import TempoModel, positions, schedule
from transient_model import TransientModel

NCH = 3

# The restatement's own worst (rms / L, max / L) against the reference models, per FFT size, over every block of every channel of every case of case_list() below (fixed hop
# and families).  Measured by tests/test_stretch_level_model.py::test_restatement_figures_are_pinned_and_reproduced, plus 3 % and rounded up to two digits; the test
# asserts the restatement stays under them and within a factor 1.25.
RESTATEMENT_FIGURES = {
    256: (1.6e-7, 4.4e-7),       # measured 1.540e-07, 4.185e-07   (rms / L at 256/7/8, halo 31)
    512: (8.0e-8, 6.1e-7),       # measured 7.719e-08, 5.836e-07
    1024: (1.5e-7, 4.7e-7),      # measured 1.445e-07, 4.472e-07   (rms / L at 1024/7/8, halo 127)
    2048: (7.7e-8, 4.6e-7),      # measured 7.431e-08, 4.465e-07
    4096: (8.0e-8, 5.4e-7),      # measured 7.727e-08, 5.160e-07
    8192: (6.8e-8, 4.7e-7),      # measured 6.520e-08, 4.474e-07
}

SIGNALS = ("fade", "burst", "quiet_mid", "quiet_first", "quiet_last", "scaled_up", "scaled_down", "loud_partial")
# (N, ha, hs, frames or None, signals): the fixed-hop shapes
FIXED_SHAPES = [
    (256, 64, 80, None, SIGNALS),
    (256, 7, 8, 400, SIGNALS),                      # halo 31
    (512, 100, 97, None, SIGNALS),
    (512, 32, 256, 160, SIGNALS),                   # hs = N / 2
    (1024, 256, 320, None, SIGNALS),
    (1024, 256, 128, None, SIGNALS),
    (1024, 7, 8, 1200, ("fade", "burst")),          # halo 127
    (2048, 512, 1024, None, SIGNALS),
    (4096, 1024, 1280, None, SIGNALS),
    (8192, 2048, 1536, None, SIGNALS),
]
FAMILY_SHAPES = [(256, 64, 80), (1024, 256, 320), (4096, 1024, 1280), (256, 7, 8)]
# family -> signals.  sched: a random schedule in [floor, N] (TempoModel); resets: the same with two reset flags (TransientModel); link3: G = 3 at the fixed hop
# (LinkModel), the -100 dB channel rotated by angles the full-scale one sets; link2s: G = 2 on the schedule, the first two channels of the signal.
FAMILIES = {"sched": ("fade", "burst", "quiet_mid"), "resets": ("fade", "burst", "quiet_mid"), "link3": ("quiet_mid", "quiet_first", "quiet_last"),
            "link2s": ("fade", "burst", "quiet_mid")}


# the cases of the exact-scaling test: `fade` at the fixed hop, and one linked schedule
SCALING_CASES = [("fixed", 1024, 256, 320, "fade"), ("fixed", 4096, 1024, 1280, "fade"), ("link2s", 1024, 256, 320, "fade")]


def gate(N):
    """(K_rms, K_max) the kernels are held to at FFT size N."""
    r, m = RESTATEMENT_FIGURES[N]
    return LM.GATE_FACTOR * r, LM.GATE_FACTOR * m


def halo_of(N, hs):
    return (N - 1) // hs


def chain_floor(N, hs):
    """The shortest chain of a launch: four times the halo + 1 frames a chain recomputes (pv_stretch_capi.hip, pick_chain).  A call whose frames per channel do not
    outnumber the chains the chip holds at once runs at this length; the GPU tests read the length the handle reports."""
    return 4 * (halo_of(N, hs) + 1)


def frames(N, ha, hs, listed=None):
    """The frames of a case: the listed count, or level_model.nhops(N) lengthened to three chains at the shortest chain length (the rule of
    test_gpu_stretch_edges._frames without its floor of 64)."""
    if listed is not None:
        return listed
    F0 = chain_floor(N, hs)
    return max(LM.nhops(N), 2 * F0 + F0 // 2 + 1)


def shape_frames(N, ha, hs):
    for n, a, s, listed, _ in FIXED_SHAPES:
        if (n, a, s) == (N, ha, hs):
            return frames(N, ha, hs, listed)
    return frames(N, ha, hs)


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------------------

def burst_layout(N, Spos, hs):
    """(first silent sample, one past the last, B): the silence of `burst` is placed so that the frames B - halo - 1 .. B + 1 hold only zeros, B the first multiple of
    the shortest chain length that leaves three hops of the loud part before it: blocks B - 1, B and B + 1 have L == 0, and a launch at the shortest chain length starts
    a chain on the middle one."""
    halo, F0 = halo_of(N, hs), chain_floor(N, hs)
    T = len(Spos) - 1
    B = F0
    while B + 2 <= T and int(Spos[B - halo]) - N < int(Spos[3]):
        B += F0
    assert B + 2 < T, ("the stream is too short for the silence of burst", N, hs, T, B)
    return int(Spos[B - halo]) - N, int(Spos[B + 2]), B


def stretch_corpus(N, ha_or_hops, T, hs):
    """name -> float32[NCH, S[T]]: the signals of level_model.corpus, sized by the input that T frames consume (level_model.corpus(N, hop) is 48 hops long, shorter than
    one frame at a hop of 7 or 8).  ha_or_hops: the fixed analysis hop, or the schedule int[T]."""
    hops = np.full(T, int(ha_or_hops), np.int64) if np.ndim(ha_or_hops) == 0 else np.asarray(ha_or_hops, np.int64)
    assert hops.size == T
    Spos = positions(hops)
    n = int(Spos[-1])
    out = {}
    fade = LM._material(1, n, 11) * LM._fade_gain(n)                          # the -140 dB parabola
    out["fade"] = fade
    b = LM._material(1, n, 12)
    s0, s1, B = burst_layout(N, Spos, hs)
    b[:, s0:s1] = 0.0                                                       # digital silence: halo + 3 frames hold nothing else
    b[:, s1:] *= 1e-5                                                       # the -100 dB tone
    assert np.count_nonzero(Spos[1:] - N >= s1) >= 5, "burst: fewer than five frames lie wholly in the quiet tone"
    out["burst"] = b
    q = LM._material(1, n, 13)
    gains = {"quiet_mid": (1.0, 1e-5, 1e-3), "quiet_first": (1e-5, 1.0, 1e-3), "quiet_last": (1e-3, 1.0, 1e-5)}
    for name, g in gains.items():
        out[name] = q * np.asarray(g)[:, None]
    out["scaled_up"] = fade * 2.0 ** 20
    out["scaled_down"] = fade * 2.0 ** -20
    i = np.arange(n, dtype=np.float64)
    out["loud_partial"] = np.stack([0.5 * np.sin(2 * np.pi * (0.0731 + 0.011 * c) * i)
                                    + S.lcg_noise(3000 + c, n, 0.5 * 10.0 ** (-110.0 / 20.0)).astype(np.float64) for c in range(NCH)])
    out = {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------------------

def frames_at(x, Spos, N, dtype=np.float32, hist=None):
    """[nch, T, N]: frame m = x[S[m + 1] - N, S[m + 1]); before the stream zeros, or hist (float32[nch, >= N - S[1]], the imported history)."""
    x = np.asarray(x)
    pre = np.zeros(x.shape[:-1] + (N,), x.dtype)
    if hist is not None:
        h = np.asarray(hist, x.dtype)
        pre[..., N - h.shape[-1]:] = h
    xp = np.concatenate([pre, x], axis=-1)
    idx = np.asarray(Spos[1:], np.int64)[:, None] + np.arange(N)[None, :]
    return xp[..., idx].astype(dtype)


def block_levels(x, Spos, N, hs, hist=None):
    """(L float64[nch, T], the frames' own rms float64[nch, T])."""
    w = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N))
    f = frames_at(x, Spos, N, np.float64, hist) * w
    fr = np.sqrt(np.mean(f * f, axis=-1))
    L = fr.copy()
    for j in range(1, min(halo_of(N, hs), fr.shape[1] - 1) + 1):
        L[:, j:] = np.maximum(L[:, j:], fr[:, :-j])
    return L, fr


def silent_frames(x, Spos, N, G=1, hist=None):
    """bool[nch / G, T]: the window of the group's mix holds only zeros.  No transform can decide such a frame differently (X is exactly 0, there is no peak), although
    stretch_model.doubtful_frame calls it doubtful: every comparison of its magnitudes is a tie."""
    u = mix(x, G)
    uh = None if hist is None else mix(hist, G)
    return ~np.any(frames_at(u, Spos, N, np.float32, uh) != 0, axis=-1)


def skip_blocks(doubt, N, hs):
    """bool[nch, T]: the blocks m .. m + halo a doubtful frame m reaches (what test_gpu_stretch_edges.block_gate leaves out)."""
    skip = np.zeros(doubt.shape, bool)
    for c, m in np.argwhere(doubt):
        skip[c, m:m + halo_of(N, hs) + 1] = True
    return skip


def block_failures(y, ref, L, hs, k_rms, k_max, skip=None):
    """([(channel, block, rms / L, max / L)] of the blocks that miss the gate, worst (rms / L, max / L)) over the blocks outside `skip`."""
    rr, mm = LM.hop_metrics(y, ref, L, hs)
    if skip is not None:
        rr, mm = np.where(skip, 0.0, rr), np.where(skip, 0.0, mm)
    bad = np.argwhere((rr > k_rms) | (mm > k_max))
    return [(int(c), int(b), float(rr[c, b]), float(mm[c, b])) for c, b in bad], (float(rr.max()), float(mm.max()))


def zero_blocks_exact(y, L, hs):
    """Every block with L == 0 is exactly 0 in y."""
    nch, T = L.shape
    return not np.any(np.asarray(y).reshape(nch, T, hs)[L == 0] != 0)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------------

def case_list():
    """[(family, N, ha, hs, signal)] of every case the GPU file runs."""
    out = [("fixed", N, ha, hs, s) for N, ha, hs, _, sigs in FIXED_SHAPES for s in sigs]
    out += [(fam, N, ha, hs, s) for fam, sigs in FAMILIES.items() for N, ha, hs in FAMILY_SHAPES for s in sigs]
    return out


def case_id(c):
    return "-".join(str(v) for v in c)


def reference(family, N, ha, hs, x, hops, resets):
    """(the reference's output, its doubtful flags bool[groups, T]) of one case, from the model the family is defined by."""
    nch = x.shape[0]
    if family == "fixed":
        m = StretchModel(N, ha, hs, nch, track_doubt=True)
        y = m.process(x)
    elif family == "sched":
        m = TempoModel(N, ha, hs, nch, track_doubt=True)
        y = m.process_hops(x, hops)
    elif family == "resets":
        m = TransientModel(N, ha, hs, nch, 1, track_doubt=True)
        y = m.process_hops(x, hops, resets)
    elif family == "link3":
        m = LinkModel(N, ha, hs, nch, 3, track_doubt=True)
        y = m.process(x)
    elif family == "link2s":
        m = LinkModel(N, ha, hs, nch, 2, track_doubt=True)
        y = m.process_hops(x, hops)
    else:
        raise ValueError(family)
    return y, np.asarray(m.doubtful, bool)


@functools.lru_cache(maxsize=None)
def case(family, N, ha, hs, signal):
    """One case, with everything the model alone says about it: T, G, x, hops / resets (None at the fixed hop), the burst's block B, the cuts of the three-call form,
    ref, L, the frames' rms, doubt_raw and silent (bool[groups, T]: the model's flags, the frames whose window holds only zeros), doubt (bool[nch, T]: the NON-SILENT doubtful frames, a group's flags on each of its channels) and skip (the blocks they reach)."""
    T = shape_frames(N, ha, hs)
    G = {"link3": 3, "link2s": 2}.get(family, 1)
    hops = schedule("random", ha, N, T, seed=N) if family in ("sched", "resets", "link2s") else None
    Spos = positions(np.full(T, ha, np.int64) if hops is None else hops)
    B = burst_layout(N, Spos, hs)[2]
    x = stretch_corpus(N, ha if hops is None else hops, T, hs)[signal]
    if family == "link2s":
        x = np.ascontiguousarray(x[:2])
    resets = None
    if family == "resets":
        resets = np.zeros(T, np.uint8)
        resets[[B + 2, T // 2]] = 1                                          # the first frame after the silence of burst, and the bottom of fade
    ref, raw = reference(family, N, ha, hs, x, hops, resets)
    silent = silent_frames(x, Spos, N, G)
    dm = raw & ~silent
    doubt = np.repeat(dm, G, axis=0)
    L, fr = block_levels(x, Spos, N, hs)
    cuts = (0, B + 1, T // 2, T)                                             # a cut inside the silence of burst (off the chain boundary B), one at the bottom of fade
    assert cuts[1] < cuts[2] < cuts[3]
    for a in (x, ref, L):
        a.setflags(write=False)
    return types.SimpleNamespace(family=family, N=N, ha=ha, hs=hs, signal=signal, T=T, G=G, nch=x.shape[0], x=x, hops=hops, resets=resets, S=Spos, B=B, cuts=cuts,
                                 ref=ref, L=L, frame_rms=fr, doubt_raw=raw, silent=silent, doubt=doubt, skip=skip_blocks(doubt, N, hs))


def doubt_count(c):
    """(non-silent doubtful frames, frames) of a case, over all its channels (groups, where linked: doubt is judged on the mix)."""
    return int(c.doubt[::c.G].sum()), c.T * c.nch // c.G


def doubt_cap(frames):
    """At most 1 % of a case's frames plus one may be doubtful."""
    return 0.01 * frames + 1


# ---- the float32 restatement of the synthesis half ----------------------------------------------------------------------------------------------------

def restate(N, floor, hs, x, hops=None, resets=None, G=1):
    """(y32, yref): the restatement's output and the output of the fp64 model it follows, both float32[nch, T hs].  The model is TransientModel, which is StretchModel
    at a fixed hop, TempoModel on a schedule and LinkModel in groups (tests/test_stretch_level_model.py holds its output to theirs bit for bit); it is driven frame by
    frame and its decisions and integers are read back after each frame."""
    x = np.asarray(x, np.float32)
    nch, n = x.shape
    hops = np.full(n // floor, floor, np.int64) if hops is None else np.asarray(hops, np.int64)
    T, H = hops.size, N // 2 + 1
    flags = np.zeros(T, bool) if resets is None else np.asarray(resets).astype(bool)
    Spos = positions(hops)
    hann = hann_f32(N)
    xw = frames_at(x, Spos, N, np.float32) * hann                              # f32, as the model's x * hann
    m = TransientModel(N, floor, hs, nch, G)
    yref = np.zeros((nch, T * hs), np.float32)
    Y = np.zeros((nch, T, N), np.complex64)
    for g in range(nch // G):
        for t in range(T):
            outs = m.group_frame(g, [x[g * G + i, Spos[t]:Spos[t + 1]] for i in range(G)], bool(flags[t]))
            for i in range(G):
                yref[g * G + i, t * hs:(t + 1) * hs] = outs[i]
            P, q, psi = m.last["peaks"], m.last["q"], m.psi[g]
            if P[0] < 0:
                continue                                                     # no peak: silence
            s = (psi[P].astype(np.int64) - q[P].astype(np.int64)) & 0xFFFFFFFF
            s = np.where(s >= 1 << 31, s - TWO32, s)
            th = 2.0 * np.pi * s.astype(np.float64) / TWO32
            rot = (np.cos(th).astype(np.float32) + 1j * np.sin(th).astype(np.float32)).astype(np.complex64)
            for i in range(G):
                c = g * G + i
                X = m.last["X"] if G == 1 else np.fft.rfft(xw[c, t].astype(np.float64))
                Y[c, t, :H] = X.astype(np.complex64) * rot
    k = np.arange(1, N // 2)
    Y[..., N - k] = np.conj(Y[..., k])
    assert Y.dtype == np.complex64
    fr = LM.fft32(Y, inverse=True).real * np.float32(1.0 / N)
    fr = (fr * hann) * np.float32(hs / N)
    assert fr.dtype == np.float32
    y = np.zeros((nch, T * hs), np.float32)
    acc = np.zeros((nch, N), np.float32)
    for t in range(T):
        acc = acc + fr[:, t]
        y[:, t * hs:(t + 1) * hs] = acc[:, :hs]
        acc = np.concatenate([acc[:, hs:], np.zeros((nch, hs), np.float32)], axis=1)
    return y, yref


def restate_case(c):
    return restate(c.N, c.ha, c.hs, c.x, c.hops, c.resets, c.G)


# ---- exact scaling ------------------------------------------------------------------------------------------------------------------------------------

def scaling_conditions(c, ks=(-20, 0, 20)):
    """(smallest, largest) non-zero value, over the runs of case c with its input scaled by 2^k, k in ks, of everything the kernels round to float32 on the way: the
    windowed input, the squared magnitudes (fp64 sum, stored as f32), and each component of the spectra X that the rotation reads as f32.  A power of two commutes with
    every rounding as long as these stay in the float32 normal range [2^-126, 2^128); an exact 0 scales to itself."""
    lo, hi = [np.inf, np.inf], [0.0, 0.0]                                      # [values that scale by 2^k, squared magnitudes: by 4^k]
    hann = hann_f32(c.N)
    xw = (frames_at(c.x, c.S, c.N, np.float32) * hann).astype(np.float64)
    X = np.fft.rfft(xw, axis=-1)
    if c.G > 1:
        X = np.concatenate([X, np.fft.rfft((frames_at(mix(c.x, c.G), c.S, c.N, np.float32) * hann).astype(np.float64), axis=-1)])
    for j, v in ((0, np.abs(xw)), (0, np.abs(X.real)), (0, np.abs(X.imag)), (1, X.real * X.real + X.imag * X.imag)):
        nz = v[v > 0]
        lo[j], hi[j] = min(lo[j], float(nz.min())), max(hi[j], float(nz.max()))
    k0, k1 = min(ks), max(ks)
    return min(lo[0] * 2.0 ** k0, lo[1] * 4.0 ** k0), max(hi[0] * 2.0 ** k1, hi[1] * 4.0 ** k1)
