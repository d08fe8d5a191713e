"""CPU model of the variable-tempo time stretch (TimeStretch.process_hops / pv_tempo_*): StretchModel with a per-frame analysis hop.  TEST INFRASTRUCTURE ONLY.

Frame m of a channel consumes hops[m] >= the floor (the handle's analysis_hop) input samples and emits hs output samples.  Its window is the newest N
samples of the stream, and hops[m] takes the place of ha in the phase advance; everything else is StretchModel.frame (DESIGN.md "Time stretch",
"Variable tempo").  The carried history stays N - floor samples long, which is what any hop >= floor needs.
"""
import numpy as np

import tones as TN
from stretch_model import StretchModel


def positions(hops):
    """int64[nframes + 1]: S[0] = 0, S[m + 1] = S[m] + hops[m], the input consumed before frame m (frame m's window ends at S[m + 1])."""
    return np.concatenate([[0], np.cumsum(np.asarray(hops, np.int64))])


def hop_rows(hops, nch):
    """int64[nch, nframes] from a shared row (1-D) or per-channel rows (2-D)."""
    hops = np.asarray(hops, np.int64)
    if hops.ndim == 1:
        return np.broadcast_to(hops, (nch, hops.size))
    assert hops.shape[0] == nch, hops.shape
    return hops


class TempoModel(StretchModel):
    """One pv_stretch handle with `nch` channel slots and analysis hop floor `floor`, run with per-frame hops.  `frame(c, block)` takes the hop from
    len(block); `process` (the fixed-hop call) is the schedule with every hop equal to the floor."""

    def __init__(self, N, floor, hs, nch=1, track_doubt=False):
        super().__init__(N, floor, hs, nch, track_doubt)
        self.floor = floor
        self.hist = [h.copy() for h in self.hist]        # rows: N - hop long for the duration of a frame, N - floor between frames

    def frame(self, c, block):
        N, h = self.N, len(block)
        if not self.floor <= h <= N:
            raise ValueError(f"hop {h} outside [{self.floor}, {N}]")
        full = np.concatenate([self.hist[c], np.asarray(block, np.float32)])
        self.hist[c] = full[full.size - N:full.size - h]  # the N - h samples before the block: StretchModel.frame windows hist ++ block
        self.ha = h
        try:
            y = super().frame(c, block)
        finally:
            self.ha = self.floor
        self.hist[c] = full[full.size - (N - self.floor):]
        return y

    def process_hops(self, x, hops):
        """x: float32[nch, >= every row's total]; hops: int[nframes] (every channel) or int[nch, nframes] -> float32[nch, nframes * hs]."""
        x = np.asarray(x, np.float32)
        nch = x.shape[0]
        rows = hop_rows(hops, nch)
        T = rows.shape[1]
        y = np.zeros((nch, T * self.hs), np.float32)
        for c in range(nch):
            S = positions(rows[c])
            assert S[-1] <= x.shape[1], (S[-1], x.shape)
            for m in range(T):
                y[c, m * self.hs:(m + 1) * self.hs] = self.frame(c, x[c, S[m]:S[m + 1]])
        return y


def frame_spans(S, N, hs):
    """Per frame m: (first input sample of its window, one past its last) = (S[m + 1] - N, S[m + 1]), and the output its N samples overlap-add into,
    [m hs, m hs + N) (the output of frame m's call starts with them: acc holds what earlier frames left for it)."""
    S = np.asarray(S, np.int64)
    m = np.arange(S.size - 1, dtype=np.int64)
    return S[1:] - N, S[1:], m * hs, m * hs + N


def switch_bounds(S, N, hs, P):
    """For input that switches signal at sample P: (end of the output no frame whose window reaches P writes to, start of the output no frame whose
    window still holds input before P writes to).  Before the first bound the output can hold only the old signal, after the second only the new."""
    w0, w1, o0, o1 = frame_spans(S, N, hs)
    first = int(np.argmax(w1 > P))                      # the first frame whose window reaches P
    last = int(np.nonzero(w0 < P)[0].max())             # the last frame whose window holds input before P
    return int(o0[first]), int(o1[last])


def schedule(kind, floor, top, T, seed=0):
    """int64[T]: 'ramp' floor -> top, 'random' uniform in [floor, top], 'alt' floor and top in turn."""
    if kind == "ramp":
        return np.rint(np.linspace(floor, top, T)).astype(np.int64)
    if kind == "random":
        return np.random.default_rng(seed).integers(floor, top + 1, T)
    if kind == "alt":
        return np.where(np.arange(T) % 2 == 0, floor, top).astype(np.int64)
    raise ValueError(kind)


# (N, floor, hs, partials, amplitudes): the fixed-hop tone cases' shapes with the floor as the onset bound; the schedule's top is N
TONE_SHAPES = {
    "256-32-80": (256, 32, 80, [40.3], [0.5]),
    "1024-205-320": (1024, 205, 320, [64.37], [0.5]),
    "1024-128-384": (1024, 128, 384, [64.37], [0.5]),
    "2048-256-256": (2048, 256, 256, [300.6], [0.5]),
    "4096-512-1024": (4096, 512, 1024, [700.2], [0.5]),
    "8192-1024-2560": (8192, 1024, 2560, [1000.37], [0.5]),
}


# The hop edges (tests/test_gpu_stretch_families.py): halo = (N - 1) // hs of 127, 255, 5, 1, 20, 127, 1, floors that do not divide N, hs = N / 2 and
# hs = 1, with the partials of tones.CASES.  The model's own error is <= 4.1e-7 under every schedule kind but 512-32-256 "alt" (9.2e-7).  256-1-8 is
# left out: the model itself gives 2.3e-6 ("random") and 4.0e-6 ("alt") there, the algorithm at hop 1 after hop 256, above the gate of 3e-6.
TONE_SHAPES_EDGES = {
    "1024-7-8": (1024, 7, 8, [64.37], [0.5]),
    "256-8-1": (256, 8, 1, [40.3], [0.5]),
    "512-100-97": (512, 100, 97, [77.7], [0.5]),
    "512-32-256": (512, 32, 256, [77.7], [0.5]),
    "2048-256-100": (2048, 256, 100, [300.6], [0.5]),
    "8192-1024-64": (8192, 1024, 64, [1000.37], [0.5]),
    "4096-64-2048": (4096, 64, 2048, [700.2], [0.5]),
}


def tone_schedule_input(N, floor, hs, freqs, amps, kind, seed=0):
    """(hops, float32[sum hops]): enough frames for 8 N of steady output (tones.steady_range with the floor)."""
    lo, _ = TN.steady_range(N, floor, hs, 0)
    T = -(-(lo + 9 * N) // hs)
    hops = schedule(kind, floor, N, T, seed)
    rng = np.random.default_rng(seed)
    return hops, TN.partials(N, freqs, amps, rng.uniform(0, 2 * np.pi, len(freqs)), int(hops.sum()))
