"""CPU model of the variable-ratio band-limited resampler (VariResampler / pv_vari_*): plain numpy, fp64.  TEST INFRASTRUCTURE ONLY.

The normative definition (DESIGN.md "Pitch curves"):
  blocks of B input samples, block b emits c = counts[b] outputs, min_count <= c <= max_count; 1 <= B <= 4096, 1 <= min_count <= max_count <= 8192,
  B <= 8 min_count, max_count <= 8 B; W = ceil(32 max(1, B / min_count)) in integers, T = 2 W;
  output k of stream block b: n = b B + (k B) div c, r = (k B) mod c; tap i = 0 .. T - 1 reads x[n - 2 W + 1 + i] (x zero before the stream) at
  a = |(i - W + 1) c - r| units of 1 / c sample from the output position b B + k B / c - W;
  prototype P[q] = f32(h0(q / Q)), h0(t) = 0.91 sinc(0.91 t) I0(9 sqrt(1 - (t / 32)^2)) / I0(9), q = 0 .. 32 Q - 1, Q = 256; P[q] = 0 from 32 Q on;
  den = max(B, c): q = (a Q) div den, f = ((a Q) mod den) / den, w = P[q] + f (P[q + 1] - P[q]), 0 when q >= 32 Q;
  y = (sum_i w_i x_i) / (sum_i w_i).
The model forms the weights and the sums in fp64 from the f32 table (the integers are exact either way); the kernel's f32 roundings are what the
GPU tests bound.  Nothing here is taken from the reference: the reference leaves resampling to the browser's player.
"""
import numpy as np

BETA = 9.0
CUTOFF = 0.91
HALF_WIDTH = 32
Q = 256
TABLE = HALF_WIDTH * Q + 2
MAX_BLOCK = 4096
MAX_COUNT = 8192


def half_width(block, min_count, max_count):
    """W, or ValueError: what pv_vari_create accepts."""
    B, lo, hi = int(block), int(min_count), int(max_count)
    if not 1 <= B <= MAX_BLOCK:
        raise ValueError("block outside [1, 4096]")
    if not 1 <= lo <= hi <= MAX_COUNT:
        raise ValueError("counts need 1 <= min_count <= max_count <= 8192")
    if B > 8 * lo or hi > 8 * B:
        raise ValueError("the step block / count must lie within [1/8, 8]")
    return -(-HALF_WIDTH * max(B, lo) // lo)


def h0(t):
    """The continuous prototype on |t| <= 32 (fp64), 0 outside."""
    t = np.abs(np.asarray(t, np.float64))
    arg = np.sqrt(np.clip(1.0 - (t / HALF_WIDTH) ** 2, 0.0, None))
    return np.where(t < HALF_WIDTH, CUTOFF * np.sinc(CUTOFF * t) * np.i0(BETA * arg) / np.i0(BETA), 0.0)


def prototype():
    """P f32[8194]: h0 at q / Q for q < 32 Q, zeros from 32 Q on."""
    P = np.zeros(TABLE, np.float32)
    P[:HALF_WIDTH * Q] = h0(np.arange(HALF_WIDTH * Q) / Q).astype(np.float32)
    return P


def weights(B, c, r, W, table, exact=False):
    """fp64[len(r), T]: the weights of outputs with remainders r in a block of count c.  exact=True: h0 itself at the taps' distances, no table.
    Also returns |f (P[q + 1] - P[q])|, the part of each weight that carries the roundings of the interpolation."""
    T = 2 * W
    i = np.arange(T, dtype=np.int64)[None, :]
    a = np.abs((i - W + 1) * int(c) - np.asarray(r, np.int64)[:, None])
    den = max(int(B), int(c))
    if exact:
        return h0(a.astype(np.float64) * (1.0 / den)), None         # a / c samples, stretched by c / den: the argument of h0 is a / den
    aq = a * Q
    q = aq // den
    f = (aq % den).astype(np.float64) / den
    qc = np.minimum(q, HALF_WIDTH * Q)
    P = np.asarray(table, np.float64)
    d = P[qc + 1] - P[qc]
    return P[qc] + f * d, np.abs(f * d)


def nonzero_weights(B, c, r, W, table):
    """bool[len(r), T]: the taps whose weight is non-zero IN THE KERNEL'S ARITHMETIC, w = fmaf(f32(rem) * (1.0f / f32(den)), P[q + 1] - P[q], P[q]).  The
    product and the sum are evaluated in fp64 from the f32 operands f^ = fl(rem * fl(1 / den)) and d^ = fl(P[q + 1] - P[q]): f^ d^ is exact in fp64
    (24 + 24 bits), and an exact f^ d^ + P[q] that is not zero is a multiple of 2^-298 no smaller than that, far inside the fp64 range, so the rounded
    fp64 sum is zero exactly when the fused f32 operation gives zero.  (The model's own fp64 f = rem / den would answer another question.)"""
    T = 2 * W
    i = np.arange(T, dtype=np.int64)[None, :]
    a = np.abs((i - W + 1) * int(c) - np.asarray(r, np.int64)[:, None])
    den = max(int(B), int(c))
    aq = a * Q
    q = np.minimum(aq // den, HALF_WIDTH * Q)
    P = np.asarray(table).astype(np.float32)
    f = (aq % den).astype(np.float32) * (np.float32(1.0) / np.float32(den))
    d = P[q + 1] - P[q]
    assert f.dtype == np.float32 and d.dtype == np.float32
    return f.astype(np.float64) * d.astype(np.float64) + P[q].astype(np.float64) != 0.0


class VariModel:
    """One pv_vari handle with `nch` channel slots.  `table`: another f32[8194] in place of the model's own (the GPU tests pass the library's)."""

    def __init__(self, block, min_count, max_count, nch=1, table=None):
        self.W = half_width(block, min_count, max_count)
        self.T = 2 * self.W
        self.B, self.min_count, self.max_count = int(block), int(min_count), int(max_count)
        self.table = (prototype() if table is None else np.asarray(table, np.float32)).astype(np.float64)
        assert self.table.size == TABLE
        self.hist = np.zeros((nch, self.T - 1), np.float32)
        self.blocks = 0
        self.outputs = 0

    def process(self, x, counts, bound=False, exact=False, reach=False):
        """x: float32[nch, nblocks B], counts int[nblocks] -> fp64[nch, sum(counts)].  bound=True: also, per output sample, A = sum_i m_i |x_i|,
        S = sum_i m_i with m_i = |w_i| + |f_i (P[q_i + 1] - P[q_i])| >= |w_i|, D = sum_i w_i (one row: the weights are the same in every channel) and
        Tloc, the number of non-zero weights.
        reach=True: the rule for non-finite input (pv_vari.h).  Every sample that is not finite, in the carried history or in x, counts as 0 in y (and
        in A), and two bool[nch, total] are appended to the result: `poisoned`, the outputs with such a sample under a tap whose weight is non-zero
        in the kernel's own arithmetic (nonzero_weights) -- the kernel gives a non-finite value exactly there -- and `near`, the outputs with such a
        sample anywhere under their T taps.  The history keeps the samples as they came.  Without reach a non-finite sample poisons whatever fp64
        makes of it (0 * nan): that is no statement about the kernel."""
        x = np.asarray(x, np.float32)
        if x.ndim == 1:
            x = x[None, :]
        counts = np.asarray(counts, np.int64)
        nch, nin = x.shape
        B, W, T = self.B, self.W, self.T
        assert nin == counts.size * B and np.all((counts >= self.min_count) & (counts <= self.max_count))
        raw = np.concatenate([self.hist[:nch], x], axis=1)                             # raw[:, e] = call-relative input index e - (T - 1)
        bad = ~np.isfinite(raw) if reach else None
        buf = (np.where(bad, np.float32(0.0), raw) if reach else raw).astype(np.float64)
        total = int(counts.sum())
        y = np.zeros((nch, total), np.float64)
        A = np.zeros((nch, total), np.float64)
        S, D, Tloc = np.zeros(total, np.float64), np.zeros(total, np.float64), np.zeros(total, np.int64)
        poisoned, near = np.zeros((nch, total), bool), np.zeros((nch, total), bool)
        at = 0
        for b, c in enumerate(counts.tolist()):
            k = np.arange(c, dtype=np.int64)
            n = b * B + (k * B) // c
            r = (k * B) % c
            step = max(1, (1 << 21) // T)
            for s in range(0, c, step):
                w, fd = weights(B, c, r[s:s + step], W, self.table, exact)
                idx = n[s:s + step, None] + np.arange(T)[None, :]                      # tap i reads index n - 2 W + 1 + i, i.e. buf[n + i]
                m = np.abs(w) + (fd if fd is not None else 0.0)
                sl = slice(at + s, at + s + w.shape[0])
                D[sl] = w.sum(axis=1)
                S[sl] = m.sum(axis=1)
                Tloc[sl] = (w != 0.0).sum(axis=1)
                nz = nonzero_weights(B, c, r[s:s + step], W, self.table) if reach else None
                for ch in range(nch):
                    xv = buf[ch][idx]
                    y[ch, sl] = (w * xv).sum(axis=1) / D[sl]
                    if bound:
                        A[ch, sl] = (m * np.abs(xv)).sum(axis=1)
                    if reach and bad[ch].any():
                        poisoned[ch, sl] = (nz & bad[ch][idx]).any(axis=1)
                        near[ch, sl] = bad[ch][idx].any(axis=1)
            at += c
        self.hist[:nch] = raw[:, raw.shape[1] - (T - 1):]
        self.blocks += counts.size
        self.outputs += total
        res = (y, A, S, D, Tloc) if bound else (y,)
        if reach:
            res += (poisoned, near)
        return res if len(res) > 1 else y


def positions(block, counts, W):
    """fp64 input positions of every output of a stream that starts with these counts: b B + k B / c - W."""
    out = []
    for b, c in enumerate(np.asarray(counts, np.int64).tolist()):
        out.append(b * block + np.arange(c, dtype=np.float64) * block / c - W)
    return np.concatenate(out) if out else np.zeros(0)
