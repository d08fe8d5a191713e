"""numpy / int64 restatement of the f0 tracker (pv_f0_track), of the period (pv_f0_period) and of the pitch-correction planner (pv_tune_plan), as
DESIGN.md "Pitch tracking" states them.  Every record value is an exact integer function of the frame's samples, so the device is compared with `==`;
the planner uses math.log2 and 2.0 ** r, the libm functions the library calls, and is compared exactly too."""
import math

import numpy as np

C_ONE = 1 << 14
DEFAULT_THRESHOLD = 2458


def quantise(frame):
    """int64 q of one frame (float32[W + max_lag]), or None for silence or a non-finite sample."""
    x = np.asarray(frame, np.float32)
    if not np.all(np.isfinite(x)):
        return None
    A = np.float32(np.max(np.abs(x)))
    if A == 0:
        return None
    _, e = np.frexp(A)                                                  # A = f 2^e, f in [0.5, 1)
    return np.rint(np.ldexp(x, 11 - int(e))).astype(np.int64)           # exact scaling, ties to even


def curves(q, W, max_lag):
    """(d, cum, c) for tau = 0 .. max_lag as int64 arrays (d[0] = cum[0] = 0, c[0] = 2^14), from the definition d = sum (q_i - q_{i+tau})^2."""
    q = np.asarray(q, np.int64)
    d = np.zeros(max_lag + 1, np.int64)
    win = np.lib.stride_tricks.sliding_window_view(q[:W + max_lag], W)   # win[tau] = q[tau : tau + W]
    for t0 in range(1, max_lag + 1, 256):
        t1 = min(t0 + 256, max_lag + 1)
        diff = win[t0:t1] - q[:W]
        d[t0:t1] = np.einsum("ij,ij->i", diff, diff)
    cum = np.cumsum(d)
    tau = np.arange(max_lag + 1, dtype=np.int64)
    c = np.full(max_lag + 1, C_ONE, np.int64)
    nz = cum > 0
    c[nz] = (d[nz] * tau[nz] * C_ONE) // cum[nz]
    c[0] = C_ONE
    return d, cum, c


def pick(c, min_lag, max_lag, threshold):
    """The record of one frame from its c curve."""
    c = np.asarray(c, np.int64)
    under = np.nonzero(c[min_lag:max_lag] < threshold)[0]                # lags min_lag .. max_lag - 1
    if under.size:
        tau = min_lag + int(under[0])
        while tau < max_lag - 1 and c[tau + 1] < c[tau]:
            tau += 1
        return [tau, int(c[tau - 1]), int(c[tau]), int(c[tau + 1])]
    b = min_lag + int(np.argmin(c[min_lag:max_lag]))                     # the first argmin
    return [-b, int(c[b - 1]), int(c[b]), int(c[b + 1])]


def record(frame, W, min_lag, max_lag, threshold=DEFAULT_THRESHOLD):
    q = quantise(frame)
    if q is None:
        return [0, 0, 0, 0]
    return pick(curves(q, W, max_lag)[2], min_lag, max_lag, threshold)


def frames(n, W, hop, max_lag):
    return max((n - W - max_lag) // hop + 1, 0)


def track(x, W, hop, min_lag, max_lag, threshold=DEFAULT_THRESHOLD, nframes=None):
    """int32[nframes, 4] records of one channel x; frame m reads x[m hop : m hop + W + max_lag]."""
    x = np.asarray(x, np.float32)
    nframes = frames(x.size, W, hop, max_lag) if nframes is None else nframes
    return np.array([record(x[m * hop:m * hop + W + max_lag], W, min_lag, max_lag, threshold) for m in range(nframes)], np.int32).reshape(nframes, 4)


def period(rec):
    """fp64 period of one record: parabolic refinement where the parabola opens upwards, 0 for unvoiced or empty."""
    tau, cm, c0, cp = (int(v) for v in rec)
    if tau <= 0:
        return 0.0
    den = cm - 2 * c0 + cp
    if den <= 0:
        return float(tau)
    return float(tau) + 0.5 * float(cm - cp) / float(den)


def nearest_allowed(n, scale_mask):
    """The allowed note nearest n (ties to the lower); pitch class of note k is k mod 12, C = 0."""
    lo = math.floor(n)
    hi = lo + 1
    while not (scale_mask >> (lo % 12)) & 1:
        lo -= 1
    while not (scale_mask >> (hi % 12)) & 1:
        hi += 1
    return lo if n - float(lo) <= float(hi) - n else hi


def tune_plan(records, f0_hop, f0_center, sample_rate, synthesis_hop, min_hop, max_hop, input_len, scale_mask=0xFFF, strength=1.0, retune=1.0, a4=440.0,
              shift=0):
    """(int32 hops, float64 r) of pv_tune_plan."""
    if not 1 <= scale_mask <= 0xFFF or not 0.0 <= strength <= 1.0 or not 0.0 < retune <= 1.0 or min_hop < 1 or max_hop < min_hop or f0_hop < 1:
        raise ValueError("bad argument")
    records = np.asarray(records, np.int32).reshape(-1, 4)
    nrec = records.shape[0]
    periods = [period(r) for r in records]
    hops, rs = [], []
    S, r, e = 0, 0.0, 0.0
    while True:
        t = 0.0
        if nrec:
            j = min(max((S + shift - f0_center + f0_hop // 2) // f0_hop, 0), nrec - 1)
            p = periods[j]
            if p > 0.0:
                n = 69.0 + 12.0 * math.log2(sample_rate / p / a4)
                t = strength * (float(nearest_allowed(n, scale_mask)) - n) / 12.0
        r += retune * (t - r)
        x = e + float(synthesis_hop) / (2.0 ** r)
        hop = int(min(max(math.floor(x + 0.5), min_hop), max_hop))
        e = x - float(hop)
        if S + hop > input_len:
            break
        hops.append(hop)
        rs.append(r)
        S += hop
    return np.array(hops, np.int32), np.array(rs, np.float64)


# ---- test signals: closed-form tones of a given period in samples ---------------------------------------------------------------------------

def tone(kind, period_samples, n, amplitude=0.9, phase=0.0):
    """float32[n]: 'sine'; 'harm' = harmonics 1 .. 8 at amplitude 1 / k; 'missing' = harmonics 2 .. 6 at amplitude 1 / k (no fundamental).  Scaled so that
    the peak is `amplitude`."""
    t = np.arange(n, dtype=np.float64)
    ks = {"sine": [1], "harm": range(1, 9), "missing": range(2, 7)}[kind]
    y = sum(np.sin(2.0 * np.pi * k * t / period_samples + phase * k) / k for k in ks)
    return (amplitude * y / np.max(np.abs(y))).astype(np.float32)


# ---- the planner cases shared by tests/test_f0_model.py, tests/test_f0_abi.py and tests/test_gpu_f0.py -----------------------------------------

SAMPLE_RATE = 48000.0
PLAN_GEOMETRY = dict(W=1024, hop=256, min_lag=32, max_lag=1024)
PLAN_LEN = 12000
PLAN_TONES = (452.0, 428.3, 95.0, 1210.0)
C_MAJOR = 0xAB5                                                          # C D E F G A B
_records = {}


def plan_tone(freq, n=PLAN_LEN):
    return tone("harm", SAMPLE_RATE / freq, n)


def plan_records(freq):
    """The model's records of plan_tone(freq), computed once per session; do not modify."""
    if freq not in _records:
        g = PLAN_GEOMETRY
        _records[freq] = track(plan_tone(freq), g["W"], g["hop"], g["min_lag"], g["max_lag"])
        _records[freq].setflags(write=False)
    return _records[freq]


def plan(records, **kw):
    g = PLAN_GEOMETRY
    args = dict(f0_hop=g["hop"], f0_center=(g["W"] + g["max_lag"]) // 2, sample_rate=SAMPLE_RATE, synthesis_hop=256, min_hop=128, max_hop=512, input_len=PLAN_LEN)
    args.update(kw)
    return tune_plan(records, **args)


def note_frequency(note, a4=440.0):
    return a4 * 2.0 ** ((note - 69) / 12.0)
