"""numpy / int64 restatement of the pitch contour tracker, as DESIGN.md "Pitch contour" states it: the candidate table of pv_contour_track (the K best
dips of the c curve of tests/f0_model.py, ranked by a biased key) and the path of pv_contour_path (the cheapest state sequence through the table).  Every
value is an exact integer function of the samples, so the device and the host code are compared with `==`."""
import numpy as np

from f0_model import curves, quantise

DEFAULTS = dict(bias=1024, unvoiced_cost=2458, voicing_cost=2458, jump_cost=16384)
C_CAP = 1 << 14


# ---- candidates --------------------------------------------------------------------------------------------------------------------------------

def dips(c, min_lag, max_lag, K, bias):
    """int64[K, 4]: the K dips of smallest key of one c curve, in key order; the slots beyond the number of dips are zero."""
    c = np.asarray(c, np.int64)
    t = np.arange(min_lag, max_lag, dtype=np.int64)                       # lags min_lag .. max_lag - 1
    t = t[(c[t] < c[t - 1]) & (c[t] <= c[t + 1])]
    key = ((c[t] + (bias * t) // max_lag) << 16) | t
    t = t[np.argsort(key)][:K]                                            # the keys differ in their low 16 bits: no ties
    out = np.zeros((K, 4), np.int64)
    out[:t.size] = np.stack([t, c[t - 1], c[t], c[t + 1]], axis=1)
    return out


def frame_candidates(frame, W, min_lag, max_lag, K, bias):
    q = quantise(frame)
    if q is None:
        return np.zeros((K, 4), np.int64)
    return dips(curves(q, W, max_lag)[2], min_lag, max_lag, K, bias)


def frames(n, W, hop, max_lag):
    return max((n - W - max_lag) // hop + 1, 0)


def candidates(x, W, hop, min_lag, max_lag, K=8, bias=1024, nframes=None):
    """int32[nframes, K, 4] of one channel x; frame m reads x[m hop : m hop + W + max_lag]."""
    x = np.asarray(x, np.float32)
    nframes = frames(x.size, W, hop, max_lag) if nframes is None else nframes
    out = np.zeros((nframes, K, 4), np.int32)
    for m in range(nframes):
        out[m] = frame_candidates(x[m * hop:m * hop + W + max_lag], W, min_lag, max_lag, K, bias)
    return out


# ---- the path ----------------------------------------------------------------------------------------------------------------------------------

def observation(table, m, s, max_lag, bias, unvoiced_cost):
    """o_m(s), or None where s is not a state of frame m.  State K is the unvoiced state."""
    K = table.shape[1]
    if s == K:
        return unvoiced_cost if table[m, 0, 0] > 0 else 0
    tau, _, c0, _ = (int(v) for v in table[m, s])
    if tau <= 0:
        return None
    return min(c0, C_CAP) + (bias * tau) // max_lag


def transition(table, m, a, b, voicing_cost, jump_cost):
    """t(a -> b) from frame m - 1 to frame m."""
    K = table.shape[1]
    if a == K and b == K:
        return 0
    if a == K or b == K:
        return voicing_cost
    ta, tb = int(table[m - 1, a, 0]), int(table[m, b, 0])
    return (2 * jump_cost * abs(tb - ta)) // (ta + tb)


def path_cost(table, states, max_lag, bias=1024, unvoiced_cost=2458, voicing_cost=2458, jump_cost=16384):
    """The cost of one state sequence, or None where it passes through an empty slot."""
    table = np.asarray(table, np.int64)
    total = 0
    for m, s in enumerate(states):
        o = observation(table, m, s, max_lag, bias, unvoiced_cost)
        if o is None:
            return None
        total += o
        if m:
            total += transition(table, m, states[m - 1], s, voicing_cost, jump_cost)
    return total


def path(table, max_lag, bias=1024, unvoiced_cost=2458, voicing_cost=2458, jump_cost=16384):
    """(int32[T, 4] records, int32[T] states) of the candidate table int[T, K, 4] of one channel."""
    table = np.asarray(table, np.int64)
    T, K = table.shape[0], table.shape[1]
    records, states = np.zeros((T, 4), np.int32), np.zeros(T, np.int32)
    if T == 0:
        return records, states
    back = np.zeros((T, K + 1), np.int64)
    D = [observation(table, 0, s, max_lag, bias, unvoiced_cost) for s in range(K + 1)]
    for m in range(1, T):
        E = [None] * (K + 1)
        for s in range(K + 1):
            o = observation(table, m, s, max_lag, bias, unvoiced_cost)
            if o is None:
                continue
            best, arg = None, 0
            for a in range(K + 1):                                         # ascending: a tie stays with the lowest a
                if D[a] is None:
                    continue
                v = D[a] + transition(table, m, a, s, voicing_cost, jump_cost)
                if best is None or v < best:
                    best, arg = v, a
            E[s], back[m, s] = o + best, arg
        D = E
    s = min((v, a) for a, v in enumerate(D) if v is not None)[1]             # the first argmin
    for m in range(T - 1, -1, -1):
        states[m] = s
        if s < K:
            records[m] = table[m, s]
        elif table[m, 0, 0] > 0:
            records[m] = table[m, 0]
            records[m, 0] = -records[m, 0]
        s = int(back[m, s])
    return records, states


def track(x, W, hop, min_lag, max_lag, K=8, bias=1024, unvoiced_cost=2458, voicing_cost=2458, jump_cost=16384):
    """int32[nframes, 4]: the f0 records of the path through the candidates of one channel x."""
    return path(candidates(x, W, hop, min_lag, max_lag, K, bias), max_lag, bias, unvoiced_cost, voicing_cost, jump_cost)[0]


# ---- test signals --------------------------------------------------------------------------------------------------------------------------------

def fading_tone(period, depth, noise, n=12000, seed=1):
    """A two-harmonic tone whose fundamental fades by `depth` around the middle of 6000-sample cycles, plus white noise; peak 0.8."""
    t = np.arange(n, dtype=np.float64)
    w = 2.0 * np.pi / period
    a1 = 1.0 - depth * 0.5 * (1.0 - np.cos(2.0 * np.pi * t / 6000.0))
    y = a1 * np.sin(w * t) + 0.6 * np.sin(2.0 * w * t + 0.3) + noise * np.random.default_rng(seed).standard_normal(n)
    return (0.8 * y / np.max(np.abs(y))).astype(np.float32)


def leap_tone(p0=200.0, p1=100.0, at=8000, n=16000, noise=0.02, seed=1):
    """The two-harmonic tone with the period p0 up to sample `at` and p1 from there on, phase-continuous."""
    per = np.where(np.arange(n) < at, p0, p1)
    ph = np.concatenate([[0.0], np.cumsum(2.0 * np.pi / per)[:-1]])
    y = np.sin(ph) + 0.6 * np.sin(2.0 * ph + 0.3) + noise * np.random.default_rng(seed).standard_normal(n)
    return (0.8 * y / np.max(np.abs(y))).astype(np.float32)


def gross(records, period, tol=0.2):
    """How many voiced records lie more than tol off `period` (a number, or one per record)."""
    import f0_model
    p = np.array([f0_model.period(r) for r in np.asarray(records).reshape(-1, 4)])
    return int(np.sum((p > 0) & (np.abs(p - period) > tol * np.asarray(period, np.float64))))


# ---- the tables shared by tests/test_contour_model.py and tests/test_contour_abi.py ---------------------------------------------------------------

GEOMETRY = dict(W=512, hop=128, min_lag=32, max_lag=512)
_tables = {}


def tone_noise_tone(period=100.37):
    """The steady tone with samples 6000 .. 10000 replaced by noise."""
    x = np.array(fading_tone(period, 0.0, 0.02))
    x[6000:10000] = (0.2 * np.random.default_rng(1).standard_normal(12000)[6000:10000]).astype(np.float32)
    return x


def signal(name):
    """'fade P depth' | 'noisy P level' | 'leap' | 'tnt'."""
    kind, *args = name.split()
    if kind == "fade":
        return fading_tone(float(args[0]), float(args[1]), 0.02)
    if kind == "noisy":
        return fading_tone(float(args[0]), 0.0, float(args[1]))
    return {"leap": leap_tone, "tnt": tone_noise_tone}[kind]()


def table(name, K=8, bias=1024):
    """The model's candidate table of signal(name) at GEOMETRY, computed once per session; do not modify."""
    if (name, K, bias) not in _tables:
        g = GEOMETRY
        t = candidates(signal(name), g["W"], g["hop"], g["min_lag"], g["max_lag"], K, bias)
        t.setflags(write=False)
        _tables[name, K, bias] = t
    return _tables[name, K, bias]


FADES = [f"fade {p} {d}" for p in (100.37, 217.3) for d in (0.9, 0.97)]
NOISY = [f"noisy {p} {n}" for n in (0.2, 0.3) for p in (40.0, 100.37, 217.3)]


def random_table(rng, T, K, max_lag=512, lead=0):
    """int32[T, K, 4]: a few lags and a few c values only, so that costs tie; slots emptied at random (holes as well as tails, slot 0 too), whole frames
    emptied, and `lead` empty frames in front."""
    lags = rng.choice(np.arange(2, max_lag), size=min(5, max_lag - 2), replace=False)
    t = np.zeros((T, K, 4), np.int32)
    t[:, :, 0] = rng.choice(lags, size=(T, K))
    t[:, :, 1:] = rng.choice([0, 100, 100, 2458, 2500, 16384, 40000], size=(T, K, 3))
    t[rng.random((T, K)) < 0.25] = 0
    t[rng.random(T) < 0.15] = 0
    t[:lead] = 0
    return t
