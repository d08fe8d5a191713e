"""The variable-ratio resampler's numpy model (tests/vari_model.py) against closed forms: what the definition itself leaves, before any kernel is involved.

Every gate is twice the figure measured on this model (DESIGN.md "Pitch curves" lists them); the figures are printed before each assertion.
"""
import numpy as np
import pytest

import resample_model as RM
import vari_model as VM


def schedule(name):
    """(B, min_count, max_count, counts)"""
    if name == "320x256":
        return 320, 256, 256, np.full(40, 256)
    if name == "320x400":
        return 320, 400, 400, np.full(40, 400)
    if name == "ramp":
        return 320, 200, 440, np.round(np.linspace(200, 436, 60)).astype(np.int64)
    if name == "64x8":
        return 64, 8, 8, np.full(400, 8)
    if name == "64x512":
        return 64, 512, 512, np.full(40, 512)
    raise KeyError(name)


# max |y - cos| at the exact positions for a unit tone at `frac` of the narrower Nyquist (the input's, or the sparsest block's), measured on this model
PASSBAND = {
    "320x256": {0.1: 1.28e-5, 0.5: 3.38e-6, 0.8: 4.16e-5},
    "320x400": {0.1: 1.34e-5, 0.5: 3.18e-6, 0.8: 4.21e-5},
    "ramp": {0.1: 1.61e-5, 0.5: 2.16e-5, 0.8: 3.13e-5},
    "64x8": {0.1: 1.20e-5, 0.5: 1.29e-6, 0.8: 3.07e-5},
    "64x512": {0.1: 1.38e-5, 0.5: 1.56e-6, 0.8: 3.77e-5},
}
TABLE_VS_EXACT = 4.77e-6          # max |w from the table - h0 at the tap's distance| over the shapes below, measured
# against ResampleModel(c, B) on unit noise, measured: name -> (max |difference|, RMS of it over the RMS of the output)
VS_FIXED = {"320x256": (2.19e-5, 5.62e-6), "320x400": (2.19e-5, 5.42e-6), "64x8": (1.66e-6, 1.33e-6), "64x512": (1.60e-5, 1.78e-6)}


def tone_error(name, frac, process=None, table=None):
    """max |y - cos(2 pi f p + 0.3)| over every output whose taps lie inside the stream, p its exact input position."""
    B, lo, hi, counts = schedule(name)
    m = VM.VariModel(B, lo, hi, 1, table)
    f = 0.5 * frac * min(1.0, counts.min() / B)
    x = np.cos(2.0 * np.pi * f * np.arange(counts.size * B, dtype=np.float64) + 0.3).astype(np.float32)
    y = np.asarray(process(x[None, :], counts) if process else m.process(x, counts), np.float64)[0]
    p = VM.positions(B, counts, m.W)
    ok = p >= m.W
    assert ok.sum() > 1000
    return float(np.max(np.abs(y[ok] - np.cos(2.0 * np.pi * f * p[ok] + 0.3))))


@pytest.mark.parametrize("name", sorted(PASSBAND))
def test_passband_tones_follow_the_cosine_at_the_exact_positions(name):
    for frac, measured in PASSBAND[name].items():
        err = tone_error(name, frac)
        print(f"passband {name} at {frac}: {err:.3e} (gate {2 * measured:.1e})")
        assert err <= 2 * measured, (name, frac, err)


@pytest.mark.parametrize("name", ["320x256", "ramp", "64x8", "64x512"])
def test_dc_gain_is_exactly_one(name):
    B, lo, hi, counts = schedule(name)
    m = VM.VariModel(B, lo, hi)
    y = m.process(np.ones(counts.size * B, np.float32), counts)[0]
    ok = VM.positions(B, counts, m.W) >= m.W
    assert np.all(y[ok] == 1.0)


def test_table_weights_follow_the_prototype():
    P = VM.prototype()
    assert P.dtype == np.float32 and P.size == 32 * 256 + 2 and P[0] == np.float32(0.91) and np.all(P[32 * 256:] == 0.0)
    worst = 0.0
    for B, c, W in [(320, 256, 40), (320, 400, 32), (320, 200, 52), (320, 436, 52), (64, 8, 256), (64, 512, 32), (4096, 8191, 256), (4095, 4096, 32)]:
        r = (np.arange(c) * B) % c
        wt, fd = VM.weights(B, c, r, W, P)
        we, _ = VM.weights(B, c, r, W, None, exact=True)
        worst = max(worst, float(np.max(np.abs(wt - we))))
        assert np.all(wt[(np.abs((np.arange(2 * W)[None, :] - W + 1) * c - r[:, None]) >= 32 * max(B, c))] == 0.0)      # zero from 32 widened samples on
        assert np.all((wt != 0).sum(axis=1) <= 2 * -(-32 * max(B, c) // c))                                             # at most 2 ceil(32 sigma) taps
    print(f"table against h0: {worst:.3e} (gate {2 * TABLE_VS_EXACT:.1e})")
    assert worst <= 2 * TABLE_VS_EXACT


@pytest.mark.parametrize("name", sorted(VS_FIXED))
def test_constant_counts_agree_with_the_fixed_resampler(name):
    """With every count c the step is B / c = M / L of ResampleModel(c, B); the two filters share the prototype and differ in normalisation (a sum
    per output against a sum per phase row) and in the table interpolation.  The variable model's output J sits W input samples later, W c / B outputs."""
    B, lo, hi, counts = schedule(name)
    c = int(counts[0])
    m = VM.VariModel(B, lo, hi)
    x = np.random.default_rng(1).standard_normal(counts.size * B).astype(np.float32)
    y = m.process(x, counts)[0]
    fixed = RM.ResampleModel(c, B)
    z = fixed.process(x[None, :])[0]
    assert fixed.W == m.W and (m.W * c) % B == 0
    shift = m.W * c // B
    n = min(y.size - shift, z.size)
    d = y[shift:shift + n] - z[:n]
    worst, rel = float(np.max(np.abs(d))), float(np.sqrt(np.mean(d ** 2)) / np.sqrt(np.mean(z[:n] ** 2)))
    print(f"against the fixed resampler {name}: max {worst:.3e}, relative RMS {rel:.3e} (gates {2 * VS_FIXED[name][0]:.1e}, {2 * VS_FIXED[name][1]:.1e})")
    assert n > 3000 and worst <= 2 * VS_FIXED[name][0] and rel <= 2 * VS_FIXED[name][1]


def test_shapes_outside_the_range_are_refused():
    for B, lo, hi in [(0, 1, 1), (4097, 4096, 4096), (320, 0, 440), (320, 300, 200), (320, 200, 8193), (320, 39, 440), (64, 8, 513), (1, 1, 9)]:
        with pytest.raises(ValueError):
            VM.half_width(B, lo, hi)
    assert VM.half_width(320, 200, 440) == 52 and VM.half_width(64, 8, 512) == 256 and VM.half_width(1, 1, 8) == 32 and VM.half_width(4096, 512, 8192) == 256
    assert VM.half_width(320, 40, 440) == 256 and VM.half_width(320, 400, 400) == 32


@pytest.mark.parametrize("shape", [(320, 200, 440), (64, 8, 512), (1, 1, 8)])
def test_any_split_of_a_stream_gives_the_same_model_output(shape):
    B, lo, hi = shape
    rng = np.random.default_rng(B + hi)
    counts = rng.integers(lo, hi + 1, 30 if B > 1 else 300)
    x = rng.standard_normal((2, counts.size * B)).astype(np.float32)
    whole = VM.VariModel(B, lo, hi, 2)
    want = whole.process(x, counts)
    assert want.shape[1] == counts.sum()
    m = VM.VariModel(B, lo, hi, 2)
    at, parts = 0, []
    while at < counts.size:
        n = int(rng.integers(1, 7))
        parts.append(m.process(x[:, at * B:(at + n) * B], counts[at:at + n]))
        at += n
    got = np.concatenate(parts, axis=1)
    assert np.array_equal(got, want) and np.array_equal(m.hist, whole.hist) and (m.blocks, m.outputs) == (whole.blocks, whole.outputs)


# ---- the composition: StretchModel followed by the variable model at constant counts, against the closed form of tests/test_resample_model.py ----

# name -> (N, hop, hs, partials, amplitudes): pitch x hs / hop at constant duration
GLIDE_CASES = {"1024-256-320": (1024, 256, 320, [64.37], [0.5]), "256-80-64": (256, 80, 64, [40.3], [0.5]), "1024-400-320": (1024, 400, 320, [64.37], [0.5])}
# measured on the models: case -> (largest |fitted amplitude / A - 1|, relative residual)
GLIDE_MEASURED = {"1024-256-320": (1.42e-5, 1.32e-6), "256-80-64": (1.15e-6, 1.27e-6), "1024-400-320": (1.42e-7, 3.55e-7)}


def glide_fit(name, process=None):
    """(amplitude ratios, relative residual) of the case's tone through stretch then resampler at the constant hop.  Output j of the pair sits at
    position j hs / hop - W of the stretched signal; W hop / hs is a whole number in every case, so dropping that many outputs puts the rest on the
    grid of test_resample_model.pitch_basis.  process(x[1, n], hops) -> [1, n] replaces the models (the GPU test passes the handle)."""
    import tones
    from stretch_model import StretchModel
    import test_resample_model as TRM
    N, hop, hs, freqs, amps = GLIDE_CASES[name]
    tones.check_partials(N, freqs)
    T, x = tones.case_input(N, hop, hs, freqs, amps)
    hops = np.full(T, hop, np.int32)
    W = VM.half_width(hs, hop, hop)
    if process is None:
        mid = StretchModel(N, hop, hs).process(x[None, :]).astype(np.float32)
        y = VM.VariModel(hs, hop, hop).process(mid, hops)[0]
    else:
        y = np.asarray(process(x[None, :], hops), np.float64)[0]
    assert y.size == x.size and (W * hop) % hs == 0                      # duration is kept sample for sample
    L, M = RM.reduce_ratio(hop, hs)
    return TRM.pitch_fit(y[W * hop // hs:], T * hs - W, N, hop, hs, L, M, freqs, amps)


@pytest.mark.parametrize("name", sorted(GLIDE_CASES))
def test_stretch_then_variable_resampler_fits_the_closed_form(name):
    ratio, res = glide_fit(name)
    amp_gate, res_gate = (2 * v for v in GLIDE_MEASURED[name])
    print(f"glide {name}: amplitude ratio {ratio}, residual {res:.3e} (gates {amp_gate:.1e}, {res_gate:.1e})")
    assert np.max(np.abs(ratio - 1.0)) <= amp_gate and res <= res_gate, (name, ratio, res)


# ---- non-finite input: the reach of a bad sample (pv_vari.h, NON-FINITE INPUT) ----

def _reach_case():
    """A small schedule whose counts lie on both sides of B (widened and plain taps), two calls, bad samples in the first T - 1 samples, mid-stream and
    on the last sample of the first call."""
    B, lo, hi = 20, 12, 40
    rng = np.random.default_rng(20)
    counts = np.array([12, 40, 12, 33, 20, 40, 13, 21, 40, 12], np.int64)
    x = rng.standard_normal((3, counts.size * B)).astype(np.float32)
    x[1, 5], x[1, 4 * B - 1], x[1, 7 * B] = np.nan, np.inf, -np.inf
    x[2, 3 * B] = np.nan
    return B, lo, hi, counts, x, 4


def test_the_poisoned_mask_equals_a_per_output_evaluation_in_exact_arithmetic():
    """Output by output and tap by tap in Python integers and f32 scalars, the weight's zero test in exact rationals: nothing shared with
    VariModel.process but the definition."""
    from fractions import Fraction
    B, lo, hi, counts, x, cut = _reach_case()
    m = VM.VariModel(B, lo, hi, 3)
    W, T = m.W, m.T
    P = VM.prototype()
    ya, pa, na = m.process(x[:, :cut * B], counts[:cut], reach=True)
    yb, pb, nb = m.process(x[:, cut * B:], counts[cut:], reach=True)
    y, poisoned, near = np.concatenate([ya, yb], axis=1), np.concatenate([pa, pb], axis=1), np.concatenate([na, nb], axis=1)
    stream = np.concatenate([np.zeros((3, T - 1), np.float32), x], axis=1)       # stream[:, T - 1 + e] = x[:, e], zeros before the stream
    bad = ~np.isfinite(stream)
    want_p, want_n = np.zeros_like(poisoned), np.zeros_like(near)
    j = 0
    for b, c in enumerate(counts.tolist()):
        den = max(B, c)
        inv = np.float32(1.0) / np.float32(den)
        for k in range(c):
            n, r = b * B + (k * B) // c, (k * B) % c
            for i in range(T):
                aq = abs((i - W + 1) * c - r) * VM.Q
                q = min(aq // den, VM.HALF_WIDTH * VM.Q)
                f, d = np.float32(aq % den) * inv, P[q + 1] - P[q]
                assert type(f) is np.float32 and type(d) is np.float32
                nonzero = Fraction(float(f)) * Fraction(float(d)) + Fraction(float(P[q])) != 0
                hit = bad[:, n + i]                                                # tap i reads x[n - 2 W + 1 + i] = stream[n + i]
                want_n[:, j] |= hit
                if nonzero:
                    want_p[:, j] |= hit
            j += 1
    assert j == counts.sum()
    assert np.array_equal(poisoned, want_p) and np.array_equal(near, want_n)
    assert not poisoned[0].any() and poisoned[1].any() and poisoned[2].any()
    assert np.any(near & ~poisoned)                                                # some output has a bad sample under zero weights only
    assert np.all(np.isfinite(y))
    # the values are those of the stream with the bad samples replaced by 0, the history is the input as it came
    z = VM.VariModel(B, lo, hi, 3)
    assert np.array_equal(y, z.process(np.where(np.isfinite(x), x, np.float32(0.0)), counts))
    assert np.array_equal(m.hist.view(np.uint32), x[:, x.shape[1] - (T - 1):].view(np.uint32))


def test_a_clean_input_has_an_empty_mask_and_unchanged_results():
    B, lo, hi, counts, x, cut = _reach_case()
    x = np.where(np.isfinite(x), x, np.float32(0.25))
    a, b = VM.VariModel(B, lo, hi, 3), VM.VariModel(B, lo, hi, 3)
    plain = a.process(x, counts, bound=True)
    with_reach = b.process(x, counts, bound=True, reach=True)
    assert len(with_reach) == len(plain) + 2
    for u, v in zip(plain, with_reach):
        assert np.array_equal(u, v)
    assert not with_reach[-2].any() and not with_reach[-1].any()
    assert np.array_equal(a.hist, b.hist) and (a.blocks, a.outputs) == (b.blocks, b.outputs)
    y2, p2, n2 = VM.VariModel(B, lo, hi, 3).process(x, counts, reach=True)
    assert np.array_equal(y2, plain[0]) and not p2.any() and not n2.any()


def test_the_kernel_weight_is_zero_exactly_from_32_widened_samples_on():
    """On the shapes the GPU tests use no weight cancels to zero inside the prototype's support, so there `non-zero weight` is `closer than 32 max(1, B / c)
    samples`; the mask does not rely on it."""
    P = VM.prototype()
    for B, c, W in [(320, 200, 52), (320, 440, 52), (64, 8, 256), (64, 512, 256), (64, 9, 256), (64, 511, 256)]:
        r = (np.arange(c) * B) % c
        nz = VM.nonzero_weights(B, c, r, W, P)
        a = np.abs((np.arange(2 * W)[None, :] - W + 1) * c - r[:, None])
        assert np.array_equal(nz, a * VM.Q // max(B, c) < VM.HALF_WIDTH * VM.Q)
