"""Parity at level, CPU side (tests/level_model.py): the float32 restatement's own figures against the oracle are pinned and reproduced -- the GPU gate of
tests/test_gpu_level_parity.py is 4 x these --, the corpus meets the conditions the oracle alone must meet on it, the per-bin bound of the shifted spectrum holds for the
model that names its operations, and the hop metric sees planted errors that the stream rms gate of 2e-7 lets through.  No kernel is involved."""
import numpy as np
import pytest

import gpu_algo_model as G
import level_model as LM
import oracle_lib
import signals as S

SIZES = sorted({N for N, _ in LM.SHAPES})


def test_fft32_is_float32_arithmetic_and_a_dft():
    rng = np.random.default_rng(5)
    for N in (16, 64, 2048):
        z = (rng.standard_normal((3, N)) + 1j * rng.standard_normal((3, N))).astype(np.complex64)
        for inv in (False, True):
            got = LM.fft32(z, inverse=inv)
            assert got.dtype == np.complex64
            ref = np.fft.ifft(z.astype(np.complex128)) * N if inv else np.fft.fft(z.astype(np.complex128))
            err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
            assert 0 < err < 4 * np.log2(N) * LM.EPS32, (N, inv, err)            # f32 round-off is there (not a double transform), and no more than that


@pytest.mark.parametrize("N", [256, 1024, 2048])
def test_residue32_is_residue_upper_batched(N):
    """Both parities of log2 N; bit for bit against the model the kernels follow, and within f32 round-off of what the oracle's transform leaves above Nyquist."""
    hop = N // 4
    x = LM.corpus(1024, 256)["quiet_mid"][0][:3 * N]
    xw = LM.frames_of(x, N, hop)[[5, 7]] * G.hann(N)
    got = LM.residue32(xw)
    H = N // 2 + 1
    for j in range(2):
        want = G.residue_upper(xw[j])
        assert np.array_equal(got[j, H:].view(np.uint32), want[H:].view(np.uint32))
    o = oracle_lib.Oracle(N, hop, 1)
    for m in range(8):
        o.process([x[m * hop:(m + 1) * hop]], 0.8)
    d = o.debug()
    Xo = d["X"][0::2] + 1j * d["X"][1::2]
    assert np.max(np.abs(got[1, H:] - Xo[H:])) < 8 * np.log2(N) * LM.EPS32 * np.max(np.abs(Xo[H:]))
    Xl = LM.fft32((xw[1]).astype(np.complex64))
    assert np.max(np.abs(Xl[:H] - Xo[:H])) < 8 * np.log2(N) * LM.EPS32 * np.max(np.abs(Xo[:H]))


@pytest.mark.parametrize("N,hop", [(1024, 256), (2048, 128), (4096, 512)])
def test_levels_take_their_alignment_from_the_oracle(N, hop):
    """`burst`: the oracle's output is nonzero exactly on the hops with L > 0 -- the loud tail leaves the accumulator on the hop L says, the quiet tone arrives on the hop L says."""
    x = LM.corpus(N, hop)["burst"]
    L = LM.hop_levels(x, N, hop)
    R, T = N // hop, x.shape[1] // hop
    for row in LM.PITCH_ROWS:
        yo, _ = LM.oracle_run(N, hop, "burst", row)
        live = np.any(yo.reshape(LM.NCH, T, hop) != 0, axis=-1)
        assert np.array_equal(live, L > 0), row
    silent = np.flatnonzero(L[0] == 0)
    assert list(silent) == [3 + 2 * R - 2, 3 + 2 * R - 1]                     # two hops of exact zeros between the tail of the burst and the tone


@pytest.mark.parametrize("N,hop", LM.SHAPES)
def test_corpus_conditions(N, hop):
    """What the oracle alone must meet on the corpus, so that the GPU test cannot hide behind its inputs: every L > 0 hop finite, every L == 0 hop exactly 0, peak
    levels within 1e-9 .. 1e9 -- and `fade` crosses the low end of the guarded range of the fp32-first kernels (max|X|^2 = 1.1e-7, pv_guard.h) in both directions."""
    for name, x in LM.corpus(N, hop).items():
        assert 1e-9 < np.max(np.abs(x)) < 1e9, name
        L = LM.hop_levels(x, N, hop)
        T = x.shape[1] // hop
        for row in LM.PITCH_ROWS:
            yo, _ = LM.oracle_run(N, hop, name, row)
            hops = yo.reshape(LM.NCH, T, hop)
            assert np.all(np.isfinite(hops[L > 0])), (name, row)
            assert np.all(hops[L == 0] == 0), (name, row)
            rr, mm = LM.hop_metrics(yo, yo, L, hop)
            assert rr.max() == 0 and mm.max() == 0
    if N in (1024, 2048):
        x = LM.corpus(N, hop)["fade"][0]
        top = np.max(np.abs(np.fft.rfft(LM.frames_of(x, N, hop, np.float64) * G.hann(N), axis=-1)), axis=-1) ** 2
        T = top.size
        lo, hi = 1.1e-7 / 16, 1.1e-7 * 16
        assert top[:T // 2].max() > hi and top[T // 2 - 2:T // 2 + 3].min() < lo and top[T // 2:].max() > hi


def test_the_quiet_side_is_exercised():
    """At least a quarter of all hops of the corpus lie below 1e-4 of their own stream's largest L."""
    quiet = total = 0
    for N, hop in LM.SHAPES:
        q = t = 0
        for x in LM.corpus(N, hop).values():
            L = LM.hop_levels(x, N, hop)
            q += int(np.sum(L < 1e-4 * L.max()))
            t += L.size
        print(f"{N}/{hop}: {q} of {t} hops below 1e-4 of their stream's largest L")
        quiet, total = quiet + q, total + t
    assert quiet >= total / 4, (quiet, total)


def _restatement_worst(N, hop):
    worst = np.zeros(2)
    for name, x in LM.corpus(N, hop).items():
        L = LM.hop_levels(x, N, hop)
        for row in LM.PITCH_ROWS:
            yo, peaks = LM.oracle_run(N, hop, name, row, True)
            y = LM.restate(N, hop, x, LM.pitch_row(row, x.shape[1] // hop), peaks)
            rr, mm = LM.hop_metrics(y, yo, L, hop)
            assert np.isfinite(rr.max()) and np.isfinite(mm.max()), (name, row)      # silent hops are exact zeros in the restatement too
            worst = np.maximum(worst, [rr.max(), mm.max()])
    return worst


@pytest.mark.parametrize("N", SIZES)
def test_restatement_figures_are_pinned_and_reproduced(N):
    worst = np.zeros(2)
    for n, hop in LM.SHAPES:
        if n == N:
            w = _restatement_worst(N, hop)
            print(f"restatement N={N} hop={hop}: worst rms/L {w[0]:.3e}  max/L {w[1]:.3e}")
            worst = np.maximum(worst, w)
    k_rms, k_max = LM.RESTATEMENT_FIGURES[N]
    print(f"restatement N={N}: worst rms/L {worst[0]:.3e} (pinned {k_rms:.2e})  max/L {worst[1]:.3e} (pinned {k_max:.2e})")
    assert worst[0] <= k_rms and worst[1] <= k_max
    assert worst[0] >= k_rms / 1.25 and worst[1] >= k_max / 1.25, "the pinned figures are stale"


def _ulps(y, k):
    return (y.astype(np.float64) + k * np.spacing(np.abs(y)).astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("N,hop", [(1024, 256), (2048, 128), (4096, 1024)])
def test_the_hop_metric_sees_what_the_stream_gate_does_not(N, hop):
    """Small arithmetic errors planted in a copy of the oracle's own output: a quiet channel 1e-4 off, one quiet hop off by 1e-3 of its level, one loud hop 40 ulps
    off.  Each copy passes the stream rms gate of 2e-7 and fails the hop metric at the GPU gate."""
    k_rms, k_max = LM.gate(N)
    assert 0 < k_rms < 1e-5 and 0 < k_max < 1e-4
    cases = []
    for name in ("quiet_mid", "fade"):
        x = LM.corpus(N, hop)[name]
        L = LM.hop_levels(x, N, hop)
        yo, _ = LM.oracle_run(N, hop, name, "1.5")
        T = L.shape[1]
        if name == "quiet_mid":
            y = yo.copy()
            y[1] = (yo[1].astype(np.float64) * (1 + 1e-4)).astype(np.float32)
            cases.append(("quiet channel x (1 + 1e-4)", y, yo, L))
            qc, lc = 1, 0
        else:
            qc, lc = 2, 0
        qh = int(np.argmin(np.where(L[qc] > 0, L[qc], np.inf)))                  # the quietest hop of the quiet channel (the bottom of the fade) ...
        lh = int(np.argmax(np.sqrt(np.mean(yo[lc].astype(np.float64).reshape(T, hop) ** 2, axis=-1))))     # ... and the loudest output hop of a loud one
        y = yo.copy()
        y[qc, qh * hop:(qh + 1) * hop] = (yo[qc, qh * hop:(qh + 1) * hop].astype(np.float64) + 1e-3 * L[qc, qh]).astype(np.float32)
        cases.append((f"{name}: quiet hop + 1e-3 L", y, yo, L))
        y = yo.copy()
        y[lc, lh * hop:(lh + 1) * hop] = _ulps(yo[lc, lh * hop:(lh + 1) * hop], 40)
        cases.append((f"{name}: loud hop + 40 ulps", y, yo, L))
    for what, y, yo, L in cases:
        assert S.rms(y.astype(np.float64) - yo) < LM.STREAM_RMS_GATE, what
        fails, worst = LM.hop_failures(y, yo, L, hop, k_rms, k_max)
        assert fails, (what, worst)
        assert not LM.hop_failures(yo, yo, L, hop, k_rms, k_max)[0]


@pytest.mark.parametrize("N,hop", [(1024, 256), (2048, 512), (4096, 1024), (8192, 2048)])
@pytest.mark.parametrize("pitch", [1.5, 0.8])
def test_the_per_bin_bound_holds_for_the_model(N, hop, pitch):
    """gpu_algo_model.shift_spectrum does exactly the operations level_model.spectrum_bound names (X rounded to f32, f32 root of unity, f32 product, f32 sum): its Y
    is the oracle's within C(n) 2^-24 A[k] on every bin, exactly 0 where nothing lands, and A bounds the oracle's |Y|."""
    H = N // 2 + 1
    worst = 0.0
    for signal in ("loud_partial", "fade"):
        for m, (X, Yr, peaks) in LM.oracle_taps(N, hop, signal, pitch).items():
            Ym, _, pk, (A, n, n_res) = G.shift_spectrum(X[:H], X, np.float32(pitch), m * hop, N, contributions=True)
            assert np.array_equal(pk, peaks)
            assert len(G.shift_spectrum(X[:H], X, np.float32(pitch), m * hop, N)) == 3          # one result by default
            assert np.all(np.abs(Yr) <= A * (1 + 1e-12)), (signal, m)
            assert np.all(Yr[A == 0] == 0) and np.all(Ym[A == 0] == 0) and np.all((A == 0) == (n == 0))
            assert (pitch < 1) == bool(n_res.any()), "sources above Nyquist are read exactly when the spectrum moves down"
            bound = LM.spectrum_bound(A, n, 0 * n_res, N, X)                        # (the model takes the residue from the oracle's fp64 spectrum: no residue term)
            k = np.arange(1, H - 1)
            err = np.abs(Ym.astype(np.complex128) - Yr)[k]
            live = A[k] > 0
            assert live.sum() > H // 4
            ratio = np.max(err[live] / bound[k][live])
            worst = max(worst, ratio)
            assert ratio <= 1.0, (signal, m, ratio)
    print(f"model N={N} pitch={pitch}: worst |Ym - Yr| / bound {worst:.3f}")
