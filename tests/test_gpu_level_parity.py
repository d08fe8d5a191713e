"""Parity at level, GPU side: every output hop of every channel of the pitch shifter's frame kernels against the oracle at that hop's own level L(c, h)
(tests/level_model.py: the largest rms of the windowed input frames whose overlap-add reaches the hop), on signals with dynamics -- a fade through the low end of the
guarded range and back, a burst followed by digital silence and a -100 dB tone, a -100 dB channel next to a full-scale one, the same 2^20 up and down, one partial over
a -110 dB floor -- and the shifted spectrum bin by bin against a bound that scales with what lands on the bin.  One shape per kernel path, each as one batch, in chunks
of five frames and split into calls of 1, 3 and the rest: every form is held on its own, so the first hop after a cut meets the gate by itself.

The gate is 4 x the figures the float32 restatement of the operation reaches against the oracle on the CPU (level_model.RESTATEMENT_FIGURES, pinned and reproduced by
tests/test_level_model.py); it is never fitted to a kernel.  Each test prints the worst rms / L, max / L and per-bin ratio it saw (DESIGN.md section 2a records them)."""
import numpy as np
import pytest

import gpu_algo_model as G
import level_model as LM

pytestmark = pytest.mark.gpu

GENERIC, WORKGROUP, RESIDENT, FP64_FORWARD = 1, 4, 32, 256

# id, N, hop, flags, the kernel the handle must report
PATHS = [
    ("wave1024", 1024, 256, 0, "pv_wave_kernel_1024"),
    ("wave1024_fp64_forward", 1024, 256, FP64_FORWARD, "pv_wave_kernel_1024"),
    ("wave1024_resident", 1024, 256, RESIDENT, "pv_wave_kernel_1024"),
    ("wave2k_512", 2048, 512, 0, "pv_wave2k_kernel"),
    ("wave2k_128", 2048, 128, 0, "pv_wave2k_kernel"),
    ("wg16_4096", 4096, 1024, 0, "pv_wg16_kernel"),
    ("wg16_8192", 8192, 2048, 0, "pv_wg16_kernel"),
    ("wg_4096_512", 4096, 512, WORKGROUP, "pv_wg_kernel"),
    ("generic_2048_128", 2048, 128, GENERIC, "pv_chain_kernel"),
    ("generic_256", 256, 64, 0, "pv_chain_kernel"),
    ("generic_64", 64, 16, 0, "pv_chain_kernel"),
]
SIGNALS = ["fade", "burst", "quiet_mid", "quiet_first", "quiet_last", "scaled_up", "scaled_down", "loud_partial"]
FORMS = ("batch", "chunks_of_5", "calls_1_3_rest")
WORST = {}                                                                   # path id -> [rms / L, max / L] over what has run so far


def _pv(N, hop, T, flags, fpc=0):
    import phaze_amd
    return phaze_amd.PhaseVocoder(fft_size=N, hop_size=hop, max_channels=LM.NCH, max_hops=T, frames_per_chunk=fpc, flags=flags)


def _quanta(pv, x, pitch, a, b, y):
    """hops [a, b) one render quantum at a time (the only way onto the resident kernel)"""
    hop, nch = pv.hop_size, x.shape[0]
    for m in range(a, b):
        o = [np.zeros(hop, np.float32) for _ in range(nch)]
        assert pv.process([[x[c, m * hop:(m + 1) * hop] for c in range(nch)]], [o], {"pitchFactor": pitch[m:m + 1]}) is True
        for c in range(nch):
            y[c, m * hop:(m + 1) * hop] = o[c]


def _batch(pv, x, pitch, a, b, y):
    hop = pv.hop_size
    y[:, a * hop:b * hop] = pv.process_batch(x[:, a * hop:b * hop], pitch[a:b])


def _run(pv, form, resident, x, pitch):
    """One stream in one of the three forms.  On the resident instance the stream is quanta; its cuts are batch calls between them (the waves leave, a launch runs --
    in chunks of five frames where the form says so --, the next quantum brings them back)."""
    T = x.shape[1] // pv.hop_size
    y = np.full_like(x, np.nan)
    pv.reset()
    if resident:
        cuts = {"batch": [], "chunks_of_5": [(10, min(20, T - 1))], "calls_1_3_rest": [(1, 4)]}[form]
        pos = 0
        for a, b in cuts:
            _quanta(pv, x, pitch, pos, a, y)
            _batch(pv, x, pitch, a, b, y)
            pos = b
        _quanta(pv, x, pitch, pos, T, y)
    elif form == "calls_1_3_rest":
        for a, b in ((0, 1), (1, 4), (4, T)):
            _batch(pv, x, pitch, a, b, y)
    else:
        _batch(pv, x, pitch, 0, T, y)
    return y


@pytest.mark.parametrize("signal", SIGNALS)
@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_every_hop_of_every_channel_at_its_own_level(path, signal):
    """rms(y - yo over the hop) / L(c, h) <= K_rms and max|y - yo| / L(c, h) <= K_max for every channel and hop, no hop left out; where L == 0 the kernel's hop
    and the oracle's are exactly 0.  K = 4 x the restatement's own figures at this FFT size."""
    pid, N, hop, flags, kernel = path
    x = LM.corpus(N, hop)[signal]
    T = x.shape[1] // hop
    L = LM.hop_levels(x, N, hop)
    k_rms, k_max = LM.gate(N)
    handles = {form: _pv(N, hop, T, flags, 5 if form == "chunks_of_5" else 0) for form in FORMS}
    worst = WORST.setdefault(pid, [0.0, 0.0])
    try:
        for pv in handles.values():
            assert pv.info()["kernel_name"] == kernel
        for row in LM.PITCH_ROWS:
            pitch = LM.pitch_row(row, T)
            yo, _ = LM.oracle_run(N, hop, signal, row)
            for form, pv in handles.items():
                y = _run(pv, form, bool(flags & RESIDENT), x, pitch)
                assert np.all(np.isfinite(y)), (pid, signal, row, form)
                fails, (wr, wm) = LM.hop_failures(y, yo, L, hop, k_rms, k_max)
                print(f"level parity {pid} {signal} pitch {row} {form}: worst rms/L {wr:.3e} (gate {k_rms:.2e})  max/L {wm:.3e} (gate {k_max:.2e})")
                if np.isfinite(wr):
                    worst[0], worst[1] = max(worst[0], wr), max(worst[1], wm)
                assert not fails, (pid, signal, row, form, f"{len(fails)} hops miss the gate; (channel, hop, rms/L, max/L):", fails[:6])
    finally:
        for pv in handles.values():
            pv.close()
    print(f"level parity {pid}: worst so far rms/L {worst[0]:.3e}  max/L {worst[1]:.3e}")


SPECTRUM_MODES = [
    ("wg16_4096", 4096, 1024, 0, False),
    ("wg16_8192", 8192, 2048, 0, False),
    ("wave1024_fp64_forward", 1024, 256, FP64_FORWARD, False),
    ("wave2k_fp64_forward", 2048, 512, FP64_FORWARD, False),
    ("wave1024_default", 1024, 256, 0, True),                                 # class-A frames take X from the fp32 transform: the bound gains E_b per contribution
    ("wave2k_default", 2048, 512, 0, True),
]


@pytest.mark.parametrize("pitch", [1.5, 0.8])
@pytest.mark.parametrize("mode", SPECTRUM_MODES, ids=[m[0] for m in SPECTRUM_MODES])
def test_shifted_spectrum_bin_by_bin(mode, pitch):
    """|Yg[k] - Yr[k]| <= C(n) 2^-24 A[k] on every bin 1 .. H - 2 of three frames each of `loud_partial` (weak bins that carry signal 110 dB under the partial) and
    `fade` (a loud frame, one at the low end of the guarded range, the quietest), A[k] = the sum of |X[src]| over the n source bins that land on k
    (level_model.spectrum_bound derives C and names the terms of sources that are not fp64); a bin on which nothing lands is exactly 0.  f = 0.8 is the colliding scatter."""
    import phaze_amd
    pid, N, hop, flags, fp32_forward = mode
    H = N // 2 + 1
    k = np.arange(1, H - 1)
    worst = 0.0
    for signal in ("loud_partial", "fade"):
        taps = LM.oracle_taps(N, hop, signal, pitch)
        x = LM.corpus(N, hop)[signal][0]
        pv = phaze_amd.PhaseVocoder(fft_size=N, hop_size=hop, max_channels=1, max_hops=1, flags=flags)
        try:
            for m in range(max(taps) + 1):
                blk = np.ascontiguousarray(x[m * hop:(m + 1) * hop])
                if m in taps:
                    X, Yr, peaks = taps[m]
                    got = pv.debug_frame(0, blk, pitch)
                    assert np.array_equal(np.nonzero(got["flags"])[0], peaks), (signal, m, "peak set")
                    if not fp32_forward:
                        Xg = got["X"][0::2] + 1j * got["X"][1::2]
                        assert np.max(np.abs(Xg[:H] - X[:H])) < 1e-12 * np.max(np.abs(X[:H])), (signal, m, "fp64 forward spectrum")
                    Yg = (got["Y"][0::2] + 1j * got["Y"][1::2]).astype(np.complex128)
                    _, _, _, (A, n, n_res) = G.shift_spectrum(X[:H], X, np.float32(pitch), m * hop, N, contributions=True)
                    bound = LM.spectrum_bound(A, n, n_res, N, X, fp32_forward)
                    live = A[k] > 0
                    assert np.all(Yg[k][~live] == 0), (signal, m, "a bin on which nothing lands")
                    ratio = np.abs(Yg - Yr)[k][live] / bound[k][live]
                    kw = int(np.argmax(ratio))
                    print(f"spectrum {pid} {signal} frame {m} f={pitch}: worst |Yg - Yr| / bound {ratio[kw]:.3f} at bin {k[live][kw]} (n = {n[k][live][kw]}, {int(live.sum())} live bins)")
                    worst = max(worst, float(ratio[kw]))
                    assert ratio[kw] <= 1.0, (signal, m, int(k[live][kw]), float(ratio[kw]))
                assert pv.process([[blk]], [[np.zeros(hop, np.float32)]], {"pitchFactor": np.array([pitch], np.float32)}) is True
        finally:
            pv.close()
    print(f"spectrum {pid} f={pitch}: worst per-bin ratio to the bound {worst:.3f}")
