"""The pitch contour tracker (pv_contour_*) on the GPU.  Every field of a candidate table is an exact integer function of its frame, so the device is compared
with tests/contour_model.py with `==` on all 4 K fields: at every shape where the kernel takes another path (odd tails, one and several passes over the
lags, one and several 256-sample accumulator blocks, the largest LDS layout), at K = 1, 3 and 8 and at both ends of the bias range, on tones (fewer dips than
slots), noise (far more), a full-scale square wave (plateaus and ties), a constant and a ramp, frames holding a NaN or an Inf, silence and a subnormal tone;
in the host and the device form, in pieces, twice, and through a staging buffer smaller than the call.  One cross-check does not rest on the new model: at
bias 0 slot 0 is the first argmin that F0Tracker reports for an unvoiced frame.  End to end, ContourTracker.track equals the model's path, and
Psola.process_tuned with a ContourTracker cuts whole-period grains on the fading tone where an F0Tracker of the same geometry cuts half-period ones."""
import json
import shutil
import subprocess

import numpy as np
import pytest

import contour_model as CM
import f0_model as FM
import psola_model as PM

pytestmark = pytest.mark.gpu

# (W, hop, min_lag, max_lag, the largest frame count tested)
SHAPES = [(48, 5, 2, 37, 70), (64, 16, 2, 64, 70), (257, 64, 2, 300, 70), (1024, 256, 32, 1024, 70), (4096, 4096, 2, 4096, 3)]
IDS = [f"W{s[0]}-lag{s[3]}" for s in SHAPES]
KS = (1, 3, 8)
BIASES = (0, 1024, 16384)
KINDS = ["tone", "noise", "square", "constant", "ramp", "nan", "inf", "zeros", "subnormal"]
_signals, _curves, _tables = {}, {}, {}


def _span(W, hop, ML, F):
    return (F - 1) * hop + W + ML


def _signal(kind, W, hop, ML, F):
    n = _span(W, hop, ML, F)
    rng = np.random.default_rng(W + 3 * ML)
    if kind == "tone":
        return (FM.tone("harm", ML / 3.3, n, 0.7) + 0.002 * rng.standard_normal(n)).astype(np.float32)
    if kind == "noise":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "zeros":
        return np.zeros(n, np.float32)
    if kind == "constant":
        return np.full(n, 0.37, np.float32)
    if kind == "ramp":
        return np.linspace(-0.9, 0.9, n).astype(np.float32)
    if kind == "nan":                                                       # the last sample of the last frame: the frames before it are clean
        x = _signal("tone", W, hop, ML, F)
        x[n - 1] = np.nan
        return x
    if kind == "inf":                                                       # the first sample: frame 0 alone holds it
        x = _signal("tone", W, hop, ML, F)
        x[0] = -np.inf
        return x
    if kind == "subnormal":
        return FM.tone("harm", ML / 2.7, n, 1e-41)
    if kind == "square":                                                    # one ulp under full scale: q = +-2048, c == 0 at every multiple of the period
        half = max(ML // 5, 2)
        return np.where((np.arange(n) // half) % 2 == 0, 1.0, -1.0).astype(np.float32) * np.nextafter(np.float32(1), np.float32(0))
    raise KeyError(kind)


def _model(kind, shape, K, bias):
    """(signal, model table int32[F, K, 4]) of one channel kind over `shape`, computed once and left unchanged; a shorter call's table is a prefix.  The c
    curve of a frame is computed once for every K and bias, and the table of K slots is the first K slots of the table of 8."""
    W, hop, lo, ML, F = shape
    if (kind, shape) not in _signals:
        x = _signal(kind, W, hop, ML, F)
        x.setflags(write=False)
        _signals[kind, shape] = x
        cs = []
        for m in range(F):
            q = FM.quantise(x[m * hop:m * hop + W + ML])
            cs.append(None if q is None else FM.curves(q, W, ML)[2])
        _curves[kind, shape] = cs
    if (kind, shape, bias) not in _tables:
        t = np.array([np.zeros((8, 4), np.int64) if c is None else CM.dips(c, lo, ML, 8, bias) for c in _curves[kind, shape]], np.int32).reshape(F, 8, 4)
        t.setflags(write=False)
        _tables[kind, shape, bias] = t
    return _signals[kind, shape], _tables[kind, shape, bias][:, :K]


def _device_track(trk, x, nframes, bias, pad=(3, 2)):
    """pv_contour_track_device on padded strides; returns the tables and checks that nothing beyond them was written."""
    import torch
    nch, n = x.shape
    d_in = torch.zeros((nch, n + pad[0]), dtype=torch.float32, device="cuda")
    d_in[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_cand = torch.full((nch, nframes + pad[1], trk.K, 4), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    trk.track_device(d_in.data_ptr(), nch, nframes, n + pad[0], d_cand.data_ptr(), nframes + pad[1], bias)
    trk.synchronize()
    out = d_cand.cpu().numpy()
    assert np.all(out[:, nframes:] == -77)
    return out[:, :nframes]


def test_the_model_is_the_definition_on_a_curve_by_hand():
    """The keys of a short curve worked out by hand, so that the comparisons below do not rest on one implementation alone."""
    c = np.array([16384, 9000, 500, 500, 700, 300, 300, 200, 900, 100, 400], np.int64)       # lags 0 .. 10: dips at 2 (c < before, <= after), 7, 9 ...
    got = CM.dips(c, 2, 10, 5, 0)                                                                # ... and at 5: the plateaus 2-3 and 5-6 count at their first lag
    assert got.tolist() == [[9, 900, 100, 400], [7, 300, 200, 900], [5, 700, 300, 300], [2, 9000, 500, 500], [0, 0, 0, 0]]
    assert CM.dips(c, 2, 10, 2, 16384)[:, 0].tolist() == [2, 5]                                 # keys 500 + 3276, 300 + 8192, 200 + 11468, 100 + 14745
    assert CM.dips(c, 3, 9, 8, 0)[:, 0].tolist() == [7, 5, 0, 0, 0, 0, 0, 0]                     # lag 9 = max_lag is outside, lag 2 below min_lag


def _stories(short, K, bias):
    """The model's tables of every kind, int32[kinds, F, K, 4], checked for what each kind is there to show."""
    want = np.stack([_model(k, short, K, bias)[1] for k in KINDS])
    full = np.stack([_model(k, short, 8, bias)[1] for k in KINDS])
    i = {k: j for j, k in enumerate(KINDS)}
    if short[3] >= 64:
        assert np.all(full[i["noise"], :, :, 0] > 0)                        # far more dips than slots
        assert np.all(full[i["tone"], :, 0, 0] > 0) and np.all(full[i["tone"], :, 7] == 0)          # fewer dips than slots: empty ones
    assert np.all(want[i["constant"]] == 0) and np.all(want[i["zeros"]] == 0)
    assert np.all(want[i["nan"], -1] == 0) and want[i["nan"], 0, 0, 0] > 0 and np.all(want[i["inf"], 0] == 0) and want[i["inf"], 1, 0, 0] > 0
    assert np.all(want[i["subnormal"], :, 0, 0] > 0)
    if bias == 0:
        assert np.all(want[i["square"], :, 0, 2] == 0) and np.all(want[i["square"], :, 0, 0] > 0)   # an exact repeat
    return want


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_kind_of_frame_equals_the_model(shape, K):
    import phaze_amd
    W, hop, lo, ML, _ = shape
    F = 2 if W == 4096 else 3
    short = (W, hop, lo, ML, F)
    x = np.stack([_model(k, short, K, 0)[0] for k in KINDS])
    trk = phaze_amd.ContourTracker(W, hop, lo, ML, candidates=K, max_channels=len(KINDS), max_frames=F)
    for bias in BIASES:
        want = _stories(short, K, bias)
        got = trk.candidates(x, bias)
        assert got.dtype == np.int32 and got.shape == want.shape
        for c, k in enumerate(KINDS):
            assert np.array_equal(got[c], want[c]), (k, bias, got[c].tolist(), want[c].tolist())
        assert np.array_equal(_device_track(trk, x, F, bias), want)         # the host form equals the device form
        assert np.array_equal(trk.candidates(x, bias), want)                # and a repeated run
    trk.close()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_tables_equal_the_model_at_every_frame_count_stride_and_bias(shape, K):
    import phaze_amd
    W, hop, lo, ML, Fmax = shape
    kinds = ["tone", "noise", "zeros"]
    trk = phaze_amd.ContourTracker(W, hop, lo, ML, candidates=K, max_channels=3, max_frames=4)      # the host form stages 70 frames in pieces of 4
    for bias in BIASES:
        for nframes in sorted({1, 2, Fmax}):
            n = _span(W, hop, ML, nframes)
            for nch in (1, 3):
                x = np.stack([_model(k, shape, K, bias)[0][:n] for k in kinds[:nch]])
                want = np.stack([_model(k, shape, K, bias)[1][:nframes] for k in kinds[:nch]])
                assert trk.frames(n) == nframes and trk.frames(n - 1) == nframes - 1
                got = trk.candidates(x, bias)
                assert np.array_equal(got, want), (bias, nframes, nch, np.argwhere(got != want)[:4].tolist())
                assert np.array_equal(_device_track(trk, x, nframes, bias), want), (bias, nframes, nch)
        if Fmax > 23:                                                       # the same stream in two pieces that overlap by W + max_lag - hop samples
            k = 23
            a = trk.candidates(x[:, :_span(W, hop, ML, k)], bias)
            b = trk.candidates(x[:, k * hop:], bias)
            assert a.shape[1] == k and b.shape[1] == Fmax - k and np.array_equal(np.concatenate([a, b], axis=1), want)
    trk.close()


@pytest.mark.parametrize("shape", SHAPES[:4], ids=IDS[:4])
def test_slot_0_at_bias_0_is_the_first_argmin_the_f0_tracker_reports(shape):
    """Not through the new model: with threshold 1 the f0 tracker calls every frame without an exact repeat unvoiced and reports b, the first argmin of c
    over [min_lag, max_lag - 1].  Where min_lag < b < max_lag - 1 that lag is a dip, and no dip has a smaller key at bias 0."""
    import phaze_amd
    W, hop, lo, ML, F = shape
    x = np.stack([_model(k, shape, 8, 0)[0] for k in ("tone", "noise")])
    f0 = phaze_amd.F0Tracker(W, hop, lo, ML, max_channels=2)
    rec = f0.track(x, threshold=1)
    f0.close()
    trk = phaze_amd.ContourTracker(W, hop, lo, ML, candidates=1, max_channels=2)
    got = trk.candidates(x, 0)[:, :, 0]
    trk.close()
    inner = (rec[:, :, 0] < -lo) & (rec[:, :, 0] > -(ML - 1))
    assert inner.sum() >= F                                                 # most frames of both channels
    want = np.array(rec)
    want[:, :, 0] *= -1
    assert np.array_equal(got[inner], want[inner])


def test_rejected_calls_return_before_any_device_work():
    import ctypes as C

    import phaze_amd
    import torch
    from phaze_amd import capi
    W, hop, lo, ML, K = 64, 16, 2, 64, 3
    trk = phaze_amd.ContourTracker(W, hop, lo, ML, candidates=K, max_channels=2, max_frames=4)
    n = _span(W, hop, ML, 5)
    d_in = torch.zeros((2, n), dtype=torch.float32, device="cuda")
    d_cand = torch.full((2, 8, K, 4), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ARG, CAP = capi.PV_ERR_ARGUMENT, capi.PV_ERR_CAPACITY
    for args, status, word in (((d_in.data_ptr(), 2, -1, n, d_cand.data_ptr(), 8, 1024), ARG, "negative"),
                               ((d_in.data_ptr(), -1, 5, n, d_cand.data_ptr(), 8, 1024), ARG, "negative"),
                               ((d_in.data_ptr(), 3, 5, n, d_cand.data_ptr(), 8, 1024), CAP, "max_channels"),
                               ((d_in.data_ptr(), 2, 5, n, d_cand.data_ptr(), 8, -1), ARG, "bias"),
                               ((d_in.data_ptr(), 2, 5, n, d_cand.data_ptr(), 8, 16385), ARG, "bias"),
                               ((None, 2, 5, n, d_cand.data_ptr(), 8, 1024), ARG, "null"),
                               ((d_in.data_ptr(), 2, 5, n, None, 8, 1024), ARG, "null"),
                               ((d_in.data_ptr(), 2, 5, n - 1, d_cand.data_ptr(), 8, 1024), ARG, "stride"),
                               ((d_in.data_ptr(), 2, 5, n, d_cand.data_ptr(), 4, 1024), ARG, "stride"),
                               ((d_in.data_ptr(), 2, 5, n, d_cand.data_ptr() + 4, 8, 1024), ARG, "aligned")):
        with pytest.raises(phaze_amd.PvError) as e:
            trk.track_device(*args)
        assert e.value.status == status and word in str(e.value), str(e.value)
    trk.synchronize()
    assert torch.all(d_cand == -77).item()                                  # nothing ran
    x = np.zeros((2, n), np.float32)
    cand = np.full((2, 5, K, 4), -77, np.int32)
    L = phaze_amd.load_library()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    assert L.pv_contour_track(trk._h, x.ctypes.data_as(fp), 2, 5, n - 1, 1024, cand.ctypes.data_as(ip), 5) == ARG
    assert L.pv_contour_track(trk._h, None, 2, 5, n, 1024, cand.ctypes.data_as(ip), 5) == ARG
    assert L.pv_contour_track(trk._h, x.ctypes.data_as(fp), 2, 5, n, 99999, cand.ctypes.data_as(ip), 5) == ARG
    assert L.pv_contour_track(trk._h, x.ctypes.data_as(fp), 3, 5, n, 1024, cand.ctypes.data_as(ip), 5) == CAP
    assert L.pv_contour_track(trk._h, x.ctypes.data_as(fp), 0, 5, n, 1024, cand.ctypes.data_as(ip), 5) == capi.PV_OK       # nothing to do
    assert np.all(cand == -77)                                              # the buffer of a refused call is untouched
    assert trk.candidates(np.zeros((1, W + ML - 1), np.float32)).shape == (1, 0, K, 4)
    trk.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------

GEOMETRY = (512, 128, 32, 512)


def test_track_equals_the_models_path():
    """Two channels with different stories: the fading tone (the path stays on the period) and tone / noise / tone (voiced, unvoiced, voiced)."""
    import phaze_amd
    a = CM.fading_tone(217.3, 0.97, 0.02)
    b = np.array(CM.fading_tone(100.37, 0.0, 0.02))
    b[6000:10000] = (0.2 * np.random.default_rng(1).standard_normal(12000)[6000:10000]).astype(np.float32)
    x = np.stack([a, b])
    trk = phaze_amd.ContourTracker(*GEOMETRY, max_channels=2)
    got = trk.track(x)
    other = trk.track(x, threshold=600)
    trk.close()
    assert got.dtype == np.int32 and got.shape == (2, 86, 4)
    for c in range(2):
        assert np.array_equal(got[c], CM.track(x[c], *GEOMETRY)), c
        assert np.array_equal(other[c], CM.track(x[c], *GEOMETRY, unvoiced_cost=600)), c
    assert CM.gross(got[0], 217.3) == 0 and np.all(got[0, :, 0] > 0) and CM.gross(got[1], 100.37) == 0 and np.any(got[1, :, 0] < 0)


def test_process_tuned_with_a_contour_tracker_cuts_whole_period_grains():
    """The user-visible difference, on the fading tone (P = 217.3, depth 0.97): Psola.process_tuned with a ContourTracker returns the grains of the model's plan
    on the model's path records, every half length L within 2 of 217; with an F0Tracker of the same geometry the frames read an octave up give grains
    with L below 130."""
    import phaze_amd
    x = CM.fading_tone(217.3, 0.97, 0.02)
    ps = phaze_amd.Psola(512)
    ct = phaze_amd.ContourTracker(*GEOMETRY)
    y, grains = ps.process_tuned(x, 48000, tracker=ct)
    ct.close()
    recs = CM.track(x, *GEOMETRY)
    want = PM.psola_plan(recs, 128, 512, x.size, 256.0, 32, 512, ratios=PM.tune_ratios(recs, 48000.0))
    assert np.array_equal(grains, want) and y.shape == x.shape and np.all(np.isfinite(y))
    assert np.all(np.abs(grains[:, 3] - 217) <= 2), (int(grains[:, 3].min()), int(grains[:, 3].max()))
    assert np.array_equal(y, ps.process(x, grains))
    f0 = phaze_amd.F0Tracker(*GEOMETRY)
    _, old = ps.process_tuned(x, 48000, tracker=f0)
    f0.close()
    ps.close()
    assert np.any(old[:, 3] < 130), int(old[:, 3].min())


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_contour_example_counts_no_gross_frame_on_the_path(tmp_path):
    import test_contour_abi as TCA
    exe = TCA.build_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    print(j)
    assert j["frames"] == 86 and j["gross_contour"] == 0 and j["unvoiced_contour"] == 0 and j["gross_f0"] >= 10
