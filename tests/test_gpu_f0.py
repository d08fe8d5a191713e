"""The f0 tracker (pv_f0_*) and pitch correction (PitchGlide.process_tuned) on the GPU.  Every record is an exact integer function of its frame, so the
device is compared with tests/f0_model.py with `==` on all four fields: at every shape where the kernel takes another path (odd tails, one and several
passes over the lags, one and several 256-sample accumulator blocks, the largest LDS layout), on tones, noise, frames holding a NaN or an Inf, silence, a
subnormal tone (the exact-scaling path) and a full-scale square wave (the accumulator-width path); in the host and the device form, in pieces, twice,
and through a staging buffer smaller than the call.  End to end, process_tuned plans what the model plans and moves a detuned tone onto its note."""
import json
import shutil
import subprocess

import numpy as np
import pytest

import f0_model as FM

pytestmark = pytest.mark.gpu

# (W, hop, min_lag, max_lag, the largest frame count tested)
SHAPES = [(48, 5, 2, 37, 70), (64, 16, 2, 64, 70), (257, 64, 2, 300, 70), (1024, 256, 32, 1024, 70), (4096, 4096, 2, 4096, 2)]
IDS = [f"W{s[0]}-lag{s[3]}" for s in SHAPES]
_cache = {}


def _span(W, hop, ML, F):
    return (F - 1) * hop + W + ML


def _channel(kind, W, hop, ML, F):
    n = _span(W, hop, ML, F)
    rng = np.random.default_rng(W + 3 * ML)
    if kind == "tone":
        return (FM.tone("harm", ML / 3.3, n, 0.7) + 0.002 * rng.standard_normal(n)).astype(np.float32)
    if kind == "noise":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "zeros":
        return np.zeros(n, np.float32)
    if kind == "nan":                                                       # the last sample of the last frame: the frames before it are clean
        x = _channel("tone", W, hop, ML, F)
        x[n - 1] = np.nan
        return x
    if kind == "inf":                                                       # the first sample: frame 0 alone holds it
        x = _channel("tone", W, hop, ML, F)
        x[0] = -np.inf
        return x
    if kind == "subnormal":
        return FM.tone("harm", ML / 2.7, n, 1e-41)
    if kind == "square":                                                    # one ulp under full scale: q = +-2048, every difference 4096
        half = max(ML // 5, 2)
        return np.where((np.arange(n) // half) % 2 == 0, 1.0, -1.0).astype(np.float32) * np.nextafter(np.float32(1), np.float32(0))
    raise KeyError(kind)


def _model(kind, shape, threshold=FM.DEFAULT_THRESHOLD):
    """(signal, model records) of one channel kind over the shape's largest frame count, computed once; a shorter call's records are a prefix."""
    key = (kind, shape, threshold)
    if key not in _cache:
        W, hop, lo, ML, F = shape
        x = _channel(kind, W, hop, ML, F)
        rec = FM.track(x, W, hop, lo, ML, threshold)
        x.setflags(write=False)
        rec.setflags(write=False)
        _cache[key] = (x, rec)
    return _cache[key]


def _device_track(trk, x, nframes, threshold=FM.DEFAULT_THRESHOLD, pad=(3, 2)):
    """pv_f0_track_device on padded strides; returns the records and checks that nothing beyond them was written."""
    import torch
    nch, n = x.shape
    d_in = torch.zeros((nch, n + pad[0]), dtype=torch.float32, device="cuda")
    d_in[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_rec = torch.full((nch, nframes + pad[1], 4), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    trk.track_device(d_in.data_ptr(), nch, nframes, n + pad[0], d_rec.data_ptr(), nframes + pad[1], threshold)
    trk.synchronize()
    out = d_rec.cpu().numpy()
    assert np.all(out[:, nframes:] == -77)
    return out[:, :nframes]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_kind_of_frame_equals_the_model(shape):
    import phaze_amd
    W, hop, lo, ML, _ = shape
    F = 2 if W == 4096 else 3
    kinds = ["tone", "noise", "nan", "inf", "zeros", "subnormal", "square"]
    short = (W, hop, lo, ML, F)
    x = np.stack([_model(k, short)[0] for k in kinds])
    want = np.stack([_model(k, short)[1] for k in kinds])
    assert np.all(want[0, :, 0] > 0) and np.all(want[1, :, 0] < 0) and np.all(want[4] == 0) and np.all(want[5, :, 0] > 0) and np.all(want[6, :, 0] > 0)
    assert np.all(want[2, -1] == 0) and want[2, 0, 0] > 0 and np.all(want[3, 0] == 0) and want[3, 1, 0] > 0
    trk = phaze_amd.F0Tracker(W, hop, lo, ML, max_channels=len(kinds), max_frames=F)
    got = trk.track(x)
    assert got.dtype == np.int32 and got.shape == want.shape
    for c, k in enumerate(kinds):
        assert np.array_equal(got[c], want[c]), (k, got[c].tolist(), want[c].tolist())
    dev = _device_track(trk, x, F)
    assert np.array_equal(dev, want)                                        # the host form equals the device form
    assert np.array_equal(trk.track(x), want)                               # and a repeated run
    trk.close()


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("nframes", [1, 2, 70])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_records_equal_the_model_at_every_frame_count_and_stride(shape, nframes, nch):
    import phaze_amd
    W, hop, lo, ML, Fmax = shape
    nframes = min(nframes, Fmax)
    kinds = ["tone", "noise", "zeros"][:nch]
    n = _span(W, hop, ML, nframes)
    x = np.stack([_model(k, shape)[0][:n] for k in kinds])
    want = np.stack([_model(k, shape)[1][:nframes] for k in kinds])
    trk = phaze_amd.F0Tracker(W, hop, lo, ML, max_channels=3, max_frames=4)     # the host form stages 70 frames in pieces of 4
    assert trk.frames(n) == nframes and trk.frames(n - 1) == nframes - 1
    got = trk.track(x)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert np.array_equal(_device_track(trk, x, nframes), want)
    if nframes > 2:                                                         # the same stream in two pieces that overlap by W + max_lag - hop samples
        k = 23
        a = trk.track(x[:, :_span(W, hop, ML, k)])
        b = trk.track(x[:, k * hop:])
        assert a.shape[1] == k and b.shape[1] == nframes - k and np.array_equal(np.concatenate([a, b], axis=1), want)
    trk.close()


@pytest.mark.parametrize("shape", SHAPES[1:4], ids=IDS[1:4])
def test_thresholds_at_both_ends_of_the_range(shape):
    """Threshold 1 passes only c == 0; 16384 passes every c below 2^14, so the pick is the first lag from min_lag on whose c is, walked down."""
    import phaze_amd
    W, hop, lo, ML, _ = shape
    short = (W, hop, lo, ML, 3)
    trk = phaze_amd.F0Tracker(W, hop, lo, ML, max_channels=2, max_frames=3)
    x = np.stack([_model("tone", short)[0], _model("square", short)[0]])
    for thr in (1, 16384):
        want = np.stack([_model("tone", short, thr)[1], _model("square", short, thr)[1]])
        assert np.array_equal(trk.track(x, thr), want), thr
        assert np.array_equal(_device_track(trk, x, 3, thr), want), thr
    one = np.concatenate([_model("tone", short, 1)[1], _model("square", short, 1)[1]])
    assert np.all((one[:, 0] < 0) | (one[:, 2] == 0)) and np.all(one[3:, 0] > 0)                   # the square wave repeats exactly: c == 0 at its period
    assert np.all(_model("tone", short, 16384)[1][:, 0] > 0)
    trk.close()


def test_rejected_calls_return_before_any_device_work():
    import phaze_amd
    import torch
    from phaze_amd import capi
    W, hop, lo, ML = 64, 16, 2, 64
    trk = phaze_amd.F0Tracker(W, hop, lo, ML, max_channels=2, max_frames=4)
    n = _span(W, hop, ML, 5)
    d_in = torch.zeros((2, n), dtype=torch.float32, device="cuda")
    d_rec = torch.full((2, 8, 4), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ARG, CAP = capi.PV_ERR_ARGUMENT, capi.PV_ERR_CAPACITY
    for args, status, word in (((d_in.data_ptr(), 2, -1, n, d_rec.data_ptr(), 8, 2458), ARG, "negative"),
                               ((d_in.data_ptr(), -1, 5, n, d_rec.data_ptr(), 8, 2458), ARG, "negative"),
                               ((d_in.data_ptr(), 3, 5, n, d_rec.data_ptr(), 8, 2458), CAP, "max_channels"),
                               ((d_in.data_ptr(), 2, 5, n, d_rec.data_ptr(), 8, 0), ARG, "threshold"),
                               ((d_in.data_ptr(), 2, 5, n, d_rec.data_ptr(), 8, 16385), ARG, "threshold"),
                               ((None, 2, 5, n, d_rec.data_ptr(), 8, 2458), ARG, "null"),
                               ((d_in.data_ptr(), 2, 5, n, None, 8, 2458), ARG, "null"),
                               ((d_in.data_ptr(), 2, 5, n - 1, d_rec.data_ptr(), 8, 2458), ARG, "stride"),
                               ((d_in.data_ptr(), 2, 5, n, d_rec.data_ptr(), 4, 2458), ARG, "stride"),
                               ((d_in.data_ptr(), 2, 5, n, d_rec.data_ptr() + 4, 8, 2458), ARG, "aligned")):
        with pytest.raises(phaze_amd.PvError) as e:
            trk.track_device(*args)
        assert e.value.status == status and word in str(e.value), str(e.value)
    trk.synchronize()
    assert torch.all(d_rec == -77).item()                                   # nothing ran
    x = np.zeros((2, n), np.float32)
    rec = np.zeros((2, 5, 4), np.int32)
    L = phaze_amd.load_library()
    import ctypes as C
    ip = C.POINTER(C.c_int32)
    fp = C.POINTER(C.c_float)
    assert L.pv_f0_track(trk._h, x.ctypes.data_as(fp), 2, 5, n - 1, 2458, rec.ctypes.data_as(ip), 5) == ARG
    assert L.pv_f0_track(trk._h, None, 2, 5, n, 2458, rec.ctypes.data_as(ip), 5) == ARG
    assert L.pv_f0_track(trk._h, x.ctypes.data_as(fp), 2, 5, n, 99999, rec.ctypes.data_as(ip), 5) == ARG
    assert L.pv_f0_track(trk._h, x.ctypes.data_as(fp), 0, 5, n, 2458, rec.ctypes.data_as(ip), 5) == capi.PV_OK      # nothing to do
    assert trk.track(np.zeros((1, W + ML - 1), np.float32)).shape == (1, 0, 4)
    trk.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------

def _two_harmonics(freq, n):
    ph = 2.0 * np.pi * freq * np.arange(n) / FM.SAMPLE_RATE
    return (0.5 * np.sin(ph) + 0.25 * np.sin(2.0 * ph)).astype(np.float32)


def test_process_tuned_plans_what_the_model_plans_and_lands_on_the_note():
    """A 452 Hz two-harmonic tone through PitchGlide(1024, 256, 128, 512).process_tuned: the hops are the model's plan of the model's records, the output
    is bit for bit PitchGlide.process(x, hops), and its tracked period agrees with that of the constant row tempo_hops(452 / 440) within 3e-3 relative
    (twice the tracker's bound: the vocoder's own colouring is in both, what remains is the jitter of the planned row).  Frames inside the glide's lag are
    skipped.  Measured on an MI355X: worst relative difference 1.04e-3, mean 1.1e-4, corrected note 68.9997 (DESIGN.md "Pitch tracking")."""
    import phaze_amd
    N, HS, LO, HI = 1024, 256, 128, 512
    n = 24000
    x = _two_harmonics(452.0, n)
    g = phaze_amd.PitchGlide(N, HS, LO, HI, max_frames=96)
    y, hops = g.process_tuned(x, FM.SAMPLE_RATE)
    recs = FM.track(x, N, HS, 32, N)
    want_hops, _ = FM.tune_plan(recs, HS, N, FM.SAMPLE_RATE, HS, LO, HI, n)
    assert np.array_equal(hops, want_hops) and hops.dtype == np.int32
    total = int(hops.sum())
    assert y.shape == (total,) and n - HI < total <= n
    g.reset()
    assert np.array_equal(g.process(x[:total], hops).view(np.uint32), y.view(np.uint32))
    # the parent's own path: the constant row of the exact ratio
    const, _ = phaze_amd.tempo_hops(np.full(hops.size, 452.0 / 440.0), HS, LO, HI)
    g.reset()
    y_const = g.process(x[:int(const.sum())], const)
    trk = phaze_amd.F0Tracker(N, HS, 32, N)
    skip = -(-(g.latency + 2 * N) // HS)                                    # the documented lag and the stretch's onset, in frames of about hs samples
    p_tuned = phaze_amd.f0_period(trk.track(y)[0])[skip:]
    p_const = phaze_amd.f0_period(trk.track(y_const)[0])[skip:]
    m = min(p_tuned.size, p_const.size)
    assert m >= 40 and np.all(p_tuned[:m] > 0) and np.all(p_const[:m] > 0)
    rel = np.abs(p_tuned[:m] / p_const[:m] - 1.0)
    note = 69.0 + 12.0 * np.log2(FM.SAMPLE_RATE / np.median(p_tuned) / 440.0)
    print(f"tuned against the constant row: worst relative period difference {rel.max():.3e}, mean {rel.mean():.3e}; corrected note {note:.4f}")
    assert rel.max() <= 3e-3
    trk.close()
    g.close()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_tune_example_detects_and_corrects(tmp_path):
    import test_f0_abi as TFA
    exe = TFA.build_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    print(j)
    detune = 12.0 * np.log2(452.0 / 440.0)                                  # 0.466 semitones
    # the tracker's 1.5e-3 relative is 0.026 semitones; the corrected tone carries the vocoder's colouring as well: it must have come most of the way
    assert j["voiced"] == j["frames_tracked"] and abs(j["detected_note"] - (69.0 + detune)) <= 0.026
    assert j["voiced_out"] > 40 and abs(j["corrected_note"] - 69.0) <= 0.1
    assert abs(j["mean_hop"] / (256.0 * 452.0 / 440.0) - 1.0) <= 1e-3
