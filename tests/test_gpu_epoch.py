"""The epoch kernel (EpochTracker / pv_epoch_*) on the GPU against the numpy model (tests/epoch_model.py), and Psola.process_tuned(epochs=True) end to
end.  A record is four integers, an exact function of the frame's samples and of its period: every comparison with the model is `==`."""
import ctypes as C
import json
import shutil
import subprocess

import numpy as np
import pytest

import epoch_model as EM
import f0_model as FM
import psola_model as PM

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int32)


def _span(window, hop, nframes):
    return (nframes - 1) * hop + window


def _want(x, window, hop, max_period, periods):
    return np.stack([EM.track(c, window, hop, max_period, periods, nframes=len(periods)) for c in x])


def _host(trk, x, periods, lead=1, pad_in=1, pad_rec=2):
    """pv_epoch_track on rows that start four bytes off numpy's alignment and are an odd number of floats apart; checks that nothing beyond the records
    was written."""
    nch, n = x.shape
    nframes = len(periods)
    buf = np.zeros(lead + nch * (n + pad_in), np.float32)
    rows = buf[lead:].reshape(nch, n + pad_in)
    rows[:, :n] = x
    per = np.ascontiguousarray(periods, np.int32)
    rec = np.full((nch, nframes + pad_rec, 4), -77, np.int32)
    trk._check(trk._L.pv_epoch_track(trk._h, rows.ctypes.data_as(FP), nch, nframes, n + pad_in, per.ctypes.data_as(IP), rec.ctypes.data_as(IP), nframes + pad_rec))
    assert np.all(rec[:, nframes:] == -77)
    return rec[:, :nframes]


def _device(trk, x, periods, lead=1, pad_in=1, pad_rec=2, stream=None):
    """pv_epoch_track_device on the same kind of rows (the records stay 16-byte aligned: one store each)."""
    import torch
    nch, n = x.shape
    nframes = len(periods)
    d_buf = torch.zeros(lead + nch * (n + pad_in), dtype=torch.float32, device="cuda")
    d_rows = d_buf[lead:].view(nch, n + pad_in)
    d_rows[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_per = torch.from_numpy(np.ascontiguousarray(periods, np.int32)).cuda()
    d_rec = torch.full((nch, nframes + pad_rec, 4), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert d_rows.data_ptr() % 16 == 4
    if stream is not None:
        trk.set_stream(stream.cuda_stream)
    trk.track_device(d_rows.data_ptr(), nch, nframes, n + pad_in, d_per.data_ptr(), d_rec.data_ptr(), nframes + pad_rec)
    trk.synchronize()
    if stream is not None:
        trk.set_stream(None)
    out = d_rec.cpu().numpy()
    assert np.all(out[:, nframes:] == -77)
    return out[:, :nframes]


def _pulses(rng, n, period, level=0.8):
    """A decaying pulse train of the given period over a little noise: something for the comb to find."""
    t = np.arange(n, dtype=np.float64)
    ph = np.mod(t + rng.uniform(0, period), period)
    return (level * np.exp(-ph / (period / 5.0)) * np.cos(2.0 * np.pi * ph / max(period / 4.0, 2.5)) + 0.02 * rng.standard_normal(n)).astype(np.float32)


def test_the_smallest_shape_at_its_period_edges():
    """Window 64, hop 16, longest period 32, 37 frames: the periods 8 (w = 2, the floor), 8 + 1/256, 17.3 and 32 (window = 2 max_period: one tooth), one
    and three channels, the host form in pieces of 5 frames."""
    import phaze_amd
    window, hop, mp, F = 64, 16, 32, 37
    rng = np.random.default_rng(41)
    periods = np.array([(256 * 8, 256 * 8 + 1, 4429, 256 * 32)[m % 4] for m in range(F)], np.int32)
    n = _span(window, hop, F)
    x = np.stack([_pulses(rng, n, 17.3), rng.standard_normal(n).astype(np.float32), _pulses(rng, n, 8.0, 3e-5)])
    want = _want(x, window, hop, mp, periods)
    assert np.all(want[:, :, 1] >= 1) and np.all(want[:, 3::4, 1] == 1) and np.all(want[:, 0::4, 2] == 2) and len(np.unique(want[0, :, 0])) > 8
    trk = phaze_amd.EpochTracker(window, hop, mp, max_channels=3, max_frames=5)
    assert trk.frames(n) == F and trk.frames(n - 1) == F - 1
    for nch in (1, 3):
        got = _host(trk, x[:nch], periods)
        assert got.dtype == np.int32 and np.array_equal(got, want[:nch]), np.argwhere(got != want[:nch])[:4].tolist()
        assert np.array_equal(_device(trk, x[:nch], periods), want[:nch])
    assert np.array_equal(trk.track(x, periods), want)
    trk.close()


def test_the_largest_shape_where_the_prefix_sums_wrap():
    """Window 8192, hop 4096, longest period 2048, 3 frames at the periods 2048, 8 and 2048.  Channel 0 is near full scale throughout, so the sum of q^2 over
    a frame passes 2^32 and the uint32 prefix sums of the kernel wrap; the differences it uses do not."""
    import phaze_amd
    window, hop, mp = 8192, 4096, 2048
    rng = np.random.default_rng(42)
    periods = np.array([256 * 2048, 256 * 8, 256 * 2048], np.int32)
    n = _span(window, hop, 3)
    loud = (np.sign(rng.standard_normal(n)) * rng.uniform(0.9, 0.999, n)).astype(np.float32)
    x = np.stack([loud, _pulses(rng, n, 2048.0), _pulses(rng, n, 8.0)])
    q = EM.quantise(loud[:window])
    assert int(np.sum(q * q)) > 1 << 32
    want = _want(x, window, hop, mp, periods)
    assert want[:, :, 1].tolist() == [[3, 1023, 3]] * 3 and want[:, :, 2].tolist() == [[512, 2, 512]] * 3
    trk = phaze_amd.EpochTracker(window, hop, mp, max_channels=3, max_frames=2)
    got = _host(trk, x, periods)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert np.array_equal(_device(trk, x, periods), want)
    trk.close()


def test_the_voice_at_three_phases_in_every_form():
    """Window 2048, hop 256, longest period 1024 on the two-formant voice of period 217.3 at three phases, one per channel: the host form in one call and
    in pieces of one frame, the device form on the handle's stream and on a user stream, and a repeated call all give the model's records."""
    import phaze_amd
    import torch
    window, hop, mp, F = 2048, 256, 1024, 6
    p = FM.period(PM.records_of([217.3])[0])
    p256 = int(EM.periods(PM.records_of([217.3]))[0])
    n = _span(window, hop, F)
    x = np.stack([PM.voice(p, n, phase=j / 8) for j in (0, 3, 4)])
    periods = np.full(F, p256, np.int32)
    want = _want(x, window, hop, mp, periods)
    lag = [((m * hop + int(want[c, m, 0]) - j / 8 * p) / p) % 1.0 * p for c, j in enumerate((0, 3, 4)) for m in range(F)]
    assert 4.0 < min(lag) and max(lag) < 8.0 and np.all(want[:, :, 3] > EM.S_ONE // 2)                 # a few samples after the pulse at every phase
    whole = phaze_amd.EpochTracker(window, hop, mp, max_channels=3, max_frames=F)
    ones = phaze_amd.EpochTracker(window, hop, mp, max_channels=3, max_frames=1)
    assert np.array_equal(_host(whole, x, periods), want)
    assert np.array_equal(_host(ones, x, periods), want)
    assert np.array_equal(_device(whole, x, periods), want)
    assert np.array_equal(_device(whole, x, periods, stream=torch.cuda.Stream()), want)
    assert np.array_equal(_host(whole, x, periods), want) and np.array_equal(whole.track(x, periods), want)
    assert np.array_equal(_host(whole, x[:1], periods[:1]), want[:1, :1])
    whole.close()
    ones.close()


def test_frames_without_a_record_do_not_touch_their_neighbours():
    """Frames that do not overlap (hop = window = 256, longest period 64): silence, a NaN, +Inf and -Inf, and periods out of range (data, not an error)
    give {0, 0, 0, 0} for that frame only; a constant frame has no step anywhere and gives the first candidate with strength 0; a frame of subnormal
    samples is scaled like any other."""
    import phaze_amd
    window = hop = 256
    mp, F = 64, 12
    rng = np.random.default_rng(43)
    x = _pulses(rng, F * window, 40.0)[None, :].copy()
    periods = np.full(F, 256 * 40, np.int32)
    x[0, 1 * window:2 * window] = 0.0
    x[0, 2 * window + 100] = np.nan
    x[0, 3 * window] = np.inf
    x[0, 4 * window + 255] = -np.inf
    x[0, 5 * window:6 * window] = 0.25
    periods[6], periods[7], periods[8], periods[9] = 0, 256 * 64 + 1, 256 * 8 - 1, -256 * 40
    x[0, 10 * window:11 * window] *= np.float32(2.0 ** -140)
    want = _want(x, window, hop, mp, periods)
    empty = [1, 2, 3, 4, 6, 7, 8, 9]
    assert np.all(want[0, empty] == 0) and np.all(want[0, [0, 10, 11], 1] >= 1) and np.all(want[0, [0, 10, 11], 3] > 0)
    assert want[0, 5].tolist() == [10, want[0, 0, 1], 10, 0]
    trk = phaze_amd.EpochTracker(window, hop, mp, max_frames=5)
    assert np.array_equal(_host(trk, x, periods), want)
    assert np.array_equal(_device(trk, x, periods), want)
    trk.close()


def test_refused_calls_leave_the_records_untouched():
    import phaze_amd
    import torch
    from phaze_amd import capi
    window, hop, mp = 64, 16, 32
    trk = phaze_amd.EpochTracker(window, hop, mp, max_channels=2, max_frames=4)
    n = _span(window, hop, 5)
    d_in = torch.zeros((2, n), dtype=torch.float32, device="cuda")
    d_per = torch.full((8,), 256 * 16, dtype=torch.int32, device="cuda")
    d_rec = torch.full((2, 8, 4), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ARG, CAP = capi.PV_ERR_ARGUMENT, capi.PV_ERR_CAPACITY
    i, q, r = d_in.data_ptr(), d_per.data_ptr(), d_rec.data_ptr()
    for args, status, word in (((i, 2, -1, n, q, r, 8), ARG, "negative"), ((i, -1, 5, n, q, r, 8), ARG, "negative"), ((i, 3, 5, n, q, r, 8), CAP, "max_channels"),
                               ((None, 2, 5, n, q, r, 8), ARG, "null"), ((i, 2, 5, n, None, r, 8), ARG, "null"), ((i, 2, 5, n, q, None, 8), ARG, "null"),
                               ((i, 2, 5, n - 1, q, r, 8), ARG, "stride"), ((i, 2, 5, n, q, r, 4), ARG, "stride"), ((i, 2, 1 << 31, n, q, r, 8), ARG, "frames"),
                               ((i, 2, 5, n, q, r + 4, 8), ARG, "aligned")):
        with pytest.raises(phaze_amd.PvError) as e:
            trk.track_device(*args)
        assert e.value.status == status and word in str(e.value), str(e.value)
    trk.synchronize()
    assert torch.all(d_rec == -77).item()                                   # nothing ran
    x = np.zeros((2, n), np.float32)
    per = np.full(5, 256 * 16, np.int32)
    rec = np.full((2, 5, 4), -77, np.int32)
    L = phaze_amd.load_library()
    xp, pp, rp = x.ctypes.data_as(FP), per.ctypes.data_as(IP), rec.ctypes.data_as(IP)
    assert L.pv_epoch_track(trk._h, xp, 2, 5, n - 1, pp, rp, 5) == ARG
    assert L.pv_epoch_track(trk._h, xp, 2, 5, n, pp, rp, 4) == ARG
    assert L.pv_epoch_track(trk._h, None, 2, 5, n, pp, rp, 5) == ARG
    assert L.pv_epoch_track(trk._h, xp, 2, 5, n, None, rp, 5) == ARG
    assert L.pv_epoch_track(trk._h, xp, 2, 5, n, pp, None, 5) == ARG
    assert L.pv_epoch_track(trk._h, xp, 3, 5, n, pp, rp, 5) == CAP
    assert L.pv_epoch_track(trk._h, xp, 2, -5, n, pp, rp, 5) == ARG
    assert L.pv_epoch_track(trk._h, xp, 0, 5, n, pp, rp, 5) == capi.PV_OK and L.pv_epoch_track(trk._h, xp, 2, 0, n, pp, rp, 5) == capi.PV_OK      # nothing to do
    assert np.all(rec == -77)
    with pytest.raises(ValueError):
        trk.track(x, np.full(6, 256 * 16, np.int32))                        # more periods than frames
    assert L.pv_epoch_track(trk._h, xp, 2, 5, n, pp, rp, 5) == capi.PV_OK and np.all(rec == 0)          # silence: empty records
    trk.close()
    assert L.pv_epoch_track(None, xp, 2, 5, n, pp, rp, 5) == ARG


def test_process_tuned_with_epochs_plans_the_models_grains_and_keeps_the_envelope():
    """The two-formant voice at 452 Hz (period 106.19) started half a period off the pulses, twelve thousand samples.  process_tuned(epochs=True) returns
    the model's grains (the f0 records are the model's, tests/test_gpu_f0.py, and the epoch records equal the model's here) and the bits of
    process(x, grains); the output's tracked note is 69 within the bound of tests/test_gpu_psola.py; and its envelope stays within the gate of
    tests/test_epoch_model.py: the deviation of a harmonic between 300 and 5000 Hz is at most the on-pulse figure of the unaligned path (the same plan on
    the phase-0 voice) plus 1 dB, with the strongest harmonic next to 1200 Hz.  epochs=False still returns today's grains and bits."""
    import phaze_amd
    n = FM.PLAN_LEN
    p = FM.SAMPLE_RATE / 452.0
    x = PM.voice(p, n, phase=0.5)[None, :]
    x0 = PM.voice(p, n)
    ps = phaze_amd.Psola(1024)
    y, grains = ps.process_tuned(x, FM.SAMPLE_RATE, epochs=True)
    recs = FM.track(x[0], 1024, 256, 32, 1024)
    ratios = PM.tune_ratios(recs, FM.SAMPLE_RATE)
    trk = phaze_amd.EpochTracker(2048, 256, 1024)
    ep = trk.track(x[0], phaze_amd.epoch_periods(recs))[0]
    trk.close()
    assert np.array_equal(ep, EM.track(x[0], 2048, 256, 1024, EM.periods(recs))) and np.all(ep[:, 1] >= 1)
    want = EM.epoch_plan(recs, 256, 1024, n, 256.0, 32, 1024, ratios=ratios, epochs=ep)
    plain = PM.psola_plan(recs, 256, 1024, n, 256.0, 32, 1024, ratios=ratios)
    assert np.all(recs[:, 0] > 0) and np.array_equal(grains, want) and not np.array_equal(grains, plain) and y.shape == x.shape
    assert np.array_equal(y, ps.process(x, grains))
    y_off, g_off = ps.process_tuned(x, FM.SAMPLE_RATE, epochs=False)
    y_def, g_def = ps.process_tuned(x, FM.SAMPLE_RATE)
    assert np.array_equal(g_off, plain) and np.array_equal(g_def, plain) and np.array_equal(y_off, ps.process(x, plain)) and np.array_equal(y_def, y_off)
    # the reference of the envelope gate: the unaligned plan with its marks on the pulses
    recs0 = FM.track(x0, 1024, 256, 32, 1024)
    y0 = ps.process(x0[None, :], PM.psola_plan(recs0, 256, 1024, n, 256.0, 32, 1024, ratios=PM.tune_ratios(recs0, FM.SAMPLE_RATE)))
    ps.close()
    out = FM.track(y[0, 2048:n - 1024], 1024, 256, 32, 1024)
    notes = [69.0 + 12.0 * np.log2(FM.SAMPLE_RATE / FM.period(r) / 440.0) for r in out]
    print("tracked notes of the output:", min(notes), max(notes))
    assert np.all(out[:, 0] > 0) and max(abs(v - 69.0) for v in notes) <= 12.0 * np.log2(1.0 + 2 * 1.5e-3)
    f, a, _ = PM.harmonic_amplitudes(x0, p, 3000, 9000)
    scale = float(np.median(a / PM._resonator_response(f * FM.SAMPLE_RATE, FM.SAMPLE_RATE)))
    p_out = FM.SAMPLE_RATE / 440.0

    def deviation(v):
        f, a, res = PM.harmonic_amplitudes(v, p_out, 3000, 9000)
        hz = f * FM.SAMPLE_RATE
        sel = (hz >= 300.0) & (hz <= 5000.0)
        dev = 20.0 * np.log10(a[sel] / (scale * PM._resonator_response(hz[sel], FM.SAMPLE_RATE)))
        return float(np.max(np.abs(dev))), float(hz[np.argmax(a)]), res

    on_pulse, _, _ = deviation(y0[0])
    dev, peak, res = deviation(y[0])
    unaligned, _, _ = deviation(y_off[0])
    print(f"envelope deviation: {dev:.2f} dB with epochs (strongest {peak:.0f} Hz, residual {res:.1e}), {unaligned:.2f} dB without, {on_pulse:.2f} dB with the marks on the pulses")
    assert dev <= on_pulse + 1.0 and abs(peak - 1200.0) < 440.0


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_epoch_example_runs_and_prints_its_line(tmp_path):
    import test_epoch_abi as TEA
    exe = TEA.build_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    print(j)
    assert j["epochs_found"] == j["frames_tracked"] and j["grains_moved"] > j["grains"] // 2
    assert abs(j["detected_note"] - (69.0 + 12.0 * np.log2(452.0 / 440.0))) < 0.03
    for key in ("corrected_note", "corrected_note_epochs"):
        assert abs(j[key] - 69.0) <= 12.0 * np.log2(1.0 + 2 * 1.5e-3), key
    assert abs(j["strongest_harmonic_in"] - 3 * 452.0) < 1.0 and abs(j["strongest_harmonic_out_epochs"] - 3 * 440.0) < 1.0
