"""Throughput of the time-stretch kernels (pv_stretch_process_device), one JSON line per shape.

Same discipline as bench.py: HBM-resident input, `--warmup` untimed launches, then `--steps` launches bracketed by HIP events on the launch stream.
frames/s counts channel-frames; `hbm_fraction` is the algorithmic traffic of a frame, (ha + hs) * 4 B, against 8 TB/s.  Two comparison lines time the
pitch kernel on the same input: the headline form (pitchFactor 1.5), and the GPU part of the host speed path (pitch-shift-cli.js --speed 1.25: the input
resampled to 0.8x on the host, then the pitch kernel at pitchFactor 1 / 1.25), which produces the same output duration as a 1.25x stretch.  The tempo
line runs the mono 1024 shape through pv_tempo_process_device on a handle with floor 205, its schedule sweeping the analysis hop 205 -> 320 -> 205 (mean
262.5, next to the fixed 256): the per-frame position table against the fixed hop.  The linked lines (pv_link_channels) run the stereo 2048 shape
with G = 2, the 8-channel 4096 shape with G = 8 and as four stereo pairs (G = 2), each with its ratio to the unlinked line of the same shape.
The reset line (pv_transient_process_device) is the mono 1024 shape on the floor-205 handle at hop 256 with a hold every 64 frames (a flagged frame and
three more at hop 320 = hs), with its ratio to the tempo line; the strength line (pv_onset_strength_device) analyses the mono 1024 input at hop 256.
The resample lines (pv_resample_process_device) take the mono 1024 shape's stretched length, frames * 320 samples, down by 4/5 (taps in LDS) and by
147/160; their `hbm_fraction` is (M / L + 1) * 4 B per output against 8 TB/s.  The pitch line (pv_pitch_process_device) is the mono 1024 shape, 256 -> 320
and then 4/5, with its ratio to the stretch line of the same shape.
With --vari: the variable-ratio resampler (pv_vari_process_device) on the same stretched length in blocks of 320, once with counts alternating 256 /
257 (the fixed 4/5 line's neighbour) and once on a 200 .. 400 ramp, and the pitch-curve handle (pv_glide_process_device) on the mono 1024 shape with
the same two hop rows, with its ratio to the stretch line.
With --f0: only the f0 tracker (pv_f0_track_device) at W = 1024, max_lag = 1024, hop = 256, lags from 32, mono and 8 channels, --f0-frames frames per
channel of a harmonic tone; frames/s counts channel-frames, and `macs_per_s` is frames/s times the W * max_lag multiply-adds of a frame's lag products.
With --contour: the --f0 lines, then the same shapes and signals through the candidate kernel of the contour tracker (pv_contour_track_device) at K = 8, bias
1024, in the same process, each with its ratio to the --f0 line of the same shape.
With --psola: only the pitch-synchronous overlap-add kernel (pv_psola_process_device), 2^24 outputs mono, periods 192 .. 208 samples moved by 1.25; a
launch includes the host's validation of the grain table, the walk that finds every tile's grains and the upload of both.
With --epoch: only the epoch kernel (pv_epoch_track_device) at window 2048, hop 256, longest period 1024, mono and 8 channels, --f0-frames frames per
channel of a pulse train of period 217.3; frames/s counts channel-frames.
With --tsm: only the time-scale modification kernel (pv_tsm_process_device, max_period 1024, max_rate 2) on the --psola workload: 2^24 outputs mono,
periods 192 .. 208 moved by 1.25, at the rates 1, 1/2 and 2 (the input is rate times as long as the output); the --psola line runs first in the same
process: at rate 1 the two kernels do the same arithmetic on the same table.
With --harmony: only the harmony kernel (pv_harmony_process_device, max_period 1024, max_rate 2) on the --psola workload: 2^24 outputs mono, V = 4 voices
at the degrees (0, 2, 4, -3) of C major, gains 1/4, one grain table per voice from tsm_plan at rate 1; then what stands in for it without the kernel:
four pv_tsm_process_device calls into four buffers and a torch weighted sum.  Both lines are input-resident and use the same steps and warmup.
With --takes: only the per-take call (pv_takes_process_device, max_period 1024) against the loop it replaces: 256 takes of 2^16 outputs mono (--psola-outputs
in all), each with its own table, periods 192 .. 208 moved by 1.25; (a) all at rate 1 on a (1024, 2) configuration, (b) every 16th take planned at rate 4
on (1024, 4): tiles of mixed occupancy classes.  The yardstick is a loop of 256 pv_tsm_process_device calls on one Tsm of the same configuration, then one
synchronise.  Input-resident; the host's validation, walk and upload are inside the timed call; the outputs are asserted equal before timing; three runs
of each line, alternating, and their spread.
With --mirror: only the mirrored-grain kernel (pv_mirror_process_device, max_period 1024, max_rate 2) on the --tsm workload at rate 1/2 with every second
block of 64 records unvoiced: the plan with mirrored grains, the plan made with mirror = 0 through the same kernel, and that plan through
pv_tsm_process_device (asserted equal bit for bit before timing); three runs of each line, alternating, and their spread.
With --formant: only the warped-grain kernel (pv_formant_process_device, max_period 1024, max_rate 2) on the --tsm workload at rate 1: the unwarped plan
through pv_tsm_process_device and through the new kernel (asserted equal bit for bit before timing), and the same plan warped at 0.8 and at 1.5; three runs
of each line, alternating, and their spread.
With --choir: only the full-grain harmony kernel (pv_choir_process_device, max_period 1024, max_rate 2) on the --harmony workload: pv_harmony_process_device
on the four plain tables, pv_choir_process_device on the same tables (asserted equal bit for bit before timing), and pv_choir_process_device on four voices
planned by choir_plan at rate 1/2 with mirror on and the warps 1, 0.8, 1.25 and 0.8, every second block of 64 records unvoiced so that the mirrored warped
grains exist; three runs of each line, alternating, and their spread.

    python tools/bench_stretch.py [--steps 10] [--warmup 3] [--frames 1048576] [--vari] [--f0 [--f0-frames 16384]] [--psola] [--epoch] [--tsm] [--harmony] [--takes]
                                  [--mirror] [--formant] [--contour] [--choir]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def _time(torch, stream, fn, steps, warmup):
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def stretch_line(torch, phaze_amd, N, ha, hs, nch, T, steps, warmup, G=1):
    x = (torch.rand((nch, T * ha), device="cuda") - 0.5).contiguous()
    y = torch.empty((nch, T * hs), device="cuda")
    ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=nch, channels_per_group=G)
    stream = torch.cuda.Stream()
    ts.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: ts.process_device(x.data_ptr(), y.data_ptr(), nch, T, T * ha, T * hs), steps, warmup)
    ts.close()
    frames = nch * T
    return {"kernel": "pv_stretch" if G == 1 else "pv_link", "channels_per_group": G, "fft": N, "analysis_hop": ha, "synthesis_hop": hs, "channels": nch, "frames_per_channel": T, "ms_per_launch": round(ms, 4),
            "frames_per_s": frames / (ms * 1e-3), "hbm_fraction": frames * (ha + hs) * 4 / (ms * 1e-3) / HBM_BYTES_PER_S}


def tempo_line(torch, phaze_amd, N, lo, hi, hs, T, steps, warmup):
    period = 2 * (hi - lo)
    tri = np.abs((np.arange(T) % period) - (hi - lo))                # hi - lo .. 0 .. hi - lo
    hops = (hi - tri).astype(np.int32)
    n = int(hops.astype(np.int64).sum())
    x = (torch.rand((1, n), device="cuda") - 0.5).contiguous()
    y = torch.empty((1, T * hs), device="cuda")
    ts = phaze_amd.TimeStretch(N, lo, hs, max_channels=1)
    stream = torch.cuda.Stream()
    ts.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: ts.process_hops_device(x.data_ptr(), y.data_ptr(), 1, T, hops, n, T * hs), steps, warmup)
    ts.close()
    return {"kernel": "pv_tempo", "fft": N, "analysis_hop_min": int(hops.min()), "analysis_hop_max": int(hops.max()), "analysis_hop_mean": n / T,
            "synthesis_hop": hs, "channels": 1, "frames_per_channel": T, "ms_per_launch": round(ms, 4), "frames_per_s": T / (ms * 1e-3),
            "hbm_fraction": T * (n / T + hs) * 4 / (ms * 1e-3) / HBM_BYTES_PER_S}


def reset_line(torch, phaze_amd, N, lo, ha, hs, T, steps, warmup):
    m = np.arange(T) % 64
    hops = np.where(m < 4, hs, ha).astype(np.int32)                  # a hold of four unit-tempo frames every 64, the first one flagged
    resets = (m == 0).astype(np.uint8)
    n = int(hops.astype(np.int64).sum())
    x = (torch.rand((1, n), device="cuda") - 0.5).contiguous()
    y = torch.empty((1, T * hs), device="cuda")
    ts = phaze_amd.TimeStretch(N, lo, hs, max_channels=1)
    stream = torch.cuda.Stream()
    ts.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: ts.process_hops_device(x.data_ptr(), y.data_ptr(), 1, T, hops, n, T * hs, resets=resets), steps, warmup)
    ts.close()
    return {"kernel": "pv_transient", "fft": N, "analysis_hop_floor": lo, "analysis_hop_mean": n / T, "synthesis_hop": hs, "resets": int(resets.sum()), "channels": 1,
            "frames_per_channel": T, "ms_per_launch": round(ms, 4), "frames_per_s": T / (ms * 1e-3), "hbm_fraction": T * (n / T + hs) * 4 / (ms * 1e-3) / HBM_BYTES_PER_S}


def strength_line(torch, phaze_amd, N, ha, T, steps, warmup):
    x = (torch.rand((1, T * ha), device="cuda") - 0.5).contiguous()
    c = torch.empty((1, T), dtype=torch.int32, device="cuda")
    ts = phaze_amd.TimeStretch(N, ha, N // 4, max_channels=1)
    stream = torch.cuda.Stream()
    ts.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: ts.onset_strength_device(x.data_ptr(), 1, T, T * ha, c.data_ptr(), T), steps, warmup)
    ts.close()
    return {"kernel": "pv_onset_strength", "fft": N, "analysis_hop": ha, "channels": 1, "frames_per_channel": T, "ms_per_launch": round(ms, 4),
            "frames_per_s": T / (ms * 1e-3), "hbm_fraction": T * (ha + 1) * 4 / (ms * 1e-3) / HBM_BYTES_PER_S}


def resample_line(torch, phaze_amd, up, down, n, steps, warmup):
    rs = phaze_amd.Resampler(up, down, max_channels=1, max_samples=1)
    cap = -(-n * rs.up // rs.down) + 1
    x = (torch.rand((1, n), device="cuda") - 0.5).contiguous()
    y = torch.empty((1, cap), device="cuda")
    stream = torch.cuda.Stream()
    rs.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: rs.process_device(x.data_ptr(), 1, n, n, y.data_ptr(), cap, cap), steps, warmup)
    L, M, taps = rs.up, rs.down, rs.taps_per_phase
    rs.close()
    nout = n * L / M
    return {"kernel": "pv_resample", "up": L, "down": M, "taps_per_phase": taps, "channels": 1, "input_samples": n, "ms_per_launch": round(ms, 4),
            "outputs_per_s": nout / (ms * 1e-3), "hbm_fraction": nout * (M / L + 1) * 4 / (ms * 1e-3) / HBM_BYTES_PER_S}


def pitch_stretch_line(torch, phaze_amd, N, ha, hs, T, steps, warmup):
    p = phaze_amd.PitchStretch(N, ha, hs, max_channels=1, max_frames=T)
    cap = -(-T * hs * p.resampler.up // p.resampler.down) + 1
    x = (torch.rand((1, T * ha), device="cuda") - 0.5).contiguous()
    y = torch.empty((1, cap), device="cuda")
    stream = torch.cuda.Stream()
    p.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: p.process_device(x.data_ptr(), y.data_ptr(), 1, T, T * ha, cap, cap), steps, warmup)
    L, M = p.resampler.up, p.resampler.down
    p.close()
    return {"kernel": "pv_pitch", "fft": N, "analysis_hop": ha, "synthesis_hop": hs, "up": L, "down": M, "channels": 1, "frames_per_channel": T,
            "ms_per_launch": round(ms, 4), "frames_per_s": T / (ms * 1e-3), "hbm_fraction": T * (ha + hs * L / M) * 4 / (ms * 1e-3) / HBM_BYTES_PER_S}


def _vari_counts(kind, T):
    if kind == "alternating 256 / 257":
        return (256 + (np.arange(T) & 1)).astype(np.int32)
    return np.round(np.linspace(200, 400, T)).astype(np.int32)


def vari_line(torch, phaze_amd, kind, B, T, steps, warmup):
    counts = _vari_counts(kind, T)
    total = int(counts.astype(np.int64).sum())
    rs = phaze_amd.VariResampler(B, 200, 400, max_channels=1, max_blocks=1)
    x = (torch.rand((1, T * B), device="cuda") - 0.5).contiguous()
    y = torch.empty((1, total), device="cuda")
    stream = torch.cuda.Stream()
    rs.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: rs.process_device(x.data_ptr(), 1, counts, T * B, y.data_ptr(), total, total), steps, warmup)
    taps = rs.taps
    rs.close()
    return {"kernel": "pv_vari", "schedule": kind, "block": B, "taps": taps, "channels": 1, "input_samples": T * B, "ms_per_launch": round(ms, 4),
            "outputs_per_s": total / (ms * 1e-3), "hbm_fraction": (T * B + total) * 4 / (ms * 1e-3) / HBM_BYTES_PER_S}


def glide_line(torch, phaze_amd, kind, N, hs, T, steps, warmup):
    hops = _vari_counts(kind, T)
    total = int(hops.astype(np.int64).sum())
    p = phaze_amd.PitchGlide(N, hs, 200, 400, max_channels=1, max_frames=T)
    x = (torch.rand((1, total), device="cuda") - 0.5).contiguous()
    y = torch.empty((1, total), device="cuda")
    stream = torch.cuda.Stream()
    p.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: p.process_device(x.data_ptr(), y.data_ptr(), 1, hops, total, total), steps, warmup)
    p.close()
    return {"kernel": "pv_glide", "schedule": kind, "fft": N, "synthesis_hop": hs, "channels": 1, "frames_per_channel": T, "ms_per_launch": round(ms, 4),
            "frames_per_s": T / (ms * 1e-3), "samples_per_s": total / (ms * 1e-3), "hbm_fraction": 2 * total * 4 / (ms * 1e-3) / HBM_BYTES_PER_S}


def contour_line(torch, phaze_amd, W, hop, lo, ML, nch, T, steps, warmup, f0_ms):
    """f0_line's signal through the candidate kernel at K = 8."""
    K = 8
    n = (T - 1) * hop + W + ML
    k = torch.arange(n, device="cuda", dtype=torch.float32)
    x = torch.stack([sum(torch.sin(2 * np.pi * h * k / (217.3 + 31 * c)) / h for h in range(1, 6)) for c in range(nch)]).contiguous() * 0.3
    cand = torch.empty((nch, T, K, 4), dtype=torch.int32, device="cuda")
    trk = phaze_amd.ContourTracker(W, hop, lo, ML, candidates=K, max_channels=nch, max_frames=1)
    stream = torch.cuda.Stream()
    trk.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: trk.track_device(x.data_ptr(), nch, T, n, cand.data_ptr(), T), steps, warmup)
    trk.close()
    filled = int((cand[:, :, :, 0] > 0).sum().item())
    frames = nch * T
    return {"kernel": "pv_contour", "window": W, "hop": hop, "min_lag": lo, "max_lag": ML, "candidates": K, "channels": nch, "frames_per_channel": T,
            "slots_filled": filled, "ms_per_launch": round(ms, 4), "frames_per_s": frames / (ms * 1e-3), "macs_per_frame": W * ML,
            "macs_per_s": frames * W * ML / (ms * 1e-3), "hbm_fraction": frames * (hop * 4 + 16 * K) / (ms * 1e-3) / HBM_BYTES_PER_S,
            "ratio_to_f0": round(ms / f0_ms, 4)}


def f0_line(torch, phaze_amd, W, hop, lo, ML, nch, T, steps, warmup):
    n = (T - 1) * hop + W + ML
    k = torch.arange(n, device="cuda", dtype=torch.float32)
    x = torch.stack([sum(torch.sin(2 * np.pi * h * k / (217.3 + 31 * c)) / h for h in range(1, 6)) for c in range(nch)]).contiguous() * 0.3
    rec = torch.empty((nch, T, 4), dtype=torch.int32, device="cuda")
    trk = phaze_amd.F0Tracker(W, hop, lo, ML, max_channels=nch, max_frames=1)
    stream = torch.cuda.Stream()
    trk.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: trk.track_device(x.data_ptr(), nch, T, n, rec.data_ptr(), T), steps, warmup)
    trk.close()
    voiced = int((rec[:, :, 0] > 0).sum().item())
    frames = nch * T
    return {"kernel": "pv_f0", "window": W, "hop": hop, "min_lag": lo, "max_lag": ML, "channels": nch, "frames_per_channel": T, "voiced_frames": voiced,
            "ms_per_launch": round(ms, 4), "frames_per_s": frames / (ms * 1e-3), "macs_per_frame": W * ML, "macs_per_s": frames * W * ML / (ms * 1e-3),
            "hbm_fraction": frames * (hop * 4 + 16) / (ms * 1e-3) / HBM_BYTES_PER_S}


def epoch_line(torch, phaze_amd, window, hop, max_period, nch, T, steps, warmup):
    n = (T - 1) * hop + window
    k = torch.arange(n, device="cuda", dtype=torch.float32)
    x = torch.stack([torch.exp(-torch.remainder(k + 31 * c, 217.3) / 40.0) * torch.cos(2 * np.pi * torch.remainder(k + 31 * c, 217.3) / 40.0) for c in range(nch)]).contiguous() * 0.8
    per = torch.full((T,), int(217.3 * 256), dtype=torch.int32, device="cuda")
    rec = torch.empty((nch, T, 4), dtype=torch.int32, device="cuda")
    trk = phaze_amd.EpochTracker(window, hop, max_period, max_channels=nch, max_frames=1)
    stream = torch.cuda.Stream()
    trk.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: trk.track_device(x.data_ptr(), nch, T, n, per.data_ptr(), rec.data_ptr(), T), steps, warmup)
    trk.close()
    found = int((rec[:, :, 1] > 0).sum().item())
    frames = nch * T
    return {"kernel": "pv_epoch", "window": window, "hop": hop, "max_period": max_period, "channels": nch, "frames_per_channel": T, "frames_found": found,
            "ms_per_launch": round(ms, 4), "frames_per_s": frames / (ms * 1e-3), "hbm_fraction": frames * (hop * 4 + 16) / (ms * 1e-3) / HBM_BYTES_PER_S}


def psola_line(torch, phaze_amd, n, ratio, steps, warmup):
    hop = 256
    nrec = n // hop
    lag = 200 + (np.arange(nrec) // 64) % 17 - 8                       # periods 192 .. 208 samples, a new one every 64 records
    records = np.stack([lag, np.full(nrec, 700), np.zeros(nrec, np.int64), np.full(nrec, 324)], axis=1).astype(np.int32)      # + 0.184 by the parabola
    grains = phaze_amd.psola_plan(records, hop, hop // 2, n, 256.0, 32, 1024, np.full(nrec, ratio))
    x = (torch.rand((1, n), device="cuda") - 0.5).contiguous()
    y = torch.empty((1, n), device="cuda")
    ps = phaze_amd.Psola(1024, max_channels=1, max_outputs=1024)
    stream = torch.cuda.Stream()
    ps.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: ps.process_device(x.data_ptr(), n, n, 1, grains, y.data_ptr(), 0, n, n), steps, warmup)
    ps.close()
    return {"kernel": "pv_psola", "max_period": 1024, "ratio": ratio, "channels": 1, "outputs": n, "grains": int(grains.shape[0]), "ms_per_launch": round(ms, 4),
            "outputs_per_s": n / (ms * 1e-3), "hbm_fraction": 2 * n * 4 / (ms * 1e-3) / HBM_BYTES_PER_S}


def tsm_line(torch, phaze_amd, n, ratio, rate, steps, warmup):
    hop = 256
    nin = int(n * rate)
    nrec = nin // hop
    lag = 200 + (np.arange(nrec) // 64) % 17 - 8                       # psola_line's records
    records = np.stack([lag, np.full(nrec, 700), np.zeros(nrec, np.int64), np.full(nrec, 324)], axis=1).astype(np.int32)
    grains, nout = phaze_amd.tsm_plan(records, hop, hop // 2, nin, 256.0, 32, 1024, np.full(nrec, ratio), np.full(nrec, rate))
    x = (torch.rand((1, nin), device="cuda") - 0.5).contiguous()
    y = torch.empty((1, nout), device="cuda")
    ts = phaze_amd.Tsm(1024, 2, max_channels=1, max_outputs=1024)
    stream = torch.cuda.Stream()
    ts.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: ts.process_device(x.data_ptr(), nin, nin, 1, grains, y.data_ptr(), 0, nout, nout), steps, warmup)
    ts.close()
    return {"kernel": "pv_tsm", "max_period": 1024, "max_rate": 2, "ratio": ratio, "rate": rate, "channels": 1, "inputs": nin, "outputs": nout,
            "grains": int(grains.shape[0]), "ms_per_launch": round(ms, 4), "outputs_per_s": nout / (ms * 1e-3),
            "hbm_fraction": (nin + nout) * 4 / (ms * 1e-3) / HBM_BYTES_PER_S}


def mirror_lines(torch, phaze_amd, n, steps, warmup, runs=3):
    """tsm_line's workload at rate 1/2 with every second block of 64 records unvoiced, so that half of the material is repeated noise grains.  Three lines
    on the same input: pv_mirror_process_device on the plan with mirrored grains, the same kernel on the plan made with mirror = 0, and
    pv_tsm_process_device on that plan (whose output the second line must equal bit for bit); `runs` runs of each, alternating."""
    hop = 256
    nin = n // 2
    nrec = nin // hop
    lag = 200 + (np.arange(nrec) // 64) % 17 - 8                       # psola_line's records
    lag[(np.arange(nrec) // 64) % 2 == 1] = 0                          # no lag found: unvoiced
    records = np.stack([lag, np.full(nrec, 700), np.zeros(nrec, np.int64), np.full(nrec, 324)], axis=1).astype(np.int32)
    plan = (records, hop, hop // 2, nin, 256.0, 32, 1024, np.full(nrec, 1.25), np.full(nrec, 0.5))
    mirrored, nout = phaze_amd.mirror_plan(*plan, mirror=True)
    forward, nout_f = phaze_amd.mirror_plan(*plan, mirror=False)
    assert nout == nout_f and mirrored.shape == forward.shape
    x = (torch.rand((1, nin), device="cuda") - 0.5).contiguous()
    ys = [torch.empty((1, nout), device="cuda") for _ in range(3)]
    mh = phaze_amd.Mirror(1024, 2, max_channels=1, max_outputs=1024)
    ts = phaze_amd.Tsm(1024, 2, max_channels=1, max_outputs=1024)
    stream = torch.cuda.Stream()
    mh.set_stream(stream.cuda_stream)
    ts.set_stream(stream.cuda_stream)
    calls = [("pv_mirror", "mirror = 1", mirrored, lambda: mh.process_device(x.data_ptr(), nin, nin, 1, mirrored, ys[0].data_ptr(), 0, nout, nout)),
             ("pv_mirror", "mirror = 0", forward, lambda: mh.process_device(x.data_ptr(), nin, nin, 1, forward, ys[1].data_ptr(), 0, nout, nout)),
             ("pv_tsm", "mirror = 0", forward, lambda: ts.process_device(x.data_ptr(), nin, nin, 1, forward, ys[2].data_ptr(), 0, nout, nout))]
    torch.cuda.synchronize()
    for _, _, _, fn in calls:
        fn()
    mh.synchronize()
    ts.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(ys[1], ys[2]), "pv_mirror and pv_tsm disagree on a plan without mirrored grains"
    ms = [[] for _ in calls]
    for _ in range(runs):
        for k, (_, _, _, fn) in enumerate(calls):
            ms[k].append(_time(torch, stream, fn, steps, warmup))
    mh.close()
    ts.close()
    lines = []
    for (kernel, label, grains, _), v in zip(calls, ms):
        best = min(v)
        lines.append({"kernel": kernel, "plan": label, "max_period": 1024, "max_rate": 2, "ratio": 1.25, "rate": 0.5, "channels": 1, "inputs": nin, "outputs": nout,
                      "grains": int(grains.shape[0]), "mirrored_grains": int(np.sum((grains[:, 1] >> 16) & 1)), "ms_per_launch": round(best, 4),
                      "ms_per_launch_runs": [round(t, 4) for t in v], "spread": round((max(v) - best) / best, 4), "outputs_per_s": nout / (best * 1e-3),
                      "hbm_fraction": (nin + nout) * 4 / (best * 1e-3) / HBM_BYTES_PER_S})
    lines[0]["against_pv_tsm"] = round(min(ms[0]) / min(ms[2]), 4)
    lines[1]["against_pv_tsm"] = round(min(ms[1]) / min(ms[2]), 4)
    return lines


def formant_lines(torch, phaze_amd, n, steps, warmup, runs=3):
    """tsm_line's workload at rate 1 and ratio 1.25 (all voiced: every grain fractional).  Four lines on the same input: pv_tsm_process_device on the unwarped
    plan, pv_formant_process_device on it (whose output must equal the first bit for bit), and pv_formant_process_device on the same plan warped at 0.8 and
    at 1.5; `runs` runs of each, alternating."""
    hop = 256
    nin = n
    nrec = nin // hop
    lag = 200 + (np.arange(nrec) // 64) % 17 - 8                       # psola_line's records
    records = np.stack([lag, np.full(nrec, 700), np.zeros(nrec, np.int64), np.full(nrec, 324)], axis=1).astype(np.int32)
    plan = (records, hop, hop // 2, nin, 256.0, 32, 1024, np.full(nrec, 1.25), np.full(nrec, 1.0))
    plain, nout = phaze_amd.formant_plan(*plan)
    tables = {1.0: plain}
    for warp in (0.8, 1.5):
        tables[warp], nout_w = phaze_amd.formant_plan(*plan, warps=np.full(nrec, warp))
        assert nout_w == nout and tables[warp].shape == plain.shape
    x = (torch.rand((1, nin), device="cuda") - 0.5).contiguous()
    ys = [torch.empty((1, nout), device="cuda") for _ in range(4)]
    fh = phaze_amd.Formant(1024, 2, max_channels=1, max_outputs=1024)
    ts = phaze_amd.Tsm(1024, 2, max_channels=1, max_outputs=1024)
    stream = torch.cuda.Stream()
    fh.set_stream(stream.cuda_stream)
    ts.set_stream(stream.cuda_stream)
    calls = [("pv_tsm", 1.0, lambda: ts.process_device(x.data_ptr(), nin, nin, 1, plain, ys[0].data_ptr(), 0, nout, nout)),
             ("pv_formant", 1.0, lambda: fh.process_device(x.data_ptr(), nin, nin, 1, plain, ys[1].data_ptr(), 0, nout, nout)),
             ("pv_formant", 0.8, lambda: fh.process_device(x.data_ptr(), nin, nin, 1, tables[0.8], ys[2].data_ptr(), 0, nout, nout)),
             ("pv_formant", 1.5, lambda: fh.process_device(x.data_ptr(), nin, nin, 1, tables[1.5], ys[3].data_ptr(), 0, nout, nout))]
    torch.cuda.synchronize()
    for _, _, fn in calls:
        fn()
    fh.synchronize()
    ts.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1]), "pv_formant and pv_tsm disagree on a plan without warped grains"
    ms = [[] for _ in calls]
    for _ in range(runs):
        for k, (_, _, fn) in enumerate(calls):
            ms[k].append(_time(torch, stream, fn, steps, warmup))
    fh.close()
    ts.close()
    lines = []
    for (kernel, warp, _), v in zip(calls, ms):
        best, grains = min(v), tables[warp]
        lines.append({"kernel": kernel, "warp": warp, "step": int(round(256 * warp)), "max_period": 1024, "max_rate": 2, "ratio": 1.25, "rate": 1.0, "channels": 1,
                      "inputs": nin, "outputs": nout, "grains": int(grains.shape[0]), "warped_grains": int(np.sum((grains[:, 1] >> 17) != 0)),
                      "mean_half_length": round(float(grains[:, 3].mean()), 1), "ms_per_launch": round(best, 4), "ms_per_launch_runs": [round(t, 4) for t in v],
                      "spread": round((max(v) - best) / best, 4), "outputs_per_s": nout / (best * 1e-3), "hbm_fraction": (nin + nout) * 4 / (best * 1e-3) / HBM_BYTES_PER_S})
    lines[1]["against_pv_tsm"] = round(min(ms[1]) / min(ms[0]), 4)
    for k in (2, 3):
        lines[k]["against_unwarped"] = round(min(ms[k]) / min(ms[1]), 4)
    return lines


def harmony_lines(torch, phaze_amd, n, steps, warmup):
    hop = 256
    nrec = n // hop
    lag = 200 + (np.arange(nrec) // 64) % 17 - 8                       # psola_line's records
    records = np.stack([lag, np.full(nrec, 700), np.zeros(nrec, np.int64), np.full(nrec, 324)], axis=1).astype(np.int32)
    degrees = (0, 2, 4, -3)
    nv = len(degrees)
    ratios = phaze_amd.harmony_ratios(records, 48000.0, degrees, scale_mask=0xAB5)
    plans = [phaze_amd.tsm_plan(records, hop, hop // 2, n, 256.0, 32, 1024, ratios[v], np.ones(nrec)) for v in range(nv)]
    tables, nout = [g for g, _ in plans], plans[0][1]
    gains = np.full(nv, 1.0 / nv, np.float32)
    x = (torch.rand((1, n), device="cuda") - 0.5).contiguous()
    y = torch.empty((1, nout), device="cuda")
    stream = torch.cuda.Stream()
    hv = phaze_amd.Harmony(1024, 2, max_voices=nv, max_channels=1, max_outputs=1024)
    hv.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: hv.process_device(x.data_ptr(), n, n, 1, tables, gains, y.data_ptr(), 0, nout, nout), steps, warmup)
    hv.close()
    common = {"max_period": 1024, "max_rate": 2, "voices": nv, "degrees": list(degrees), "channels": 1, "inputs": n, "outputs": nout,
              "grains": [int(g.shape[0]) for g in tables]}
    fused = dict(common, kernel="pv_harmony", ms_per_launch=round(ms, 4), outputs_per_s=nout / (ms * 1e-3), hbm_fraction=(n + nout) * 4 / (ms * 1e-3) / HBM_BYTES_PER_S)
    # the same result without the kernel: one pv_tsm launch per voice into its own buffer, then a weighted sum
    ts = phaze_amd.Tsm(1024, 2, max_channels=1, max_outputs=1024)
    ts.set_stream(stream.cuda_stream)
    parts = torch.empty((nv, nout), device="cuda")
    w = torch.from_numpy(gains).cuda()
    z = torch.empty((1, nout), device="cuda")
    torch.cuda.synchronize()

    def separate():
        for v in range(nv):
            ts.process_device(x.data_ptr(), n, n, 1, tables[v], parts[v].data_ptr(), 0, nout, nout)
        torch.matmul(w[None, :], parts, out=z)

    ms2 = _time(torch, stream, separate, steps, warmup)
    ts.close()
    same = float((z - y).abs().max().item())
    apart = dict(common, kernel="pv_tsm x 4 + torch weighted sum", ms_per_launch=round(ms2, 4), outputs_per_s=nout / (ms2 * 1e-3),
                 hbm_fraction=(nv * n + (2 * nv + 1) * nout) * 4 / (ms2 * 1e-3) / HBM_BYTES_PER_S, max_abs_difference_to_fused=same,
                 fused_speedup=round(ms2 / ms, 4))
    return fused, apart


def choir_lines(torch, phaze_amd, n, steps, warmup, runs=3):
    """harmony_lines' workload (four voices at the degrees (0, 2, 4, -3) of C major, gains 1/4, 2^24 outputs mono).  Three lines: pv_harmony_process_device on
    the plain tables, pv_choir_process_device on the same tables (whose output must equal the first bit for bit), and pv_choir_process_device on the voices
    planned at rate 1/2 with mirror on and the warps 1, 0.8, 1.25, 0.8, every second block of 64 records unvoiced (mirror_lines' records) so that half of the
    material is repeated noise grains in alternating directions; `runs` runs of each, alternating."""
    hop = 256
    degrees, warps = (0, 2, 4, -3), (1.0, 0.8, 1.25, 0.8)
    nv = len(degrees)
    gains = np.full(nv, 1.0 / nv, np.float32)

    def records_of(nrec, noise):
        lag = 200 + (np.arange(nrec) // 64) % 17 - 8                   # psola_line's records
        if noise:
            lag[(np.arange(nrec) // 64) % 2 == 1] = 0                  # no lag found: unvoiced
        return np.stack([lag, np.full(nrec, 700), np.zeros(nrec, np.int64), np.full(nrec, 324)], axis=1).astype(np.int32)

    nrec = n // hop
    records = records_of(nrec, False)
    ratios = phaze_amd.harmony_ratios(records, 48000.0, degrees, scale_mask=0xAB5)
    plans = [phaze_amd.tsm_plan(records, hop, hop // 2, n, 256.0, 32, 1024, ratios[v], np.ones(nrec)) for v in range(nv)]
    plain, nout = [g for g, _ in plans], plans[0][1]
    nin2 = n // 2
    nrec2 = nin2 // hop
    records2 = records_of(nrec2, True)
    ratios2 = phaze_amd.harmony_ratios(records2, 48000.0, degrees, scale_mask=0xAB5)
    plans2 = [phaze_amd.choir_plan(records2, hop, hop // 2, nin2, 256.0, 32, 1024, ratios2[v], np.full(nrec2, 0.5), np.full(nrec2, warps[v]), mirror=True)
              for v in range(nv)]
    full, nout2 = [g for g, _ in plans2], plans2[0][1]
    x = (torch.rand((1, n), device="cuda") - 0.5).contiguous()
    ys = [torch.empty((1, max(nout, nout2)), device="cuda") for _ in range(3)]
    stream = torch.cuda.Stream()
    hv = phaze_amd.Harmony(1024, 2, max_voices=nv, max_channels=1, max_outputs=1024)
    ch = phaze_amd.Choir(1024, 2, max_voices=nv, max_channels=1, max_outputs=1024)
    hv.set_stream(stream.cuda_stream)
    ch.set_stream(stream.cuda_stream)
    calls = [("pv_harmony", "plain", plain, n, nout, lambda: hv.process_device(x.data_ptr(), n, n, 1, plain, gains, ys[0].data_ptr(), 0, nout, nout)),
             ("pv_choir", "plain", plain, n, nout, lambda: ch.process_device(x.data_ptr(), n, n, 1, plain, gains, ys[1].data_ptr(), 0, nout, nout)),
             ("pv_choir", "warps 1 / 0.8 / 1.25 / 0.8, mirror = 1, rate 1/2", full, nin2, nout2,
              lambda: ch.process_device(x.data_ptr(), nin2, nin2, 1, full, gains, ys[2].data_ptr(), 0, nout2, nout2))]
    torch.cuda.synchronize()
    for call in calls:
        call[-1]()
    hv.synchronize()
    ch.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(ys[0][:, :nout], ys[1][:, :nout]), "pv_choir and pv_harmony disagree on plain tables"
    ms = [[] for _ in calls]
    for _ in range(runs):
        for k, call in enumerate(calls):
            ms[k].append(_time(torch, stream, call[-1], steps, warmup))
    hv.close()
    ch.close()
    lines = []
    for (kernel, label, tables, nin, no, _), v in zip(calls, ms):
        best = min(v)
        words = np.concatenate([g[:, 1] for g in tables])
        lines.append({"kernel": kernel, "tables": label, "max_period": 1024, "max_rate": 2, "voices": nv, "degrees": list(degrees), "channels": 1, "inputs": nin,
                      "outputs": no, "grains": [int(g.shape[0]) for g in tables], "mirrored_grains": int(np.sum((words >> 16) & 1)),
                      "warped_grains": int(np.sum((words >> 17) != 0)), "mirrored_warped_grains": int(np.sum(((words >> 16) & 1) & ((words >> 17) != 0))),
                      "ms_per_launch": round(best, 4), "ms_per_launch_runs": [round(t, 4) for t in v], "spread": round((max(v) - best) / best, 4),
                      "outputs_per_s": no / (best * 1e-3), "hbm_fraction": (nin + no) * 4 / (best * 1e-3) / HBM_BYTES_PER_S})
    lines[1]["against_pv_harmony"] = round(min(ms[1]) / min(ms[0]), 4)
    lines[2]["against_plain"] = round(min(ms[2]) / min(ms[1]), 4)
    return lines


def takes_lines(torch, phaze_amd, total, ntakes, steps, warmup, runs=3):
    """Two workloads of `ntakes` takes with `total` outputs together, each take with its own table: (a) all at rate 1 on a (1024, 2) configuration, (b) every
    16th take planned at rate 4 on (1024, 4), which gives tiles of mixed occupancy classes.  Per workload the batched call (one pv_takes_process_device) and
    what the library could do without it (a loop of pv_tsm_process_device calls on one Tsm of the same configuration, then one synchronise), `runs` runs of
    each, alternating.  Both go through the raw C entry points on arguments built beforehand, so that the binding's per-call work is in neither."""
    import ctypes as C
    from phaze_amd import capi
    hop = 256
    per = total // ntakes
    lines = []
    for label, max_rate, fast_every in (("rate 1", 2, 0), ("every 16th take at rate 4", 4, 16)):
        xs, tables, nins, nouts = [], [], [], []
        for k in range(ntakes):
            rate = 4.0 if fast_every and k % fast_every == fast_every - 1 else 1.0
            nin = int(per * rate)
            nrec = nin // hop
            lag = 200 + ((np.arange(nrec) + 5 * k) // 64) % 17 - 8             # psola_line's records, from another place per take
            records = np.stack([lag, np.full(nrec, 700), np.zeros(nrec, np.int64), np.full(nrec, 324)], axis=1).astype(np.int32)
            g, nout = phaze_amd.tsm_plan(records, hop, hop // 2, nin, 256.0, 32, 1024, np.full(nrec, 1.25), np.full(nrec, rate))
            tables.append(np.ascontiguousarray(g))
            nins.append(nin)
            nouts.append(nout)
            xs.append((torch.rand((nin,), device="cuda") - 0.5).contiguous())
        ys = [torch.zeros((n,), device="cuda") for n in nouts]
        zs = [torch.zeros((n,), device="cuda") for n in nouts]
        stream = torch.cuda.Stream()
        tk = phaze_amd.Takes(1024, max_rate, max_channels=1, max_outputs=1024)
        ts = phaze_amd.Tsm(1024, max_rate, max_channels=1, max_outputs=1024)
        tk.set_stream(stream.cuda_stream)
        ts.set_stream(stream.cuda_stream)
        ip = C.POINTER(C.c_int32)
        arr = (capi._Take * ntakes)()
        for k in range(ntakes):
            arr[k] = capi._Take(xs[k].data_ptr(), nins[k], nins[k], tables[k].ctypes.data_as(ip), tables[k].shape[0], ys[k].data_ptr(), 0, nouts[k], nouts[k])
        loop_args = [(C.c_void_p(xs[k].data_ptr()), nins[k], nins[k], 1, tables[k].ctypes.data_as(ip), tables[k].shape[0], C.c_void_p(zs[k].data_ptr()), 0, nouts[k],
                      nouts[k]) for k in range(ntakes)]
        L = tk._L

        def batched():
            tk._check(L.pv_takes_process_device(tk._h, arr, ntakes, 1))

        def loop():
            for a in loop_args:
                ts._check(L.pv_tsm_process_device(ts._h, *a))

        torch.cuda.synchronize()
        batched()
        loop()
        tk.synchronize()
        ts.synchronize()
        torch.cuda.synchronize()
        assert all(torch.equal(y, z) for y, z in zip(ys, zs)), "the batched call and the loop disagree"
        tiles = phaze_amd.takes_tiles(1024, max_rate, tables, [0] * ntakes, nouts)
        ms = {"batched": [], "loop": []}
        for _ in range(runs):
            ms["batched"].append(_time(torch, stream, batched, steps, warmup))
            ms["loop"].append(_time(torch, stream, loop, steps, warmup))
        tk.close()
        ts.close()
        nout = int(sum(nouts))
        common = {"workload": label, "max_period": 1024, "max_rate": max_rate, "takes": ntakes, "channels": 1, "inputs": int(sum(nins)), "outputs": nout,
                  "grains": int(sum(g.shape[0] for g in tables)), "tiles_per_class": [int(np.sum(tiles[:, 6] == c)) for c in (1, 2, 3, 4)], "outputs_equal": True}
        for kernel, key in (("pv_takes (one call)", "batched"), (f"pv_tsm x {ntakes} (a loop of calls)", "loop")):
            v = ms[key]
            best = min(v)
            lines.append(dict(common, kernel=kernel, ms_per_launch=round(best, 4), ms_per_launch_runs=[round(t, 4) for t in v], spread=round((max(v) - best) / best, 4),
                              outputs_per_s=nout / (best * 1e-3), hbm_fraction=(sum(nins) + nout) * 4 / (best * 1e-3) / HBM_BYTES_PER_S))
        lines[-1]["batched_speedup"] = round(min(ms["loop"]) / min(ms["batched"]), 4)
    return lines


def pitch_line(torch, phaze_amd, label, N, hop, nch, T, pitch, steps, warmup):
    x = (torch.rand((nch, T * hop), device="cuda") - 0.5).contiguous()
    y = torch.empty_like(x)
    p = torch.full((T,), pitch, dtype=torch.float32, device="cuda")
    pv = phaze_amd.PhaseVocoder(fft_size=N, hop_size=hop, max_channels=nch, max_hops=1)
    stream = torch.cuda.Stream()
    pv.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    ms = _time(torch, stream, lambda: pv.process_batch_device(x.data_ptr(), y.data_ptr(), nch, T, T * hop, p.data_ptr(), 0, 1), steps, warmup)
    kernel = pv.info()["kernel_name"]
    pv.close()
    frames = nch * T
    return {"kernel": kernel, "label": label, "fft": N, "hop": hop, "pitch": pitch, "channels": nch, "frames_per_channel": T, "ms_per_launch": round(ms, 4),
            "frames_per_s": frames / (ms * 1e-3), "hbm_fraction": frames * 2 * hop * 4 / (ms * 1e-3) / HBM_BYTES_PER_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1 << 20, help="frames per channel of the mono 1024 shape (the others keep its sample count)")
    ap.add_argument("--no-compare", action="store_true", help="skip the two pitch-kernel comparison lines")
    ap.add_argument("--no-tempo", action="store_true", help="skip the variable-tempo line")
    ap.add_argument("--no-link", action="store_true", help="skip the linked-channel lines")
    ap.add_argument("--no-transient", action="store_true", help="skip the reset line and the onset-strength line")
    ap.add_argument("--no-resample", action="store_true", help="skip the two resample lines and the pitch-through-the-stretch line")
    ap.add_argument("--vari", action="store_true", help="add the variable-ratio resampler lines and the pitch-curve lines")
    ap.add_argument("--f0", action="store_true", help="only the f0 tracker lines")
    ap.add_argument("--f0-frames", type=int, default=16384, help="frames per channel of the f0 lines")
    ap.add_argument("--contour", action="store_true", help="the f0 tracker lines, then the same shapes through the contour tracker's candidate kernel at K = 8")
    ap.add_argument("--psola", action="store_true", help="only the pitch-synchronous overlap-add line")
    ap.add_argument("--psola-outputs", type=int, default=1 << 24, help="outputs of the overlap-add line")
    ap.add_argument("--epoch", action="store_true", help="only the epoch kernel lines (--f0-frames frames per channel)")
    ap.add_argument("--tsm", action="store_true", help="only the overlap-add line and the time-scale modification lines at the rates 1, 1/2 and 2 (--psola-outputs outputs)")
    ap.add_argument("--harmony", action="store_true", help="only the harmony line (four voices, --psola-outputs outputs) and the four launches plus mix it replaces")
    ap.add_argument("--takes", action="store_true", help="only the per-take lines (256 takes, --psola-outputs outputs in all) and the loops of pv_tsm calls they replace")
    ap.add_argument("--mirror", action="store_true", help="only the mirrored-grain lines: the --tsm workload at rate 1/2, half of its records unvoiced, through "
                    "pv_mirror and pv_tsm")
    ap.add_argument("--formant", action="store_true", help="only the warped-grain lines: the --tsm workload at rate 1 through pv_tsm and through pv_formant unwarped, "
                    "warped at 0.8 and at 1.5")
    ap.add_argument("--choir", action="store_true", help="only the full-grain harmony lines: the --harmony workload through pv_harmony and through pv_choir on plain "
                    "tables, and pv_choir with warped voices and mirror on at rate 1/2")
    args = ap.parse_args()
    import torch
    import phaze_amd
    if args.choir:
        for line in choir_lines(torch, phaze_amd, args.psola_outputs, args.steps, args.warmup):
            print(json.dumps(line), flush=True)
        return
    if args.formant:
        for line in formant_lines(torch, phaze_amd, args.psola_outputs, args.steps, args.warmup):
            print(json.dumps(line), flush=True)
        return
    if args.mirror:
        for line in mirror_lines(torch, phaze_amd, args.psola_outputs, args.steps, args.warmup):
            print(json.dumps(line), flush=True)
        return
    if args.takes:
        for line in takes_lines(torch, phaze_amd, args.psola_outputs, 256, args.steps, args.warmup):
            print(json.dumps(line), flush=True)
        return
    if args.harmony:
        for line in harmony_lines(torch, phaze_amd, args.psola_outputs, args.steps, args.warmup):
            print(json.dumps(line), flush=True)
        return
    if args.psola:
        print(json.dumps(psola_line(torch, phaze_amd, args.psola_outputs, 1.25, args.steps, args.warmup)), flush=True)
        return
    if args.tsm:
        print(json.dumps(psola_line(torch, phaze_amd, args.psola_outputs, 1.25, args.steps, args.warmup)), flush=True)
        for rate in (1.0, 0.5, 2.0):
            print(json.dumps(tsm_line(torch, phaze_amd, args.psola_outputs, 1.25, rate, args.steps, args.warmup)), flush=True)
        return
    if args.epoch:
        for nch in (1, 8):
            print(json.dumps(epoch_line(torch, phaze_amd, 2048, 256, 1024, nch, args.f0_frames, args.steps, args.warmup)), flush=True)
        return
    if args.f0 or args.contour:
        f0_ms = {}
        for nch in (1, 8):
            line = f0_line(torch, phaze_amd, 1024, 256, 32, 1024, nch, args.f0_frames, args.steps, args.warmup)
            f0_ms[nch] = line["ms_per_launch"]
            print(json.dumps(line), flush=True)
        if args.contour:
            for nch in (1, 8):
                print(json.dumps(contour_line(torch, phaze_amd, 1024, 256, 32, 1024, nch, args.f0_frames, args.steps, args.warmup, f0_ms[nch])), flush=True)
        return
    T = args.frames
    shapes = [(1024, 256, 320, 1, T), (2048, 512, 640, 2, T // 2), (4096, 1024, 1280, 8, T // 8)]
    unlinked = {}
    for N, ha, hs, nch, t in shapes:
        r = stretch_line(torch, phaze_amd, N, ha, hs, nch, max(t, 1), args.steps, args.warmup)
        unlinked[(N, nch)] = r["frames_per_s"]
        print(json.dumps(r), flush=True)
    if not args.no_link:
        for N, ha, hs, nch, t, G in [(2048, 512, 640, 2, T // 2, 2), (4096, 1024, 1280, 8, T // 8, 8), (4096, 1024, 1280, 8, T // 8, 2)]:
            r = stretch_line(torch, phaze_amd, N, ha, hs, nch, max(t, 1), args.steps, args.warmup, G)
            r["ratio_to_unlinked"] = round(r["frames_per_s"] / unlinked[(N, nch)], 4)
            print(json.dumps(r), flush=True)
    tempo = None
    if not args.no_tempo:
        tempo = tempo_line(torch, phaze_amd, 1024, 205, 320, 320, T, args.steps, args.warmup)
        print(json.dumps(tempo), flush=True)
    if not args.no_transient:
        r = reset_line(torch, phaze_amd, 1024, 205, 256, 320, T, args.steps, args.warmup)
        if tempo:
            r["ratio_to_tempo"] = round(r["frames_per_s"] / tempo["frames_per_s"], 4)
        print(json.dumps(r), flush=True)
        print(json.dumps(strength_line(torch, phaze_amd, 1024, 256, T, args.steps, args.warmup)), flush=True)
    if not args.no_resample:
        print(json.dumps(resample_line(torch, phaze_amd, 4, 5, T * 320, args.steps, args.warmup)), flush=True)
        print(json.dumps(resample_line(torch, phaze_amd, 147, 160, T * 320, args.steps, args.warmup)), flush=True)
        r = pitch_stretch_line(torch, phaze_amd, 1024, 256, 320, T, args.steps, args.warmup)
        r["ratio_to_stretch"] = round(r["frames_per_s"] / unlinked[(1024, 1)], 4)
        print(json.dumps(r), flush=True)
    if args.vari:
        for kind in ("alternating 256 / 257", "ramp 200 .. 400"):
            print(json.dumps(vari_line(torch, phaze_amd, kind, 320, T, args.steps, args.warmup)), flush=True)
        for kind in ("alternating 256 / 257", "ramp 200 .. 400"):
            r = glide_line(torch, phaze_amd, kind, 1024, 320, T, args.steps, args.warmup)
            r["ratio_to_stretch"] = round(r["frames_per_s"] / unlinked[(1024, 1)], 4)
            print(json.dumps(r), flush=True)
    if not args.no_compare:
        print(json.dumps(pitch_line(torch, phaze_amd, "pitch headline, same input", 1024, 256, 1, T, 1.5, args.steps, args.warmup)), flush=True)
        # --speed 1.25: 0.8x as many input frames after the host resampler, pitch 1 / 1.25: the same output duration as the 1.25x stretch above
        print(json.dumps(pitch_line(torch, phaze_amd, "speed path GPU part (--speed 1.25)", 1024, 256, 1, int(T * 0.8), 1 / 1.25, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
