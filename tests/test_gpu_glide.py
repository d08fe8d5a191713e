"""PitchGlide (pv_glide_*) on the GPU: the handle is a TimeStretch on a hop row followed by a VariResampler on the same row, bit for bit and state for
state, in every call form; the output is as long as the input; a constant row shifts a tone by hs / hop; tones through it fit the closed form of
tests/test_resample_model.py at the gate tests/test_gpu_pitch.py uses for the fixed-ratio pair; a linked pair keeps its inter-channel phase.  The
stretch stage is compared GPU against GPU and the resampler has no decisions, so no frame needs to be set aside as doubtful."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import resample_model as RM
import test_resample_model as TRM
import test_vari_model as TVM
import tones
from link_model import stereo_partials, wrap
from test_gpu_link import PHASE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 61
# (N, hs, min_hop, max_hop)
SHAPES = [(256, 64, 16, 256), (1024, 320, 200, 440)]


def _input(N, nch, n, seed):
    rng = np.random.default_rng(seed)
    k = np.arange(n, dtype=np.float64)
    x = np.stack([0.4 * np.cos(2 * np.pi * (60.3 + 11 * c) * k / N + c) + 0.2 * np.cos(2 * np.pi * 171.7 * k / N) + 0.05 * rng.standard_normal(n)
                  for c in range(nch)])
    x[:, n // 2:n // 2 + 40] += 0.8 * rng.standard_normal((nch, 40))             # an attack for the resets to carry
    return x.astype(np.float32)


def _schedule(kind, rng, HS, LO, HI):
    """Random hops over the whole range with both ends present, six frames in the middle at unit pitch (hop == hs)."""
    hops = rng.integers(LO, HI + 1, FRAMES).astype(np.int32)
    hops[[1, 2, 3, 4]] = [LO, HI, LO, HI]
    hops[FRAMES // 2:FRAMES // 2 + 6] = HS
    if kind == "hops":
        return hops, None
    resets = np.zeros(FRAMES, np.uint8)
    resets[[0, FRAMES // 2, FRAMES - 1]] = 1
    return hops, resets


def _states(stretch, resampler, nch):
    st = []
    for c in range(nch):
        st += [np.asarray(a).view(np.uint32).copy() for a in stretch.export_state(c)]
        h, i, j = resampler.export_state(c)
        st += [h.view(np.uint32).copy(), np.array([i, j], np.int64)]
    return st


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("kind", ["hops", "resets"])
@pytest.mark.parametrize("N,HS,LO,HI", SHAPES)
def test_glide_handle_is_stretch_then_variable_resampler_bit_for_bit(N, HS, LO, HI, G, kind):
    import phaze_amd
    import torch
    nch = 2
    rng = np.random.default_rng(23 + G)
    hops, resets = _schedule(kind, rng, HS, LO, HI)
    at = np.concatenate([[0], np.cumsum(hops.astype(np.int64))])
    x = _input(N, nch, int(at[-1]), 5)

    ts = phaze_amd.TimeStretch(N, LO, HS, max_channels=nch, max_frames=FRAMES, channels_per_group=G)
    rs = phaze_amd.VariResampler(HS, LO, HI, max_channels=nch, max_blocks=FRAMES)
    want = rs.process(ts.process_hops(x, hops, resets), hops)
    assert want.shape == x.shape and x.shape[1] > 3 * 1024                       # the output is as long as the input
    want_state = _states(ts, rs, nch)

    def same(p, y, what):
        assert y.shape == want.shape and np.array_equal(y.view(np.uint32), want.view(np.uint32)), what
        got = _states(p.stretch, p.resampler, nch)
        assert len(got) == len(want_state) and all(np.array_equal(a, b) for a, b in zip(got, want_state)), what

    for cuts in ([FRAMES], [1, 7, FRAMES - 8], [20, 2, 39], [3] * 20 + [1]):
        p = phaze_amd.PitchGlide(N, HS, LO, HI, max_channels=nch, max_frames=4, channels_per_group=G)
        assert p.latency == N - HS + p.resampler.half_width
        parts, f0 = [], 0
        for nf in cuts:
            y = p.process(x[:, at[f0]:at[f0 + nf]], hops[f0:f0 + nf], None if resets is None else resets[f0:f0 + nf])
            assert y.shape == (nch, at[f0 + nf] - at[f0])
            parts.append(y)
            f0 += nf
        assert f0 == FRAMES
        same(p, np.concatenate(parts, axis=1), cuts)
        p.close()

    # the device form on a user stream, two calls, padded strides
    p = phaze_amd.PitchGlide(N, HS, LO, HI, max_channels=nch, max_frames=1, channels_per_group=G)
    stream = torch.cuda.Stream()
    p.set_stream(stream.cuda_stream)
    n = x.shape[1]
    d_in = torch.zeros((nch, n + 3), dtype=torch.float32, device="cuda")
    d_in[:, :n] = torch.from_numpy(x).cuda()
    d_out = torch.full((nch, n + 9), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    f0 = 0
    for nf in (25, FRAMES - 25):
        p.process_device(d_in.data_ptr() + 4 * int(at[f0]), d_out.data_ptr() + 4 * int(at[f0]), nch, hops[f0:f0 + nf], n + 3, n + 9,
                         None if resets is None else resets[f0:f0 + nf])
        f0 += nf
    p.synchronize()
    yd = d_out.cpu().numpy()
    assert np.all(yd[:, n:] == -77.0)
    same(p, np.ascontiguousarray(yd[:, :n]), "device form")
    # refused with both states untouched: a hop outside the handle's range, a reset flag that is no flag, a stride below the row
    for bad_hops, bad_resets, stride, word in (([LO, HI + 1, LO], None, n + 3, "frame 1"), ([LO - 1, HI, LO], None, n + 3, "frame 0"),
                                               ([LO, HI, LO], [0, 2, 0], n + 3, "reset"), ([LO, HI, LO], None, LO + HI, "stride")):
        with pytest.raises(phaze_amd.PvError) as e:
            p.process_device(d_in.data_ptr(), d_out.data_ptr(), nch, np.array(bad_hops, np.int32), stride, n + 9,
                             None if bad_resets is None else np.array(bad_resets, np.uint8))
        assert e.value.status == phaze_amd.capi.PV_ERR_ARGUMENT and word in str(e.value), str(e.value)
    p.synchronize()
    same(p, np.ascontiguousarray(d_out.cpu().numpy()[:, :n]), "after refused calls")
    p.set_stream(None)
    p.close()
    ts.close()
    rs.close()


def _crossing_rate(y):
    """Positive-going zero crossings per sample, first to last."""
    i = np.flatnonzero((y[:-1] < 0) & (y[1:] >= 0))
    return (i.size - 1) / float(i[-1] - i[0])


@pytest.mark.parametrize("N,HS,hop", [(256, 64, 80), (256, 64, 50), (1024, 320, 256), (1024, 320, 400)])
def test_a_constant_schedule_shifts_a_tone_by_hs_over_hop(N, HS, hop):
    """Zero crossings over at least 24 N samples behind the handle's lag: a few parts in 10^4, the 2e-3 of tests/test_resample_abi.py."""
    import phaze_amd
    f0 = 20.3 / N                                                                # cycles per sample; x hs / hop stays well inside the band
    T = -(-30 * N // hop)
    x = (0.5 * np.sin(2 * np.pi * f0 * np.arange(T * hop))).astype(np.float32)
    p = phaze_amd.PitchGlide(N, HS, min(hop, HS), max(hop, HS), max_frames=T)
    y = p.process(x, np.full(T, hop, np.int32))
    assert y.shape == x.shape
    lag = -(-(p.latency + N) * hop // HS)                                        # the documented lag and the stretch's onset, in output samples
    assert y.size - lag >= 24 * N
    got = _crossing_rate(y[lag:]) / f0
    print(f"N {N} hs {HS} hop {hop}: pitch factor {got:.6f}, hs / hop {HS / hop:.6f}")
    assert abs(got / (HS / hop) - 1.0) < 2e-3
    p.close()


@pytest.mark.parametrize("name", sorted(TVM.GLIDE_CASES))
def test_tones_through_the_glide_handle_fit_the_closed_form(name):
    """Gate: 4 x the figures of the model composition, StretchModel then the variable model (tests/test_vari_model.py GLIDE_MEASURED): the practice
    of tests/test_gpu_pitch.py for the fixed-ratio pair, for the same reason -- the stretch's f32 transforms against the model's fp64 ones move the
    fit by about its own size, and a wrong position or weight moves it by orders of magnitude."""
    import phaze_amd
    N, hop, hs, freqs, amps = TVM.GLIDE_CASES[name]
    T, _ = tones.case_input(N, hop, hs, freqs, amps)
    p = phaze_amd.PitchGlide(N, hs, hop, hop, max_frames=T)
    ratio, res = TVM.glide_fit(name, process=p.process)
    amp_gate, res_gate = (4 * v for v in TVM.GLIDE_MEASURED[name])
    print(f"gpu glide {name}: amplitude ratio - 1 {ratio - 1}, residual {res:.3e} (gates {amp_gate:.1e}, {res_gate:.1e})")
    assert np.max(np.abs(ratio - 1.0)) <= amp_gate and res <= res_gate, (ratio, res)
    p.close()


def test_a_linked_pair_keeps_its_inter_channel_phase_through_the_glide_handle():
    import phaze_amd
    n, hop, hs = 1024, 256, 320
    lo, _ = tones.steady_range(n, hop, hs, 0)
    T = -(-(lo + 9 * n) // hs)
    f = [round(n * 0.0629) + 0.37, round(n * 0.15) + 0.81]
    amps, ph = [[0.4, 0.15], [0.2, 0.3]], [[0.3, 1.1], [0.3 + np.pi / 2, 1.1 + 2.2]]
    x = stereo_partials(n, f, amps, ph, T * hop)
    dphi = wrap(np.subtract(ph[1], ph[0]))
    L, M = RM.reduce_ratio(hop, hs)
    out = {}
    for G in (1, 2):
        p = phaze_amd.PitchGlide(n, hs, hop, hop, max_channels=2, max_frames=T, channels_per_group=G)
        W = p.resampler.half_width
        y = p.process(x, np.full(T, hop, np.int32))
        fit = TRM.pitch_phase_fit(y[:, W * hop // hs:], T * hs - W, n, hop, hs, L, M, f)
        p.close()
        out[G] = np.abs(wrap(fit[1] - fit[0] - dphi))
    print(f"inter-channel phase through the glide handle: linked {out[2].max():.3e} rad, unlinked {out[1].max():.3e} rad (gate {PHASE:.1e})")
    assert out[2].max() <= PHASE, out
    assert out[1].max() > 0.1, out                                     # the unlinked handle does not keep it: the check discriminates


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
@pytest.mark.parametrize("args", [[], ["1024", "256", "320", "160", "300"]])
def test_glide_example_reports_one_call_equals_pieces_and_the_ramp(tmp_path, args):
    import test_vari_abi as TVA
    exe = TVA.build_example(tmp_path)
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["one_call_equals_pieces"] is True and j["input_samples"] == j["output_samples"]
    # 2e-2: the estimate counts whole cycles between two crossings of a tone whose pitch moves by up to a factor 1.4 within the quarter, and where the
    # curve acts is known to about a window, N samples of the quarter's 2 .. 4 10^4: N / quarter x the movement is 1 .. 2 10^-2
    for part in ("first", "last"):
        assert abs(j[f"measured_pitch_factor_{part}"] / j[f"pitch_factor_{part}"] - 1.0) < 2e-2, j
