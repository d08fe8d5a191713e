"""PitchStretch (pv_pitch_*) on the GPU: the handle is a TimeStretch followed by a Resampler, bit for bit and state for state, in every call form; tones
through it fit the closed form of tests/test_resample_model.py; a linked pair keeps its inter-channel phase; the output length is J of the stretched
length.  The stretch stage is compared GPU against GPU and the resampler has no decisions, so no frame needs to be set aside as doubtful."""
import numpy as np
import pytest

import resample_model as RM
import test_resample_model as TRM
import tones
from link_model import stereo_partials, wrap
from test_gpu_link import PHASE

pytestmark = pytest.mark.gpu

FRAMES = 61
# (N, floor hop, synthesis hop): the resampler runs at up / down = floor / hs.  Which instance of it that is follows pv_resample_create's rule (tests/test_gpu_resample.py)
SHAPES = [
    (1024, 205, 320),                # 41/64: the taps-in-LDS instance
    (1024, 251, 256),                # 251/256: generic, L <= 256 but the table does not fit beside the span
    (1024, 64, 500),                 # 16/125: generic at decimation, pitch x 7.8
    (512, 257, 40),                  # 257/40: generic, L above the thread count, pitch x 0.156 (pv_stretch_create accepts the pair: ha <= N, hs <= N / 2, 1/8 <= ha / hs <= 8)
]


def _input(N, nch, n, seed):
    rng = np.random.default_rng(seed)
    k = np.arange(n, dtype=np.float64)
    x = np.stack([0.4 * np.cos(2 * np.pi * (60.3 + 11 * c) * k / N + c) + 0.2 * np.cos(2 * np.pi * 171.7 * k / N) + 0.05 * rng.standard_normal(n)
                  for c in range(nch)])
    x[:, n // 2:n // 2 + 40] += 0.8 * rng.standard_normal((nch, 40))             # an attack for the resets to carry
    return x.astype(np.float32)


def _schedule(kind, rng, N, FLOOR, HS):
    """Hops scale with the shape: from the floor to 400 / 205 of it (at most N), six frames in the middle at unit tempo where the handle allows hop == hs."""
    if kind == "fixed":
        return None, None
    hops = rng.integers(FLOOR, min(FLOOR * 400 // 205, N + 1), FRAMES).astype(np.int32)
    hops[FRAMES // 2:FRAMES // 2 + 6] = HS if FLOOR <= HS <= N else FLOOR
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
@pytest.mark.parametrize("kind", ["fixed", "hops", "resets"])
@pytest.mark.parametrize("N,FLOOR,HS", SHAPES)
def test_pitch_handle_is_stretch_then_resample_bit_for_bit(N, FLOOR, HS, G, kind):
    import phaze_amd
    import torch
    nch = 2
    rng = np.random.default_rng(17 + G)
    hops, resets = _schedule(kind, rng, N, FLOOR, HS)
    row = np.full(FRAMES, FLOOR, np.int32) if hops is None else hops
    at = np.concatenate([[0], np.cumsum(row.astype(np.int64))])
    x = _input(N, nch, int(at[-1]), 5)
    L, M = RM.reduce_ratio(FLOOR, HS)

    ts = phaze_amd.TimeStretch(N, FLOOR, HS, max_channels=nch, max_frames=FRAMES, channels_per_group=G)
    rs = phaze_amd.Resampler(FLOOR, HS, max_channels=nch, max_samples=FRAMES * HS)
    mid = ts.process_hops(x, hops, resets)
    want = rs.process(mid)
    assert want.shape[1] == RM.count(FLOOR, HS, FRAMES * HS) > 3 * 1024          # the output length is J of the stretched length
    want_state = _states(ts, rs, nch)

    def same(p, y, what):
        assert y.shape == want.shape and np.array_equal(y.view(np.uint32), want.view(np.uint32)), what
        got = _states(p.stretch, p.resampler, nch)
        assert len(got) == len(want_state) and all(np.array_equal(a, b) for a, b in zip(got, want_state)), what

    for cuts in ([FRAMES], [1, 7, FRAMES - 8], [20, 0, 2, 39], [3] * 20 + [1]):
        p = phaze_amd.PitchStretch(N, FLOOR, HS, max_channels=nch, max_frames=4, channels_per_group=G)
        assert (p.resampler.up, p.resampler.down) == (L, M)
        parts, f0 = [], 0
        for nf in cuts:
            if nf == 0:
                continue
            n_expected = p.resampler.out_count(nf * HS)
            y = p.process_hops(x[:, at[f0]:at[f0 + nf]], None if hops is None else hops[f0:f0 + nf], None if resets is None else resets[f0:f0 + nf])
            assert y.shape[1] == n_expected
            parts.append(y)
            f0 += nf
        assert f0 == FRAMES
        same(p, np.concatenate(parts, axis=1), cuts)
        p.close()

    # the device form on a user stream, two calls, padded strides
    p = phaze_amd.PitchStretch(N, FLOOR, HS, max_channels=nch, max_frames=1, channels_per_group=G)
    stream = torch.cuda.Stream()
    p.set_stream(stream.cuda_stream)
    d_in = torch.zeros((nch, x.shape[1] + 3), dtype=torch.float32, device="cuda")
    d_in[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    d_out = torch.full((nch, want.shape[1] + 9), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    done, f0 = 0, 0
    for nf in (25, FRAMES - 25):
        done += p.process_device(d_in.data_ptr() + 4 * int(at[f0]), d_out.data_ptr() + 4 * done, nch, nf, x.shape[1] + 3, want.shape[1] + 9,
                                 want.shape[1] - done, None if hops is None else hops[f0:f0 + nf], None if resets is None else resets[f0:f0 + nf])
        f0 += nf
    p.synchronize()
    yd = d_out.cpu().numpy()
    assert done == want.shape[1] and np.all(yd[:, done:] == -77.0)
    same(p, np.ascontiguousarray(yd[:, :done]), "device form")
    # a short out_capacity is refused with both states untouched
    with pytest.raises(phaze_amd.PvError) as e:
        p.process_device(d_in.data_ptr(), d_out.data_ptr(), nch, 4, x.shape[1] + 3, want.shape[1] + 9, p.resampler.out_count(4 * HS) - 1)
    assert e.value.status == phaze_amd.capi.PV_ERR_ARGUMENT and "out_capacity" in str(e.value)
    p.synchronize()
    same(p, np.ascontiguousarray(yd[:, :done]), "after a refused call")
    p.set_stream(None)
    p.close()
    ts.close()
    rs.close()


@pytest.mark.parametrize("name", TRM.PITCH_CASES)
def test_tones_through_the_pitch_handle_fit_the_closed_form(name):
    """Gate: 4 x the model's own figures (tests/test_resample_model.py PITCH_MEASURED), the project's practice for closed forms."""
    import phaze_amd
    n, ha, hs, freqs, amps = tones.CASES[name]
    T, x = tones.case_input(n, ha, hs, freqs, amps)
    p = phaze_amd.PitchStretch(n, ha, hs, max_frames=T)
    y = p.process(x[None, :])[0]
    assert y.size == RM.count(ha, hs, T * hs)                                    # the output length is J of the stretched length
    ratio, res = TRM.pitch_fit(y, T * hs, n, ha, hs, p.resampler.up, p.resampler.down, freqs, amps)
    amp_gate, res_gate = (4 * v for v in TRM.PITCH_MEASURED[name])
    print(f"gpu pitch {name}: amplitude ratio - 1 {ratio - 1}, residual {res:.3e} (gates {amp_gate:.1e}, {res_gate:.1e})")
    assert np.max(np.abs(ratio - 1.0)) <= amp_gate and res <= res_gate, (ratio, res)
    p.close()


def test_a_linked_pair_keeps_its_inter_channel_phase_through_the_pitch_handle():
    import phaze_amd
    n, ha, hs = 1024, 256, 320
    lo, _ = tones.steady_range(n, ha, hs, 0)
    T = -(-(lo + 9 * n) // hs)
    f = [round(n * 0.0629) + 0.37, round(n * 0.15) + 0.81]
    amps, ph = [[0.4, 0.15], [0.2, 0.3]], [[0.3, 1.1], [0.3 + np.pi / 2, 1.1 + 2.2]]
    x = stereo_partials(n, f, amps, ph, T * ha)
    dphi = wrap(np.subtract(ph[1], ph[0]))
    out = {}
    for G in (1, 2):
        p = phaze_amd.PitchStretch(n, ha, hs, max_channels=2, max_frames=T, channels_per_group=G)
        fit = TRM.pitch_phase_fit(p.process(x), T * hs, n, ha, hs, p.resampler.up, p.resampler.down, f)
        p.close()
        out[G] = np.abs(wrap(fit[1] - fit[0] - dphi))
    print(f"inter-channel phase through the pitch handle: linked {out[2].max():.3e} rad, unlinked {out[1].max():.3e} rad (gate {PHASE:.1e})")
    assert out[2].max() <= PHASE, out
    assert out[1].max() > 0.1, out                                     # the unlinked handle does not keep it: the check discriminates
