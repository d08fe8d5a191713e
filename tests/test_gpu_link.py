"""GPU checks of linked channels on the time stretch (TimeStretch(channels_per_group=G), pv_link_channels) against tests/link_model.py and against the
unlinked kernels: G = 1 is the unlinked handle, identical channels give the unlinked output, a group's phases are those of a mono handle fed the mix,
the sum of a group's outputs is the mono stretch of the mix, the inter-channel phase of steady partials is kept, and every call form, chain layout and
hand-over gives the same bits.

Measured values are attached with record_property (visible with --junitxml)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import signals as S
import tones as TN
from link_model import LinkModel, mix, phase_fit, stereo_partials, wrap
from tempo_model import schedule
from test_gpu_stretch_edges import PARITY_BLOCK, PARITY_GLOBAL, _frames, _matrix_signal, _pairs, block_gate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The sum of a group's outputs against the mono GPU handle fed the mix, relative RMS.
DOWNMIX = 1e-6
# Inter-channel phase of fitted steady partials, rad.
PHASE = 5e-8
NS = (256, 512, 1024, 2048, 4096, 8192)
EDGES = ("r1.25", "r0.5", "hsN/2", "haN", "100-97")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _group_signal(kind, N, n, G):
    """G channels that differ: the matrix signal with a per-channel gain, delay and a channel-own noise floor."""
    base = _matrix_signal(kind, N, n + 64 * G)
    return np.stack([(0.3 + 0.7 * (c + 1) / G) * base[17 * c:17 * c + n] + S.lcg_noise(4000 + c, n, 0.02) for c in range(G)]).astype(np.float32)


def _state(ts, ch):
    return [np.asarray(a).copy() for a in ts.export_state(ch)]


def _same_state(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("N", NS)
def test_link_one_is_the_unlinked_handle(N):
    import phaze_amd
    ha, hs = _pairs(N)["r1.25"]
    T = _frames(N, ha, hs)
    x = _group_signal("noise", N, T * ha, 3)
    a = phaze_amd.TimeStretch(N, ha, hs, max_channels=3, max_frames=T)
    b = phaze_amd.TimeStretch(N, ha, hs, max_channels=3, max_frames=T)
    b.link_channels(1)
    assert b.channels_per_group == 1
    ya, yb = a.process(x), b.process(x)
    assert np.array_equal(_bits(ya), _bits(yb))
    for c in range(3):
        assert _same_state(_state(a, c), _state(b, c)), c
    a.close(); b.close()


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("G", [2, 4])
def test_identical_channels_are_the_unlinked_output(N, G):
    """The mix is exactly G x, and atan2, the magnitudes' order and the advance are invariant under a power-of-two scale."""
    import phaze_amd
    ha, hs = _pairs(N)["r1.25"]
    T = _frames(N, ha, hs)
    one = _matrix_signal("partials", N, T * ha)
    ref_ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=1, max_frames=T)
    ref = ref_ts.process(one[None, :])[0]
    ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=G, max_frames=T, channels_per_group=G)
    y = ts.process(np.repeat(one[None, :], G, axis=0))
    for c in range(G):
        assert np.array_equal(_bits(y[c]), _bits(ref)), c
        assert _same_state(_state(ts, c), _state(ref_ts, 0)), c
    ts.close(); ref_ts.close()


# every edge at G = 2, 3, 8, and at one edge the groups that leave the mix's batches of four slots a remainder of 1, 2, 3 and 1 again: 5, 6, 7, 9
GROUP_CASES = [pytest.param(N, name, G, id=f"{G}-{name}-{N}")
               for N, name, G in [(N, name, G) for G in (2, 3, 8) for name in EDGES for N in NS] + [(N, "r1.25", G) for G in (5, 6, 7, 9) for N in NS]]


@pytest.mark.parametrize("N,name,G", GROUP_CASES)
def test_group_phases_model_parity_and_downmix(N, name, G, record_property):
    import phaze_amd
    ha, hs = _pairs(N)[name]
    T = _frames(N, ha, hs)
    x = _group_signal("partials" if G != 3 else "noise", N, T * ha, G)
    ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=G, max_frames=T, channels_per_group=G)
    y = ts.process(x)
    # the group's phases are a mono handle's on the mix, bit for bit, in every slot of the group
    u = mix(x, G)
    mono = phaze_amd.TimeStretch(N, ha, hs, max_channels=1, max_frames=T)
    yu = mono.process(u)[0]
    _, _, phi_u, psi_u = mono.export_state(0)
    for c in range(G):
        _, _, phi, psi = ts.export_state(c)
        assert np.array_equal(phi, phi_u) and np.array_equal(psi, psi_u), c
    # the model, with the mix's doubtful frames out of the block gate
    m = LinkModel(N, ha, hs, G, G, track_doubt=True)
    ref = m.process(x)
    g = _rel(y, ref)
    b = max(block_gate(y[c], ref[c], N, hs, m.doubtful[0])[0] for c in range(G))
    down = _rel(y.astype(np.float64).sum(axis=0), yu)
    for k, v in {"global": g, "block": b, "doubtful": int(np.sum(m.doubtful[0])), "downmix": down}.items():
        record_property(k, v)
    ts.close(); mono.close()
    assert g <= PARITY_GLOBAL, (g, b)
    assert b <= PARITY_BLOCK, (g, b)
    assert down <= DOWNMIX, down


@pytest.mark.parametrize("N,ha,hs", [(1024, 256, 320), (2048, 512, 256), (8192, 1024, 2560)])
def test_inter_channel_phase_of_partials_is_kept(N, ha, hs, record_property):
    import phaze_amd
    lo, _ = TN.steady_range(N, ha, hs, 0)
    T = -(-(lo + 9 * N) // hs)
    f = [round(N * 0.0629) + 0.37, round(N * 0.15) + 0.81]
    amps, ph = [[0.4, 0.15], [0.2, 0.3]], [[0.3, 1.1], [0.3 + np.pi / 2, 1.1 + 2.2]]
    x = stereo_partials(N, f, amps, ph, T * ha)
    dphi = wrap(np.subtract(ph[1], ph[0]))
    out = {}
    for G in (1, 2):
        ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=2, max_frames=T, channels_per_group=G)
        p = phase_fit(ts.process(x), N, ha, hs, f)
        ts.close()
        out[G] = np.abs(wrap(p[1] - p[0] - dphi))
    record_property("linked", float(out[2].max()))
    record_property("unlinked", float(out[1].max()))
    assert out[2].max() <= PHASE, out
    assert out[1].max() > 0.1, out                                     # the unlinked handle does not keep it: the check discriminates


def test_anti_phase_pair_is_silent():
    import phaze_amd
    N, ha, hs, T = 1024, 256, 320, 64
    one = S.make_signal("tonal", 0, T * ha)
    ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=2, max_frames=T, channels_per_group=2)
    y = ts.process(np.stack([one, -one]))
    ts.close()
    assert not np.any(y)


@pytest.mark.parametrize("N,ha,hs", [(256, 64, 80), (2048, 512, 640), (8192, 2048, 4096)])
def test_call_forms_and_chain_layouts_bit_exact(N, ha, hs):
    """One call, pieces of every size (host staging and device calls), one-frame calls, padded strides, a user stream, groups beside groups and an
    export / import hand-over all give the same bits."""
    import phaze_amd
    import torch
    G, nch = 2, 4
    T = max(_frames(N, ha, hs), 48)
    x = np.concatenate([_group_signal("partials", N, T * ha, G), _group_signal("noise", N, T * ha, G)])
    one = phaze_amd.TimeStretch(N, ha, hs, max_channels=nch, max_frames=T, channels_per_group=G)
    ref = one.process(x)
    st_ref = [_state(one, c) for c in range(nch)]
    one.close()
    # the two groups, each on its own handle: groups beside groups do not interact
    for g in range(2):
        h = phaze_amd.TimeStretch(N, ha, hs, max_channels=G, max_frames=T, channels_per_group=G)
        assert np.array_equal(_bits(h.process(x[g * G:(g + 1) * G])), _bits(ref[g * G:(g + 1) * G])), g
        h.close()
    # host pieces (max_frames) and call splits
    for mf, split in ((1, [T]), (5, [3, T - 3]), (T, [1, 7, T - 8])):
        h = phaze_amd.TimeStretch(N, ha, hs, max_channels=nch, max_frames=mf, channels_per_group=G)
        ys, f0 = [], 0
        for n in split:
            ys.append(h.process(x[:, f0 * ha:(f0 + n) * ha]))
            f0 += n
        assert np.array_equal(_bits(np.concatenate(ys, axis=1)), _bits(ref)), (mf, split)
        assert all(_same_state(_state(h, c), st_ref[c]) for c in range(nch)), (mf, split)
        h.close()
    # device pointers with padded strides on a user stream, in two calls
    pad_i, pad_o = T * ha + 37, T * hs + 53
    dx = torch.zeros((nch, pad_i), device="cuda")
    dx[:, :T * ha] = torch.from_numpy(x)
    dy = torch.full((nch, pad_o), 7.0, device="cuda")
    h = phaze_amd.TimeStretch(N, ha, hs, max_channels=nch + 2, max_frames=1, channels_per_group=G)
    s = torch.cuda.Stream()
    h.set_stream(s.cuda_stream)
    k = T // 3
    h.process_device(dx.data_ptr(), dy.data_ptr(), nch, k, pad_i, pad_o)
    h.process_device(dx.data_ptr() + 4 * k * ha, dy.data_ptr() + 4 * k * hs, nch, T - k, pad_i, pad_o)
    h.synchronize()
    yd = dy.cpu().numpy()
    assert np.array_equal(_bits(yd[:, :T * hs]), _bits(ref))
    assert np.all(yd[:, T * hs:] == 7.0)
    for c in (nch, nch + 1):                                           # untouched slots beyond the call
        assert not any(np.any(np.asarray(a).view(np.uint32)) for a in _state(h, c)), c
    h.set_stream(None)
    h.close()
    # export / import hand-over at frame k: the group's phases travel through slot g G
    a = phaze_amd.TimeStretch(N, ha, hs, max_channels=nch, max_frames=T, channels_per_group=G)
    ya = a.process(x[:, :k * ha])
    b = phaze_amd.TimeStretch(N, ha, hs, max_channels=nch, max_frames=T, channels_per_group=G)
    for c in range(nch):
        hist, acc, phi, psi = _state(a, c)
        if c % G == 0:
            b.import_state(c, hist, acc, phi, psi)
        else:
            b.import_state(c, hist, acc)
    yb = b.process(x[:, k * ha:])
    assert np.array_equal(_bits(np.concatenate([ya, yb], axis=1)), _bits(ref))
    assert all(_same_state(_state(b, c), st_ref[c]) for c in range(nch))
    a.close(); b.close()


def test_reset_keeps_the_linking_and_link_resets():
    import phaze_amd
    N, ha, hs, T = 1024, 256, 320, 40
    x = _group_signal("noise", N, T * ha, 2)
    ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=2, max_frames=T, channels_per_group=2)
    y0 = ts.process(x)
    ts.reset()
    assert np.array_equal(_bits(ts.process(x)), _bits(y0))             # still linked after reset
    ts.link_channels(2)                                                # linking resets every slot
    assert all(not np.any(np.asarray(a).view(np.uint32)) for c in range(2) for a in _state(ts, c))
    assert np.array_equal(_bits(ts.process(x)), _bits(y0))
    ts.close()


@pytest.mark.parametrize("N,floor,hs", [(512, 96, 160), (4096, 768, 1280)])
def test_tempo_shared_and_equal_rows_match_the_model(N, floor, hs, record_property):
    import phaze_amd
    G, nch, T = 2, 4, 64
    hops = schedule("random", floor, N, T, seed=N)
    n = int(hops.sum())
    x = np.concatenate([_group_signal("partials", N, n, G), _group_signal("noise", N, n, G)])
    m = LinkModel(N, floor, hs, nch, G, track_doubt=True)
    ref = m.process_hops(x, hops)
    ts = phaze_amd.TimeStretch(N, floor, hs, max_channels=nch, max_frames=T, channels_per_group=G)
    y = ts.process_hops(x, hops)
    g = _rel(y, ref)
    b = max(block_gate(y[c], ref[c], N, hs, m.doubtful[c // G])[0] for c in range(nch))
    record_property("global", g)
    record_property("block", b)
    assert g <= PARITY_GLOBAL and b <= PARITY_BLOCK, (g, b)
    # one row per channel, equal within each group (groups differ): the same as the model with those rows
    rows = np.stack([hops, hops, hops[::-1], hops[::-1]])
    m2 = LinkModel(N, floor, hs, nch, G)
    ref2 = m2.process_hops(x, rows)
    t2 = phaze_amd.TimeStretch(N, floor, hs, max_channels=nch, max_frames=T, channels_per_group=G)
    y2 = t2.process_hops(x, rows)
    assert _rel(y2, ref2) <= PARITY_GLOBAL
    # the shared-row handle and the equal-rows handle agree bit for bit on the first group
    assert np.array_equal(_bits(y2[:G]), _bits(y[:G]))
    ts.close(); t2.close()


def test_rejected_calls_change_nothing():
    import phaze_amd
    from phaze_amd.capi import PV_ERR_ARGUMENT, PvError
    N, ha, hs, T = 512, 128, 160, 16
    x = _group_signal("noise", N, T * N, 4)
    ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=4, max_frames=T, channels_per_group=2)
    ts.process(x[:, :T * ha])
    before = [_state(ts, c) for c in range(4)]
    L, h = ts._L, ts._h
    xo = np.zeros((4, T * hs), np.float32)
    fp = C.POINTER(C.c_float)
    # an odd channel count, through the C entry point (the binding rejects it on the host first)
    assert L.pv_stretch_process(h, x.ctypes.data_as(fp), xo.ctypes.data_as(fp), 3, T, x.shape[1], T * hs) == PV_ERR_ARGUMENT
    assert "linked groups" in L.pv_stretch_last_error(h).decode()
    with pytest.raises(ValueError):
        ts.process(x[:3, :T * ha])
    hops = np.full((4, T), ha, np.int32)
    hops[3, 5] = ha + 1                                                # rows differ within group 1 at frame 5
    with pytest.raises(PvError):
        ts.process_hops(x, hops)
    msg = L.pv_stretch_last_error(h).decode()
    assert "group 1" in msg and "frame 5" in msg, msg
    with pytest.raises(PvError):
        ts.link_channels(0)
    with pytest.raises(PvError):
        ts.link_channels(5)
    assert ts.channels_per_group == 2
    after = [_state(ts, c) for c in range(4)]
    assert all(_same_state(a, b) for a, b in zip(before, after))
    ts.close()


@pytest.mark.parametrize("N,ha,hs", [(256, 64, 128), (8192, 2048, 2560)])
def test_non_finite_input_in_one_channel_recovers(N, ha, hs):
    import phaze_amd
    T, G = 200, 2
    x = _group_signal("tonal", N, T * ha, G)
    s_nan, s_inf = T * ha // 5, 2 * T * ha // 5
    x[1, s_nan] = np.nan
    x[1, s_inf] = np.inf
    ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=G, max_frames=T, channels_per_group=G)
    y = ts.process(x)
    states = [_state(ts, c) for c in range(G)]
    ts.close()
    clean_from = ((s_inf + N - ha) // ha + (N - 1) // hs + 1) * hs
    assert not np.all(np.isfinite(y))
    assert np.all(np.isfinite(y[:, clean_from:]))
    assert all(np.all(np.isfinite(s[0])) and np.all(np.isfinite(s[1])) for s in states)
    ref = LinkModel(N, ha, hs, G, G).process(x)
    assert _rel(y[:, clean_from:], ref[:, clean_from:]) <= 1e-5


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_c_example_runs(tmp_path):
    import phaze_amd
    libdir = os.path.dirname(phaze_amd.library_path())
    exe = str(tmp_path / "pv_link")
    r = subprocess.run(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "pv_link.c"), "-o", exe, "-L", libdir, "-lphaze_amd", "-Wl,-rpath," + libdir,
                        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(ln.split(":", 1) for ln in r.stdout.strip().splitlines() if ":" in ln)
    linked = float(lines["linked offset deg"])
    unlinked = float(lines["unlinked offset deg"])
    assert abs(linked - 90.0) <= 1e-2, r.stdout
    assert abs(unlinked - 90.0) > 5.0, r.stdout
