"""GPU checks of variable tempo (pv_tempo_process / pv_tempo_process_device, TimeStretch.process_hops): agreement with the fixed-hop path bit for
bit, parity with the model (tests/tempo_model.py) at every N, the closed form of stationary tones under schedules, the call forms and layouts that
must give the same bits, argument errors, and the C99 example.

Every schedule here differs from its handle's floor somewhere, so each test runs the schedule kernels and not only the fixed-hop ones."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import signals as S
import tones as TN
from stretch_model import StretchModel
from tempo_model import TONE_SHAPES, TempoModel, schedule, tone_schedule_input
from test_gpu_stretch_edges import GPU_TOL, PARITY_BLOCK, PARITY_GLOBAL, block_gate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SIZES = [256, 512, 1024, 2048, 4096, 8192]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _halo(N, hs):
    return (N - 1) // hs


def _F0(N, hs):
    """The fewest frames a chain holds: with T <= (resident slots) F0 frames a call runs ceil(T / F0) chains."""
    return 4 * (_halo(N, hs) + 1)


def _same_state(a, b, N, ca=0, cb=0):
    """Two handles' slots hold the same acc / phi / psi bits, and the newest samples of history the shorter hist holds."""
    ha, aa, pa, sa = a.export_state(ca)
    hb, ab, pb, sb = b.export_state(cb)
    n = min(ha.size, hb.size)
    assert np.array_equal(_bits(aa), _bits(ab)) and np.array_equal(pa, pb) and np.array_equal(sa, sb)
    assert np.array_equal(_bits(ha[ha.size - n:]), _bits(hb[hb.size - n:]))


# ---- 1. agreement with the fixed-hop path, bit for bit -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", SIZES)
def test_constant_schedule_is_the_fixed_handle(N):
    """hops all c on a handle with floor f < c: the bits of a handle created with analysis_hop = c (pv_stretch_process), over >= 3 chains."""
    import phaze_amd
    f, c, hs = N // 8, N // 4 + 3, 5 * N // 16
    T = 2 * _F0(N, hs) + 1
    x = S.make_signal("tonal", 1, T * c)[None, :]
    a = phaze_amd.TimeStretch(N, f, hs, max_channels=1, max_frames=T)
    b = phaze_amd.TimeStretch(N, c, hs, max_channels=1, max_frames=T)
    ya = a.process_hops(x, np.full(T, c))
    yb = b.process(x)
    assert np.array_equal(_bits(ya), _bits(yb))
    _same_state(a, b, N)
    a.close()
    b.close()


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("order", ["up", "down"])
def test_step_schedule_is_chained_fixed_handles(N, order):
    """c1 for T1 frames then c2 for T2, in one call over >= 3 chains with the step inside a chain, against a handle with analysis_hop = c1 whose
    exported state a handle with analysis_hop = c2 imports (hist rebuilt from the stream: it needs more history than the first one keeps when c2 < c1)."""
    import phaze_amd
    hs = 5 * N // 16
    lo, hi = N // 8 + 1, N // 2 + 5
    c1, c2 = (lo, hi) if order == "up" else (hi, lo)
    f = N // 8
    F0 = _F0(N, hs)
    T1, T2 = F0 + 5, F0 + 7
    x = S.make_signal("noise", 2, T1 * c1 + T2 * c2)
    t = phaze_amd.TimeStretch(N, f, hs, max_channels=1, max_frames=T1 + T2)
    y = t.process_hops(x[None, :], np.array([c1] * T1 + [c2] * T2))
    a = phaze_amd.TimeStretch(N, c1, hs, max_channels=1, max_frames=T1)
    ya = a.process(x[None, :T1 * c1])
    _, acc, phi, psi = a.export_state(0)
    stream = np.concatenate([np.zeros(N, np.float32), x])
    b = phaze_amd.TimeStretch(N, c2, hs, max_channels=1, max_frames=T2)
    b.import_state(0, stream[N + T1 * c1 - (N - c2):N + T1 * c1], acc, phi, psi)
    yb = b.process(x[None, T1 * c1:])
    assert np.array_equal(_bits(y), _bits(np.concatenate([ya, yb], axis=1)))
    _same_state(t, b, N)
    for h in (t, a, b):
        h.close()


# ---- 2. parity with the model ---------------------------------------------------------------------------------------------------------------------------

def _parity(y, ref, model, N, hs, record_property):
    g = _rel(y, ref)
    worst, nd = 0.0, 0
    for c in range(y.shape[0]):
        b, d = block_gate(y[c], ref[c], N, hs, model.doubtful[c])
        worst, nd = max(worst, b), nd + d
    for k, v in {"global": g, "block": worst, "doubtful": nd}.items():
        record_property(k, v)
    assert g <= PARITY_GLOBAL, (g, worst, nd)
    assert worst <= PARITY_BLOCK, (g, worst, nd)
    assert nd <= 0.01 * y.size / hs + y.shape[0], nd


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", ["ramp", "random", "alt"])
def test_model_parity_mono(N, kind, record_property):
    """One channel over >= 3 chains: a ramp floor -> N, uniform random hops, and floor / N in turn."""
    import phaze_amd
    hs = 5 * N // 16
    f = N // 8
    T = 2 * _F0(N, hs) + 9
    hops = schedule(kind, f, N, T, seed=N)
    x = (S.make_signal("tonal", 0, int(hops.sum())) if kind != "random" else S.make_signal("noise", 0, int(hops.sum())))[None, :]
    ts = phaze_amd.TimeStretch(N, f, hs, max_channels=1, max_frames=T)
    y = ts.process_hops(x, hops)
    m = TempoModel(N, f, hs, track_doubt=True)
    ref = m.process_hops(x, hops)
    _, acc, phi, psi = ts.export_state(0)
    ts.close()
    _parity(y, ref, m, N, hs, record_property)
    assert np.mean(phi == m.phi[0]) >= 0.99


@pytest.mark.parametrize("N", SIZES)
def test_model_parity_eight_channels_own_rows(N, record_property):
    """Eight channels, each with its own row (ramps up and down, random, alternating extremes) and so its own input total, in one call."""
    import phaze_amd
    hs = N // 4
    f = N // 8
    T = 2 * _F0(N, hs) + 3
    kinds = ["ramp", "random", "alt", "random", "ramp", "random", "alt", "random"]
    rows = np.stack([schedule(k, f, N, T, seed=10 * N + c) for c, k in enumerate(kinds)])
    rows[4] = rows[4][::-1]
    n = int(rows.sum(axis=1).max())
    x = np.stack([S.make_signal("tonal" if c % 2 == 0 else "noise", c, n) for c in range(8)])
    ts = phaze_amd.TimeStretch(N, f, hs, max_channels=8, max_frames=T)
    y = ts.process_hops(x, rows)
    ts.close()
    m = TempoModel(N, f, hs, nch=8, track_doubt=True)
    ref = m.process_hops(x, rows)
    _parity(y, ref, m, N, hs, record_property)


@pytest.mark.parametrize("kind", ["ramp", "random", "alt"])
@pytest.mark.parametrize("sid", list(TONE_SHAPES))
def test_tones_closed_form_under_schedules_gpu(sid, kind, record_property):
    import phaze_amd
    N, floor, hs, freqs, amps = TONE_SHAPES[sid]
    hops, x = tone_schedule_input(N, floor, hs, freqs, amps, kind)
    ts = phaze_amd.TimeStretch(N, floor, hs, max_channels=1, max_frames=hops.size)
    y = ts.process_hops(x[None, :], hops)[0]
    ts.close()
    ratio, res = TN.tone_fit(y, N, floor, hs, freqs, amps)
    err = max(float(np.max(np.abs(ratio - 1.0))), res)
    record_property("tone_err", err)
    assert err <= GPU_TOL, (ratio, res)


# ---- 3. call forms and layouts, bit for bit ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,f,hs", [(1024, 205, 320), (256, 32, 80), (8192, 1024, 2048)])
def test_call_forms_bit_exact(N, f, hs):
    import phaze_amd
    import torch
    F0 = _F0(N, hs)
    T = 2 * F0 + 7                                                   # >= 3 chains
    hops = schedule("random", f, N, T, seed=3)
    hops[F0 - 2:F0 + 4] = f                                          # a run at the floor: pv_stretch_process can take it
    hops[-3:] = f
    P = np.concatenate([[0], np.cumsum(hops)])
    x = S.make_signal("tonal", 0, int(P[-1]))[None, :]
    ts = phaze_amd.TimeStretch(N, f, hs, max_channels=1, max_frames=T)
    one = ts.process_hops(x, hops)
    # one frame per call
    ts.reset()
    fb = np.concatenate([ts.process_hops(x[:, P[m]:P[m + 1]], hops[m:m + 1]) for m in range(T)], axis=1)
    assert np.array_equal(_bits(fb), _bits(one))
    # irregular splits, the floor runs through pv_stretch_process
    ts.reset()
    cuts = [0, 1, F0 - 2, F0 + 4, F0 + 9, T - 3, T]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if np.all(hops[a:b] == f):
            parts.append(ts.process(x[:, P[a]:P[b]]))
        else:
            parts.append(ts.process_hops(x[:, P[a]:P[b]], hops[a:b]))
    assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(one))
    # device pointers
    ts.reset()
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.empty((1, T * hs), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ts.process_hops_device(d_in.data_ptr(), d_out.data_ptr(), 1, T, hops, int(P[-1]), T * hs)
    ts.synchronize()
    assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(one))
    # two device calls before any synchronise: the second upload of the table does not disturb the first call
    ts.reset()
    h = T // 2 + 1
    d_out.fill_(0.0)
    torch.cuda.synchronize()
    ts.process_hops_device(d_in.data_ptr(), d_out.data_ptr(), 1, h, hops[:h], int(P[h]), h * hs)
    ts.process_hops_device(d_in.data_ptr() + 4 * int(P[h]), d_out.data_ptr() + 4 * h * hs, 1, T - h, hops[h:], int(P[-1] - P[h]), (T - h) * hs)
    ts.synchronize()
    assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(one))
    ts.close()
    # staged pieces: max_frames = 1, and max_frames * floor < N (the input staging grows once to one frame of hop N)
    for mf in (1, 2, F0 - 1):
        tp = phaze_amd.TimeStretch(N, f, hs, max_channels=1, max_frames=mf)
        assert np.array_equal(_bits(tp.process_hops(x, hops)), _bits(one)), mf
        tp.close()


def _canary(shape):
    return np.full(shape, np.float32(-1234.5), np.float32)


def test_rows_slots_strides_and_handover():
    import phaze_amd
    import torch
    N, f, hs, nch, maxch = 1024, 205, 320, 3, 6
    T = 2 * _F0(N, hs) + 5
    H = N // 2 + 1
    shared = schedule("ramp", f, N, T)
    rows = np.stack([schedule("random", f, N, T, seed=c) for c in range(nch)])
    n = int(rows.sum(axis=1).max())
    x = np.stack([S.make_signal("tonal" if c % 2 == 0 else "noise", c, max(n, int(shared.sum()))) for c in range(nch)])
    xs = np.ascontiguousarray(x[:, :int(shared.sum())])
    ts = phaze_amd.TimeStretch(N, f, hs, max_channels=maxch, max_frames=9)
    rng = np.random.default_rng(5)
    slots = {}
    for c in range(nch, maxch):                                       # slots nch .. maxch - 1 hold an imported state no call may touch
        st = ((rng.standard_normal(N - f)).astype(np.float32), (rng.standard_normal(N - hs)).astype(np.float32),
              rng.integers(0, 2 ** 32, H, dtype=np.uint64).astype(np.uint32), rng.integers(0, 2 ** 32, H, dtype=np.uint64).astype(np.uint32))
        ts.import_state(c, *st)
        slots[c] = st

    def untouched():
        for c, st in slots.items():
            for a, b in zip(ts.export_state(c), st):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), c

    def fresh():
        ts.reset()
        for c, st in slots.items():
            ts.import_state(c, *st)

    # a shared row against the same row given to every channel
    fresh()
    y_shared = ts.process_hops(xs, shared)
    untouched()
    fresh()
    y_rows = ts.process_hops(xs, np.stack([shared] * nch))
    assert np.array_equal(_bits(y_rows), _bits(y_shared))
    # own rows against one fresh handle per channel
    fresh()
    own = ts.process_hops(x, rows)
    untouched()
    for c in range(nch):
        one = phaze_amd.TimeStretch(N, f, hs, max_channels=1, max_frames=T)
        assert np.array_equal(_bits(one.process_hops(x[c, :int(rows[c].sum())], rows[c])[0]), _bits(own[c])), c
        one.close()
    # padded strides through the C ABI (host pointers), rows with a padded hop_stride: the padding keeps its canary
    si, so, hsd = n + 37, T * hs + 53, T + 5
    xin = _canary((nch, si))
    xin[:, :n] = x[:, :n]
    yout = _canary((nch, so))
    hp = np.full((nch, hsd), 99999, np.int32)
    hp[:, :T] = rows
    fresh()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rc = ts._L.pv_tempo_process(ts._h, xin.ctypes.data_as(fp), yout.ctypes.data_as(fp), nch, T, hp.ctypes.data_as(ip), hsd, si, so)
    assert rc == 0, ts._L.pv_stretch_last_error(ts._h)
    assert np.array_equal(_bits(yout[:, :T * hs]), _bits(own))
    assert np.all(_bits(yout[:, T * hs:]) == _bits(_canary(1))[0])
    untouched()
    # ... and through device pointers, on a user stream
    s = torch.cuda.Stream()
    fresh()
    ts.set_stream(s.cuda_stream)
    d_in = torch.from_numpy(xin).cuda()
    d_out = torch.from_numpy(_canary((nch, so))).cuda()
    torch.cuda.synchronize()
    ts.process_hops_device(d_in.data_ptr(), d_out.data_ptr(), nch, T, hp, si, so)
    ts.synchronize()
    yd = d_out.cpu().numpy()
    assert np.array_equal(_bits(yd[:, :T * hs]), _bits(own))
    assert np.all(_bits(yd[:, T * hs:]) == _bits(_canary(1))[0])
    untouched()
    ts.set_stream(0)
    # export in mid-schedule, import on another slot, continue there
    fresh()
    k = T // 2 - 3
    P = np.concatenate([np.zeros((nch, 1), np.int64), np.cumsum(rows, axis=1)], axis=1)
    first = ts.process_hops(x[:1, :int(P[0, k])], rows[0, :k])
    st = ts.export_state(0)
    tb = phaze_amd.TimeStretch(N, f, hs, max_channels=4, max_frames=T)
    tb.import_state(2, *st)
    x3 = np.zeros((3, int(P[0, T] - P[0, k])), np.float32)
    x3[2] = x[0, int(P[0, k]):int(P[0, T])]
    r3 = np.stack([rows[0, k:]] * 3)
    rest = tb.process_hops(x3, r3)[2:3]
    assert np.array_equal(_bits(np.concatenate([first, rest], axis=1)), _bits(own[:1]))
    tb.close()
    ts.close()


# ---- 4. errors ----------------------------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_change_nothing():
    import phaze_amd
    import torch
    N, f, hs, nch = 1024, 205, 320, 2
    T = 40
    hops = schedule("random", f, N, T, seed=9).astype(np.int32)
    n = int(hops.sum())
    x = np.stack([S.make_signal("tonal", c, n) for c in range(nch)])
    ref_h = phaze_amd.TimeStretch(N, f, hs, max_channels=nch, max_frames=T)
    ref = np.concatenate([ref_h.process_hops(x[:, :int(hops[:20].sum())], hops[:20]), ref_h.process_hops(x[:, int(hops[:20].sum()):], hops[20:])], axis=1)
    ref_h.close()
    ts = phaze_amd.TimeStretch(N, f, hs, max_channels=nch, max_frames=T)
    y1 = ts.process_hops(x[:, :int(hops[:20].sum())], hops[:20])
    L, h = ts._L, ts._h
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xin = np.ascontiguousarray(x[:, int(hops[:20].sum()):])
    rest = hops[20:].copy()
    m = rest.size
    yout = np.zeros((nch, m * hs), np.float32)
    tot = int(rest.sum())

    def call(hp, stride=0, nchan=nch, nfr=m, si=tot, so=m * hs, xi=xin, yo=yout):
        return L.pv_tempo_process(h, xi.ctypes.data_as(fp) if xi is not None else None, yo.ctypes.data_as(fp) if yo is not None else None, nchan, nfr,
                                  hp.ctypes.data_as(ip) if hp is not None else None, stride, si, so)

    bad_lo, bad_hi = rest.copy(), np.tile(rest, (nch, 1))
    bad_lo[7] = f - 1
    bad_hi[1, 11] = N + 1
    cases = [
        (lambda: call(rest, xi=None), phaze_amd.capi.PV_ERR_ARGUMENT, "null buffer"),
        (lambda: call(None), phaze_amd.capi.PV_ERR_ARGUMENT, "null hops"),
        (lambda: call(rest, nfr=-1), phaze_amd.capi.PV_ERR_ARGUMENT, "negative"),
        (lambda: call(rest, nchan=3), phaze_amd.capi.PV_ERR_CAPACITY, "max_channels"),
        (lambda: call(np.tile(rest, (nch, 1)), stride=m - 1), phaze_amd.capi.PV_ERR_ARGUMENT, "hop_stride"),
        (lambda: call(bad_lo), phaze_amd.capi.PV_ERR_ARGUMENT, "channel 0, frame 7"),
        (lambda: call(bad_hi, stride=m), phaze_amd.capi.PV_ERR_ARGUMENT, "channel 1, frame 11"),
        (lambda: call(rest, si=tot - 1), phaze_amd.capi.PV_ERR_ARGUMENT, "strides"),
        (lambda: call(rest, so=m * hs - 1), phaze_amd.capi.PV_ERR_ARGUMENT, "strides"),
    ]
    for fn, code, text in cases:
        assert fn() == code, text
        assert text in L.pv_stretch_last_error(h).decode(), (text, L.pv_stretch_last_error(h).decode())
    # the device form validates the same way before any device work
    d = torch.zeros(16, device="cuda")
    assert L.pv_tempo_process_device(h, C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), 1, 2, bad_lo[6:8].ctypes.data_as(ip), 0, 16, 16) == \
        phaze_amd.capi.PV_ERR_ARGUMENT
    assert "channel 0, frame 1" in L.pv_stretch_last_error(h).decode()
    with pytest.raises(ValueError):
        ts.process_hops(xin[:, :-1], rest)                            # the binding checks the input length of a shared row
    # ... and the next valid call continues as if none of them had been made
    assert call(rest) == 0
    assert np.array_equal(_bits(np.concatenate([y1, yout], axis=1)), _bits(ref))
    ts.close()


def test_device_form_has_read_the_schedule_when_it_returns():
    import phaze_amd
    import torch
    N, f, hs = 1024, 205, 320
    T = 2 * _F0(N, hs) + 5
    hops = schedule("alt", f, N, T).astype(np.int32)
    x = S.make_signal("noise", 4, int(hops.sum()))[None, :]
    ref = phaze_amd.TimeStretch(N, f, hs, max_channels=1, max_frames=T).process_hops(x, hops)
    ts = phaze_amd.TimeStretch(N, f, hs, max_channels=1, max_frames=T)
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.empty((1, T * hs), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    buf = np.ascontiguousarray(hops)
    rc = ts._L.pv_tempo_process_device(ts._h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), 1, T, buf.ctypes.data_as(C.POINTER(C.c_int32)),
                                       0, int(hops.sum()), T * hs)
    assert rc == 0
    buf[:] = f                                                        # overwritten before the launch can have run
    ts.synchronize()
    assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(ref))
    ts.close()


# ---- 5. the C example -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
@pytest.mark.parametrize("args", [[], ["256", "80", "20", "256", "150"], ["8192", "2048", "1024", "8192", "60"]])
def test_c_example_ramp_equals_frame_by_frame(tmp_path, args):
    from test_tempo_abi import _build
    exe = _build(tmp_path)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["ramp_equals_frame_by_frame"] is True and j["output_rms"] > 1e-3 and j["min_hop"] < j["max_hop"]
