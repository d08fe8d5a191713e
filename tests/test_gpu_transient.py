"""GPU checks of phase resets and onset strength (pv_transient_process*, pv_onset_strength*, TimeStretch.process_hops(..., resets),
TimeStretch.onset_strength, TimeStretch.process_transients): the call forms that must give the same bits with resets on every kind of chain and
halo boundary, agreement with pv_tempo_process without resets, parity with the model (tests/transient_model.py), psi == phi after a reset, the
identity in a hold, the onset counts against the model, and the chain strength -> onsets -> plan -> process end to end.

Chain boundaries depend on the chip: every position is derived from the handle's own frames per chain and halo (TimeStretch.chain_layout).  The
call forms and the hold identity also run at the edges of the hop axis (HOP_EDGES, transient_model.HOLD_SHAPES); the model parity over that axis is in
tests/test_gpu_stretch_families.py."""
import ctypes as C

import numpy as np
import pytest

import signals as S
import transient_model as TM
from link_model import mix
from tempo_model import positions, schedule
from test_gpu_stretch_edges import PARITY_BLOCK, PARITY_GLOBAL, block_gate

pytestmark = pytest.mark.gpu
SIZES = [256, 512, 1024, 2048, 4096, 8192]
# (N, G, nch): every size unlinked, and groups of 2, 3 and 8
SHAPES = [(N, 1, 2) for N in SIZES] + [(256, 2, 4), (1024, 2, 2), (8192, 2, 2), (512, 3, 3), (2048, 3, 6), (1024, 8, 8), (4096, 8, 8)]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _canary(shape):
    return np.full(shape, np.float32(-1234.5), np.float32)


def _handle(N, f, hs, nch, G, max_frames):
    import phaze_amd
    return phaze_amd.TimeStretch(N, f, hs, max_channels=nch, max_frames=max_frames, channels_per_group=G)


def _whole(n, f):
    """max_frames with which a host call of n input samples per channel is ONE launch (the input staging holds max_frames * floor samples): the
    chains of a call only exist when the call is not cut into pieces first."""
    return -(-n // f)


def _tail(tail, halo):
    """Frames in the last chain: 7 unless asked for "short" (halo // 2: 1 <= r < halo, shorter than the halo the chain after it would need) or
    "one" (a chain of a single frame)."""
    return {"short": max(1, halo // 2), "one": 1}.get(tail, tail)


def _layout(N, f, hs, nch, G, tail=7):
    """(T, F, halo): T = 2 F + r frames that this chip cuts into two chains of F frames and a last one of r = _tail(tail, halo) for a call of nch
    channels."""
    probe = _handle(N, f, hs, nch, G, 1)
    _, halo = probe.chain_layout(nch, 1)
    r = _tail(tail, halo)
    T = 2 * 4 * (halo + 1) + r
    F, _ = probe.chain_layout(nch, T)
    while T != 2 * F + r:
        T = 2 * F + r
        F, _ = probe.chain_layout(nch, T)
    probe.close()
    assert halo == (N - 1) // hs and F >= 4 * (halo + 1) and T == 2 * F + r and 1 <= r < F
    assert tail != "short" or r < halo
    return T, F, halo


def reset_patterns(T, F, halo):
    """name -> flagged frames, from the chip's own chain length F and halo: frame 0; the last frame; the last frame of a chain and the first of the
    next; inside the halo of chains 1 and 2 (one frame, and every frame); two in one chain; every frame; the last frame of the next-to-last chain with
    the last frame of the call (the ONLY frame of the last chain when T = 2 F + 1)."""
    assert halo >= 1
    pats = {"frame0": [0], "last": [T - 1], "chain_edge": [F - 1, F], "halo_one": [F - 1 - (halo - 1) // 2, 2 * F - halo],
            "halo_all": list(range(F - halo, F)) + list(range(2 * F - halo, 2 * F)), "two_in_chain": [F + 1, F + 3], "every": list(range(T)),
            "mixed": [0, F - halo, F, F + 2, 2 * F - 1, T - 1], "tail": [2 * F - 1, T - 1]}
    rows = {}
    for k, v in pats.items():
        r = np.zeros(T, np.uint8)
        r[v] = 1
        rows[k] = r
    return rows


def _states(ts, nch):
    return [ts.export_state(c) for c in range(nch)]


def _same_states(a, b):
    for sa, sb in zip(a, b):
        for u, v in zip(sa, sb):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


# ---- 1. every call form gives the same bits, with resets on every kind of boundary ---------------------------------------------------------------------

# (N, floor, hs) at the edges of the halo = (N - 1) // hs: 255 (the longest), 127 with a floor that divides nothing, 127 at the largest LDS footprint,
# 5 with neither hop a divisor of N, 1 (hs = N / 2: "halo_one" and "halo_all" coincide), floor = 1 (hist is N - 1 long, one-sample hops beside hops
# of N) and floor = N (no carried history)
HOP_EDGES = [(256, 8, 1), (1024, 7, 8), (8192, 1024, 64), (512, 100, 97), (4096, 64, 2048), (2048, 1, 1024), (2048, 2048, 512)]
LONG_HALO = HOP_EDGES[:3]                                             # ... also with a last chain shorter than the halo, and of one frame


# SHAPES at N // 8, 5 N // 16 (halo 3) under the ids they have always had, then HOP_EDGES unlinked and as a group of 2, then LONG_HALO with the other
# last chains
HOP_CASES = [pytest.param(N, G, nch, N // 8, 5 * N // 16, 7, id=f"{N}-{G}-{nch}") for N, G, nch in SHAPES] + \
            [pytest.param(N, G, 2, f, hs, 7, id=f"{N}-{G}-2-{f}-{hs}") for N, f, hs in HOP_EDGES for G in (1, 2)] + \
            [pytest.param(N, G, 2, f, hs, t, id=f"{N}-{G}-2-{f}-{hs}-{t}") for N, f, hs in LONG_HALO for G in (1, 2) for t in ("short", "one")]


@pytest.mark.parametrize("N,G,nch,f,hs,tail", HOP_CASES)
def test_reset_positions_bit_exact_over_call_forms(N, G, nch, f, hs, tail):
    import torch
    T, F, halo = _layout(N, f, hs, nch, G, tail)
    hops = schedule("random", f, N, T, seed=N + G)
    hops[F - halo - 1:F + 2] = max(hs, f)                             # a unit-tempo run across the first chain boundary (hs < floor: a run at the floor)
    P = positions(hops)
    n = int(P[-1])
    x = np.stack([S.make_signal("tonal" if c % 2 == 0 else "noise", c, n) for c in range(nch)])
    ts = _handle(N, f, hs, nch, G, _whole(n, f))                      # one launch, >= 3 chains
    tp = _handle(N, f, hs, nch, G, 5)                                 # host-staged pieces of at most 5 frames
    tb = _handle(N, f, hs, nch, G, _whole(n, f))                      # the hand-over's second handle
    stream = torch.cuda.Stream()
    fp, ip, bp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    rng = np.random.default_rng(N)
    plain = None
    for name, r in reset_patterns(T, F, halo).items():
        ts.reset()
        one = ts.process_hops(x, hops, r)
        st = _states(ts, nch)
        if plain is None:
            ts.reset()
            plain = ts.process_hops(x, hops)
            plain_st = _states(ts, nch)
        # the flags did something: to the output, and where they cannot, to the state the call leaves (at hs = 1 the one output sample a last frame
        # writes itself lies under Hann's zero, so a flag on the last frame alone shows in acc and psi only)
        if hs == 1 and name == "last":
            assert not all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for sa, sb in zip(st, plain_st) for u, v in zip(sa, sb)), name
        else:
            assert not np.array_equal(_bits(one), _bits(plain)), name
        # one frame per call: chains of one frame
        ts.reset()
        fb = np.concatenate([ts.process_hops(x[:, P[m]:P[m + 1]], hops[m:m + 1], r[m:m + 1]) for m in range(T)], axis=1)
        assert np.array_equal(_bits(fb), _bits(one)), name
        _same_states(_states(ts, nch), st)
        # arbitrary splits, some of them right before and right after a flagged frame
        ts.reset()
        flagged = np.nonzero(r)[0]
        cuts = sorted(set([0, T] + rng.integers(1, T, 4).tolist() + [int(flagged[0])] + [int(flagged[-1]) + 1]) - {T + 1})
        cuts = [c for c in cuts if 0 <= c <= T]
        parts = [ts.process_hops(x[:, P[a]:P[b]], hops[a:b], r[a:b]) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(one)), (name, cuts)
        _same_states(_states(ts, nch), st)
        # host-staged pieces
        tp.reset()
        assert np.array_equal(_bits(tp.process_hops(x, hops, r)), _bits(one)), name
        _same_states(_states(tp, nch), st)
        # padded strides, rows per channel with padded row strides, device pointers on a user stream
        si, so, hsd, rsd = n + 37, T * hs + 53, T + 5, T + 3
        xin = _canary((nch, si))
        xin[:, :n] = x
        hp = np.full((nch, hsd), 99999, np.int32)
        hp[:, :T] = hops
        rp = np.full((nch, rsd), 7, np.uint8)
        rp[:, :T] = r
        ts.reset()
        ts.set_stream(stream.cuda_stream)
        d_in = torch.from_numpy(xin).cuda()
        d_out = torch.from_numpy(_canary((nch, so))).cuda()
        torch.cuda.synchronize()
        ts.process_hops_device(d_in.data_ptr(), d_out.data_ptr(), nch, T, hp, si, so, resets=rp)
        ts.synchronize()
        yd = d_out.cpu().numpy()
        ts.set_stream(0)
        assert np.array_equal(_bits(yd[:, :T * hs]), _bits(one)), name
        assert np.all(_bits(yd[:, T * hs:]) == _bits(_canary(1))[0])
        _same_states(_states(ts, nch), st)
        # ... and the same padded layout through host pointers
        ts.reset()
        yout = _canary((nch, so))
        rc = ts._L.pv_transient_process(ts._h, xin.ctypes.data_as(fp), yout.ctypes.data_as(fp), nch, T, hp.ctypes.data_as(ip), hsd, rp.ctypes.data_as(bp),
                                        rsd, si, so)
        assert rc == 0, ts._L.pv_stretch_last_error(ts._h)
        assert np.array_equal(_bits(yout[:, :T * hs]), _bits(one)) and np.all(_bits(yout[:, T * hs:]) == _bits(_canary(1))[0]), name
        # export in mid-schedule (inside the second chain), import on another handle, continue there
        ts.reset()
        k = F + 2
        first = ts.process_hops(x[:, :P[k]], hops[:k], r[:k])
        tb.reset()
        for c, s in enumerate(_states(ts, nch)):
            tb.import_state(c, *s)
        rest = tb.process_hops(x[:, P[k]:], hops[k:], r[k:])
        assert np.array_equal(_bits(np.concatenate([first, rest], axis=1)), _bits(one)), name
        _same_states(_states(tb, nch), st)
    for h in (ts, tp, tb):
        h.close()


@pytest.mark.parametrize("N,G,nch,f,hs,tail", HOP_CASES)
def test_no_flags_is_the_tempo_call(N, G, nch, f, hs, tail):
    """resets = None and all-zero flags (the reset kernels with nothing to do) both give the bits and the state of pv_tempo_process; hops = None
    with flags is the fixed-hop call."""
    T, F, halo = _layout(N, f, hs, nch, G, tail)
    hops = schedule("random", f, N, T, seed=7)
    n = int(hops.sum())
    x = np.stack([S.make_signal("noise" if c % 2 == 0 else "tonal", c, max(n, T * f)) for c in range(nch)])
    ts = _handle(N, f, hs, nch, G, _whole(n, f))
    want = ts.process_hops(x[:, :n], hops)
    st = _states(ts, nch)
    ts.reset()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xc, y = np.ascontiguousarray(x[:, :n]), np.zeros((nch, T * hs), np.float32)
    rc = ts._L.pv_transient_process(ts._h, xc.ctypes.data_as(fp), y.ctypes.data_as(fp), nch, T, hops.astype(np.int32).ctypes.data_as(ip), 0, None, 0, n, T * hs)
    assert rc == 0 and np.array_equal(_bits(y), _bits(want))
    _same_states(_states(ts, nch), st)
    ts.reset()
    assert np.array_equal(_bits(ts.process_hops(x[:, :n], hops, np.zeros(T, np.uint8))), _bits(want))
    _same_states(_states(ts, nch), st)
    # the fixed hop: hops = None
    ts.reset()
    fixed = ts.process(np.ascontiguousarray(x[:, :T * f]))
    ts.reset()
    assert np.array_equal(_bits(ts.process_hops(np.ascontiguousarray(x[:, :T * f]), None, np.zeros(T, np.uint8))), _bits(fixed))
    r = reset_patterns(T, F, halo)["mixed"]
    ts.reset()
    a = ts.process_hops(np.ascontiguousarray(x[:, :T * f]), None, r)
    ts.reset()
    b = ts.process_hops(np.ascontiguousarray(x[:, :T * f]), np.full(T, f), r)
    assert np.array_equal(_bits(a), _bits(b)) and not np.array_equal(_bits(a), _bits(fixed))
    ts.close()


@pytest.mark.parametrize("G", [1, 2, 3])
def test_own_reset_rows_are_independent_handles(G):
    """A row of flags and a row of hops per group (per channel when unlinked) against one fresh handle per group."""
    N, f, hs, groups = 1024, 205, 320, 3
    nch = groups * G
    T, F, halo = _layout(N, f, hs, nch, G)
    pats = reset_patterns(T, F, halo)
    rows = np.repeat(np.stack([schedule("random", f, N, T, seed=g) for g in range(groups)]), G, axis=0)
    early = np.zeros(T, np.uint8)
    early[5] = 1
    flags = np.repeat(np.stack([early, pats["two_in_chain"], pats["halo_one"]]), G, axis=0)       # sparse flags: a wrong row is not reset away
    n = int(rows.sum(axis=1).max())
    x = np.stack([S.make_signal("tonal" if c % 2 == 0 else "noise", c, n) for c in range(nch)])
    ts = _handle(N, f, hs, nch, G, _whole(n, f))
    own = ts.process_hops(x, rows, flags)
    st = _states(ts, nch)
    ts.reset()
    shared_hops = ts.process_hops(x[:, :int(rows[0].sum())], rows[0], flags)
    ts.close()
    for g in range(groups):
        c0 = g * G
        one = _handle(N, f, hs, G, G, _whole(n, f))
        assert np.array_equal(_bits(one.process_hops(x[c0:c0 + G, :int(rows[c0].sum())], rows[c0], flags[c0])), _bits(own[c0:c0 + G])), g
        _same_states(_states(one, G), st[c0:c0 + G])
        if g:                                                          # a shared hop row with a flag row per group
            one.reset()
            assert np.array_equal(_bits(one.process_hops(x[c0:c0 + G, :int(rows[0].sum())], rows[0], flags[c0])), _bits(shared_hops[c0:c0 + G])), g
        one.close()


def test_rejected_transient_calls_change_nothing():
    from phaze_amd import capi
    N, f, hs, nch, G, T = 1024, 205, 320, 4, 2, 6
    ts = _handle(N, f, hs, nch, G, T)
    x = np.stack([S.make_signal("tonal", c, T * f) for c in range(nch)])
    ts.process(x)
    st = _states(ts, nch)
    fp, ip, bp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    y = np.zeros((nch, T * hs), np.float32)
    hops = np.full(T, f, np.int32)

    def call(r, stride):
        return ts._L.pv_transient_process(ts._h, x.ctypes.data_as(fp), y.ctypes.data_as(fp), nch, T, hops.ctypes.data_as(ip), 0, r.ctypes.data_as(bp), stride,
                                          T * f, T * hs)
    two = np.zeros(T, np.uint8)
    two[3] = 2
    assert call(two, 0) == capi.PV_ERR_ARGUMENT and "neither 0 nor 1" in ts._L.pv_stretch_last_error(ts._h).decode()
    assert call(np.zeros((nch, T), np.uint8), T - 1) == capi.PV_ERR_ARGUMENT and "reset_stride" in ts._L.pv_stretch_last_error(ts._h).decode()
    rows = np.zeros((nch, T), np.uint8)
    rows[3, 2] = 1                                                     # differs from its group's first row
    assert call(rows, T) == capi.PV_ERR_ARGUMENT and "reset rows differ within linked group 1" in ts._L.pv_stretch_last_error(ts._h).decode()
    _same_states(_states(ts, nch), st)
    rows[2, 2] = 1
    assert call(rows, T) == capi.PV_OK
    ts.close()


# ---- 2. against the model ------------------------------------------------------------------------------------------------------------------------------

def _parity_inputs(N, G, nch):
    f, hs = N // 8, 5 * N // 16
    halo = (N - 1) // hs
    F0 = 4 * (halo + 1)
    T = 2 * F0 + 9
    hops = schedule("random", f, N, T, seed=N)
    hops[F0 - 2:F0 + 3] = hs
    r = np.zeros(T, np.uint8)
    r[[0, 5, F0 - 2, F0, F0 + 1, 2 * F0 - 1, T - 1]] = 1
    n = int(hops.sum())
    x = np.stack([S.make_signal("tonal" if c % 3 != 1 else "noise", c, n) for c in range(nch)])
    return f, hs, T, hops, r, x


@pytest.mark.parametrize("N,G,nch", SHAPES)
def test_model_parity_with_resets(N, G, nch, record_property):
    """Whole output <= 5e-7 relative RMS, every hs-block <= 4e-6 with the blocks a doubtful frame writes left out; phi exact in >= 99 % of bins; and after
    a call that ends on a flagged frame psi == phi in every bin, bit for bit."""
    f, hs, T, hops, r, x = _parity_inputs(N, G, nch)
    ts = _handle(N, f, hs, nch, G, _whole(x.shape[1], f))                # one launch, >= 3 chains
    y = ts.process_hops(x, hops, r)
    st = _states(ts, nch)
    ts.close()
    m = TM.TransientModel(N, f, hs, nch, G, track_doubt=True)
    ref = m.process_hops(x, hops, r)
    g = _rel(y, ref)
    worst, nd = 0.0, 0
    for c in range(nch):
        b, _ = block_gate(y[c], ref[c], N, hs, m.doubtful[c // G])
        worst = max(worst, b)
    nd = sum(int(np.count_nonzero(d)) for d in m.doubtful)
    for k, v in {"global": g, "block": worst, "doubtful": nd}.items():
        record_property(k, v)
    print(f"N={N} G={G}: global {g:.3e} block {worst:.3e} doubtful {nd}")
    assert g <= PARITY_GLOBAL, (g, worst, nd)
    assert worst <= PARITY_BLOCK, (g, worst, nd)
    assert nd <= 0.01 * T * (nch // G) + 1, nd
    for c in range(nch):
        _, _, phi, psi = st[c]
        assert np.array_equal(phi, psi), c                             # r[T - 1] = 1
        assert np.mean(phi == m.phi[c // G]) >= 0.99


@pytest.mark.parametrize("N,G,nch", [(1024, 1, 1), (1024, 2, 2), (4096, 1, 1), (256, 3, 3)])
def test_psi_is_phi_after_a_reset_and_through_a_unit_tempo_hold(N, G, nch):
    f, hs = N // 8, 5 * N // 16
    x = np.stack([S.make_signal("noise", c, 6 * N) for c in range(nch)])
    ts = _handle(N, f, hs, nch, G, 8)
    ts.process_hops(x[:, :4 * f + 2 * N // 3], [f, f, 2 * N // 3, f, f], None)
    assert not np.array_equal(ts.export_state(0)[2], ts.export_state(0)[3])
    at = 4 * f + 2 * N // 3
    ts.process_hops(x[:, at:at + f], [f], [1])
    for c in range(nch):
        assert np.array_equal(ts.export_state(c)[2], ts.export_state(c)[3]), c
    ts.process_hops(x[:, at + f:at + f + 5 * hs], [hs] * 5, None)       # unit tempo: the advance telescopes exactly, psi stays q
    for c in range(nch):
        assert np.array_equal(ts.export_state(c)[2], ts.export_state(c)[3]), c
    ts.process_hops(x[:, at + f + 5 * hs:at + 2 * f + 5 * hs], [f], None)
    assert not np.array_equal(ts.export_state(0)[2], ts.export_state(0)[3])
    ts.close()


# ---- 3. identity in a hold -----------------------------------------------------------------------------------------------------------------------------

def _hold_case(N, ha, hs, seed):
    J, pre = TM.hold_base(N, ha, hs)
    hops, resets, r = TM.hold_schedule(N, ha, hs, pre, J)
    x = np.random.default_rng(seed).standard_normal(int(hops.sum())).astype(np.float32)
    return hops, resets, r, J, x


@pytest.mark.parametrize("N,ha,hs", TM.HOLD_SHAPES)
def test_hold_identity_gpu(N, ha, hs, record_property):
    """The closed form of the model test, y = g(n) x[n + delta] where only the hold's frames write.  Gate: 4 x the model's value for the same case,
    computed here (the ratio the tone tests use); without the flag the same comparison exceeds 0.5."""
    hops, resets, r, J, x = _hold_case(N, ha, hs, 1)
    floor = min(ha, hs)
    ref = TM.hold_identity(TM.TransientModel(N, floor, hs).process_hops(x[None], hops, resets)[0], x, hops, N, hs, r, J)
    ts = _handle(N, floor, hs, 1, 1, _whole(x.size, floor))
    got = TM.hold_identity(ts.process_hops(x[None], hops, resets)[0], x, hops, N, hs, r, J)
    ts.reset()
    without = TM.hold_identity(ts.process_hops(x[None], hops)[0], x, hops, N, hs, r, J)
    ts.close()
    record_property("gpu", got)
    record_property("model", ref)
    print(f"hold identity N={N} ha={ha} hs={hs}: gpu {got:.3e} model {ref:.3e} without the flag {without:.3f}")
    assert got <= 4 * ref, (got, ref)
    assert without > 0.5, without


@pytest.mark.parametrize("N,ha,hs", TM.HOLD_SHAPES)
def test_hold_identity_linked_pair(N, ha, hs, record_property):
    """A linked pair of independent noises: BOTH channels are their own input in the hold (the mix's angles are zero there)."""
    hops, resets, r, J, x0 = _hold_case(N, ha, hs, 2)
    x = np.stack([x0, np.random.default_rng(3).standard_normal(x0.size).astype(np.float32) * np.float32(0.5)])
    floor = min(ha, hs)
    ref = TM.TransientModel(N, floor, hs, 2, 2).process_hops(x, hops, resets)
    ts = _handle(N, floor, hs, 2, 2, _whole(x.shape[1], floor))
    y = ts.process_hops(x, hops, resets)
    ts.close()
    for c in range(2):
        got, want = TM.hold_identity(y[c], x[c], hops, N, hs, r, J), TM.hold_identity(ref[c], x[c], hops, N, hs, r, J)
        record_property(f"gpu{c}", got)
        print(f"linked hold identity N={N} ha={ha} hs={hs} channel {c}: gpu {got:.3e} model {want:.3e}")
        assert got <= 4 * want, (c, got, want)


# ---- 4. onset strength ---------------------------------------------------------------------------------------------------------------------------------

# the last six: the edges of the hop the header allows (1 .. N): ha = 1, 2 (>= 5000 frames each), 8, ha = N, and a hop that divides nothing
ONSET_SHAPES = [(1024, 256), (2048, 256), (4096, 1024), (256, 100), (8192, 1024), (512, 128), (256, 1), (256, 2), (256, 8), (512, 512), (8192, 8192),
                (1024, 255)]


def _onset_input(N, name):
    n = 40 * N
    return TM.class_signal(name, n, N, [7 * N + 137, 17 * N + 901, 29 * N + 333], seed=3)


@pytest.mark.parametrize("N,ha", ONSET_SHAPES)
def test_onset_strength_against_the_model(N, ha, record_property):
    """|c_gpu - c_model| <= the number of that frame's bins within 2 f32 ulps of either comparison; those allowances sum to <= 1 % of the frames."""
    ts = _handle(N, ha, N // 4, 1, 1, 1)
    tot, frames, off = 0, 0, 0
    for name in sorted(TM.SIGNAL_CLASSES):
        x = _onset_input(N, name)
        c, d = TM.onset_strength(x, N, ha)
        got = ts.onset_strength(x)[0]
        assert got.shape == c.shape
        assert np.all(np.abs(got.astype(np.int64) - c) <= d), (name, np.nonzero(np.abs(got - c) > d)[0][:8])
        tot, frames, off = tot + int(d.sum()), frames + c.size, off + int(np.count_nonzero(got != c))
    ts.close()
    record_property("allowance", tot)
    record_property("frames_off", off)
    print(f"onset strength {N}/{ha}: allowance {tot} bins over {frames} frames, {off} frames differ")
    assert tot <= 0.01 * frames, (tot, frames)


@pytest.mark.parametrize("N,ha,G,nch", [(1024, 256, 2, 4), (512, 128, 3, 3), (2048, 256, 8, 8), (1024, 256, 5, 10), (256, 100, 6, 6), (4096, 1024, 7, 7),
                                        (512, 128, 9, 18)])
def test_onset_strength_of_groups_is_mono_on_the_mix(N, ha, G, nch):
    n = 60 * ha + 17
    x = np.stack([TM.class_signal("bursts_tones", n, N, [5 * N + 11 * c, 9 * N + 300], seed=c) for c in range(nch)])
    x[1] *= np.float32(-0.7)
    ts = _handle(N, ha, N // 4, nch, G, 1)
    got = ts.onset_strength(x)
    st0 = _states(ts, nch)
    ts.close()
    mono = _handle(N, ha, N // 4, nch // G, 1, 1)
    want = mono.onset_strength(mix(x, G))
    mono.close()
    assert got.shape == (nch // G, n // ha) and np.array_equal(got, want)
    for s in st0:                                                      # stateless: a fresh handle's state is still all zeros
        assert all(not np.any(a.view(np.uint32)) for a in s)


@pytest.mark.parametrize("N,ha", [(1024, 256), (256, 100), (4096, 1024)])
def test_onset_strength_in_overlapped_pieces(N, ha):
    """A buffer analysed whole and in pieces that overlap by ceil(N / ha) ha <= N + ha samples: the frames that saw no padding agree exactly."""
    import torch
    x = _onset_input(N, "bursts_noise")
    T = x.size // ha
    ts = _handle(N, ha, N // 4, 1, 1, 1)
    whole = ts.onset_strength(x)[0]
    drop = -(-N // ha)
    got = np.full(T, -1, np.int64)
    step = 37
    for a in range(0, T, step):
        p0 = max(0, a - drop)
        c = ts.onset_strength(x[p0 * ha:min(T, a + step) * ha])[0]
        got[a:a + step] = c[a - p0:]
    assert np.array_equal(got, whole)
    # the device form with a padded counts row
    d_in = torch.from_numpy(x).cuda()
    d_c = torch.full((T + 9,), -5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ts.onset_strength_device(d_in.data_ptr(), 1, T, x.size, d_c.data_ptr(), T + 9)
    ts.synchronize()
    dc = d_c.cpu().numpy()
    assert np.array_equal(dc[:T], whole) and np.all(dc[T:] == -5)
    ts.close()


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------------------------

E2E_N = 1024
E2E_PLANTED = [7 * E2E_N + 137, 17 * E2E_N + 901, 29 * E2E_N + 333]
BURST_LEN = 6 * TM.BURST_DECAY


def _locate_and_spread(res, seg, guess, N):
    """Where the burst `seg` sits in `res` (the lag of the largest |cross-correlation| within 2 N of the guess), and the energy spread of res over
    [lag - N, lag + N + len(seg))."""
    lo, hi = max(0, guess - 2 * N), min(res.size - seg.size, guess + 2 * N)
    cc = np.array([np.dot(res[l:l + seg.size], seg) for l in range(lo, hi)])
    at = lo + int(np.argmax(np.abs(cc)))
    return at, TM.energy_spread(res, max(0, at - N), min(res.size, at + N + seg.size))


@pytest.mark.parametrize("ha,hs,floor", [(256, 384, 192), (256, 192, 160)], ids=["1.5x", "0.75x"])
def test_process_transients_keeps_the_bursts_sharp(ha, hs, floor, record_property):
    """Bursts over tones through process_transients (tau 0.4, lead N / 8, release N / 2) at N = 1024.  Each burst is found in (output - the same schedule's stretch of
    the background alone) by cross-correlation; its energy spread must be within 10 % of the input burst's.  At 1.5x the plain stretch of the same
    input must be above 1.5 x the input's.

    Measured on an MI355X, equal on the model: input spreads 57.8 / 64.4 / 59.1 samples; 1.5x 56.9 / 68.3 / 61.7 (plain stretch 120.4 / 142.5 /
    121.1); 0.75x 57.7 / 64.3 / 59.1.  With release = 0 the planner's hold is two frames long at hs = 384 and 1.5x gave 68.9 / 139.5 / 117.8
    ("End to end")."""
    import phaze_amd
    N, n = E2E_N, 40 * E2E_N
    bg = TM.background("tones", n, N, 3).astype(np.float32)
    bu = TM.bursts(n, E2E_PLANTED, 3)
    x = (bg + bu).astype(np.float32)
    ts = phaze_amd.TimeStretch(N, floor, hs, max_channels=1, max_frames=64)
    y, hops, resets = ts.process_transients(x, hop=ha)
    ts.reset()
    yb = ts.process_hops(bg[None, :int(hops.sum())], hops, resets)
    ts.close()
    assert int(resets.sum()) == 1 + len(E2E_PLANTED)                  # the start of the buffer and the three bursts
    res = (y[0].astype(np.float64) - yb[0])
    Sp = positions(hops)
    T0 = n // ha
    pl = phaze_amd.TimeStretch(N, ha, hs, max_channels=2, max_frames=64)
    yp = pl.process(np.stack([x[:T0 * ha], bg[:T0 * ha]]))
    pl.close()
    resp = yp[0].astype(np.float64) - yp[1]
    fails = []
    for o in E2E_PLANTED:
        seg = bu[o:o + BURST_LEN]
        s_in = TM.energy_spread(bu, o - N, o + N + BURST_LEN)
        _, s_out = _locate_and_spread(res, seg, int(np.searchsorted(Sp, o)) * hs, N)
        _, s_plain = _locate_and_spread(resp, seg, o * hs // ha + N - hs, N)
        record_property(f"burst{o}", (s_in, s_out, s_plain))
        print(f"{hs}/{ha} burst at {o}: spread in {s_in:.1f}, process_transients {s_out:.1f}, plain stretch {s_plain:.1f}")
        if abs(s_out - s_in) > 0.1 * s_in:
            fails.append((o, s_in, s_out))
        if hs > ha:
            assert s_plain > 1.5 * s_in, (o, s_in, s_plain)
    assert not fails, fails
