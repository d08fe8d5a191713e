"""The resampler kernels (Resampler / pv_resample_*) on the GPU against the numpy model (tests/resample_model.py), split invariance, counts and closed forms.

Tolerance against the model, DERIVED: the model sums exact products in fp64 on the library's own exported taps and the same f32 input; the kernel adds T
fused multiply-adds into one f32 accumulator, each rounding once a partial sum bounded by sum_i |h_i x_i|, and the model's own fp64 rounding is far
inside one more unit: per sample |y_gpu - y_model| <= (T + 1) 2^-24 sum_i |h_i x_i|, the sum computed by the model for that very sample.  No sample is
left out.  Split invariance is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import resample_model as RM
import test_resample_model as TRM

pytestmark = pytest.mark.gpu

# Which instance a ratio takes is pv_resample_create's rule (L <= 256 threads AND the tap table fits beside the tile's span in 64 KB of LDS: the taps-in-LDS
# instance pv_resample_kernel<true>, else the generic pv_resample_kernel<false>).  No entry point reports it, so it is stated here, worked out from that rule:
GENERIC_RATIOS = [
    (16, 125),                       # generic: the smallest L whose table does not fit (decimation 7.8: T = 500 taps, span 8493)
    (16, 123),                       # shared:  its neighbour on the other side of the LDS budget
    (100, 227), (100, 223),          # generic, shared: the same boundary at a mid-size L
    (239, 240),                      # generic: near unity, L <= 256, table too large
    (232, 233),                      # shared:  the largest such L that still fits
    (257, 256),                      # generic: the smallest L above the thread count
    (1024, 8191), (1025, 8192),      # generic at / 8: T = 512, span about 8690, stride-8 LDS reads
    (8191, 1024), (8192, 1025),      # generic at x 8
]
RATIOS = [(4, 5), (5, 4), (2, 3), (3, 2), (1, 2), (2, 1), (1, 8), (8, 1), (100, 97), (97, 100), (147, 160), (160, 147), (8191, 8192), (8192, 8191), (1, 1)] + GENERIC_RATIOS
NCH = 8
OUT_TILES = 3 * 1024 + 300                    # a tile holds at most 1024 outputs: more than three per channel
FP = C.POINTER(C.c_float)


def _signals(nin, seed):
    """float32[8, nin]: noise, tones, an impulse, full-scale steps, and four more of the same kinds with other parameters."""
    rng = np.random.default_rng(seed)
    n = np.arange(nin, dtype=np.float64)
    x = np.zeros((NCH, nin), np.float64)
    x[0] = rng.standard_normal(nin)
    x[1] = 0.5 * np.cos(0.05 * n + 1.0) + 0.3 * np.cos(1.3 * n) + 0.2 * np.cos(2.9 * n + 2.0)
    x[2, nin // 3] = 1.0
    x[3] = np.where((n // 37) % 2 == 0, 1.0, -1.0)
    x[4] = rng.uniform(-1, 1, nin)
    x[5] = np.cos(np.pi * n)                                            # the input Nyquist, full scale
    x[6, 0] = x[6, nin - 1] = -1.0
    x[7] = np.where(n >= nin // 2, 1.0, 0.0)                            # one step
    return x.astype(np.float32)


_CACHE = {}


def case(up, down):
    """Shared per ratio, computed once and never written: the input, the library's taps, the model's output and its per-sample sum |h x|."""
    key = (up, down)
    if key not in _CACHE:
        import phaze_amd
        taps, L, M, W = phaze_amd.resample_design(up, down)
        nin = -(-OUT_TILES * M // L) + W
        x = _signals(nin, up * 10007 + down)
        m = RM.ResampleModel(up, down, NCH, taps)
        y, b = m.process(x, bound=True)
        for a in (x, taps, y, b):
            a.setflags(write=False)
        _CACHE[key] = dict(x=x, taps=taps, L=L, M=M, W=W, T=2 * W, y=y, b=b, hist=m.hist.copy(), I=m.I, J=m.J)
    return _CACHE[key]


def _process_strided(rs, x, pad_in, pad_out):
    """One host call through the raw C entry point with channel strides longer than the rows."""
    nch, nin = x.shape
    cap = rs.out_count(nin)
    xin = np.full((nch, nin + pad_in), np.nan, np.float32)
    xin[:, :nin] = x
    out = np.full((nch, cap + pad_out), -77.0, np.float32)
    n = C.c_int64()
    rc = rs._L.pv_resample_process(rs._h, xin.ctypes.data_as(FP), nch, nin, nin + pad_in, out.ctypes.data_as(FP), cap + pad_out, cap, C.byref(n))
    assert rc == 0, rs._L.pv_resample_last_error(rs._h)
    assert n.value == cap and np.all(out[:, cap:] == -77.0)            # nothing written behind the row
    return out[:, :cap].copy()


def _state(rs, nch):
    st = [rs.export_state(c) for c in range(nch)]
    return np.stack([s[0] for s in st]), st[0][1], st[0][2]


@pytest.mark.parametrize("up,down", RATIOS)
def test_every_sample_is_within_the_derived_bound_of_the_model(up, down):
    import phaze_amd
    k = case(up, down)
    assert k["y"].shape[1] == RM.count(up, down, k["x"].shape[1]) >= OUT_TILES
    for nch, pads in ((1, (0, 0)), (2, (5, 3)), (8, (1, 129))):
        rs = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=k["x"].shape[1])
        y = _process_strided(rs, k["x"][:nch], *pads)
        tol = (k["T"] + 1) * 2.0 ** -24 * k["b"][:nch]
        err = np.abs(y.astype(np.float64) - k["y"][:nch])
        worst = float(np.max(err / np.maximum(tol, 1e-300)))
        print(f"{up}/{down} nch {nch}: worst |err| / bound = {worst:.3f}, max |err| = {err.max():.3e}")
        assert np.all(err <= tol), (nch, int(np.sum(err > tol)), worst)
        hist, I, J = _state(rs, nch)
        assert np.array_equal(hist, k["hist"][:nch]) and (I, J) == (k["I"], k["J"])
        rs.close()


def _feed(rs, x, sizes, up, down):
    """Feed x in calls of the given sizes (host form), checking every count; returns the concatenated output."""
    at, parts = 0, []
    for n in sizes:
        want = RM.count(up, down, at + n) - RM.count(up, down, at)
        assert rs.out_count(n) == want
        y = rs.process(x[:, at:at + n])
        assert y.shape[1] == want
        parts.append(y)
        at += n
    assert at == x.shape[1]
    return np.concatenate(parts, axis=1)


def _sizes(total, draw):
    out = []
    while total > 0:
        n = min(total, draw())
        out.append(n)
        total -= n
    return out


@pytest.mark.parametrize("up,down", RATIOS)
def test_any_split_of_a_stream_gives_the_same_bits(up, down):
    import phaze_amd
    import torch
    k = case(up, down)
    nch, x, W, T = 2, k["x"][:2], k["W"], k["T"]
    nin = x.shape[1]
    rng = np.random.default_rng(down * 7919 + up)
    one = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=nin)
    whole = one.process(x)
    hist, I, J = _state(one, nch)
    assert (I, J) == (nin, RM.count(up, down, nin))

    def same(rs, y, what):
        assert y.shape == whole.shape and np.array_equal(y, whole), what
        h2, I2, J2 = _state(rs, nch)
        assert np.array_equal(h2, hist) and (I2, J2) == (I, J), what

    # random splits, among them empty calls and calls shorter than the filter
    rs = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=nin)
    same(rs, _feed(rs, x, _sizes(nin, lambda: int(rng.choice([0, 1, W - 1, W, T, int(rng.integers(1, 3000))]))), up, down), "random splits")
    # host pieces: one call, staged through a small buffer
    rs = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=257)
    same(rs, _feed(rs, x, [nin], up, down), "host pieces")
    # export / import hand-over mid-stream, at a point that is no multiple of anything
    a, b = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=nin), phaze_amd.Resampler(up, down, max_channels=nch, max_samples=nin)
    cut = nin // 2 + 13
    ya = _feed(a, x[:, :cut], [cut], up, down)
    for c in range(nch):
        b.import_state(c, *a.export_state(c))
    ob = RM.count(up, down, nin) - RM.count(up, down, cut)
    assert b.out_count(nin - cut) == ob
    yb = b.process(x[:, cut:])
    same(b, np.concatenate([ya, yb], axis=1), "export / import")
    # the device form on a user stream, in random pieces, padded strides
    rs = phaze_amd.Resampler(up, down, max_channels=nch)
    stream = torch.cuda.Stream()
    rs.set_stream(stream.cuda_stream)
    d_in = torch.zeros((nch, nin + 7), dtype=torch.float32, device="cuda")
    d_in[:, :nin] = torch.from_numpy(x.copy()).cuda()
    d_out = torch.full((nch, whole.shape[1] + 5), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    at = done = 0
    for n in _sizes(nin, lambda: int(rng.integers(1, 4000))):
        got = rs.process_device(d_in.data_ptr() + 4 * at, nch, n, nin + 7, d_out.data_ptr() + 4 * done, whole.shape[1] + 5, whole.shape[1] - done)
        assert got == RM.count(up, down, at + n) - RM.count(up, down, at)
        at, done = at + n, done + got
    rs.synchronize()
    yd = d_out.cpu().numpy()
    assert np.all(yd[:, whole.shape[1]:] == -77.0)
    same(rs, yd[:, :whole.shape[1]], "device form")
    rs.set_stream(None)
    # 1-sample calls and calls shorter than W: on a prefix (the output of a prefix is a prefix of the output)
    short = min(nin, 6 * T + 40 * max(1, down // up))
    for what, draw in (("1-sample calls", lambda: 1), ("calls shorter than W", lambda: int(rng.integers(1, W)))):
        rs = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=W)
        y = _feed(rs, x[:, :short], _sizes(short, draw), up, down)
        assert y.shape[1] == RM.count(up, down, short) > 0 and np.array_equal(y, whole[:, :y.shape[1]]), what
        ref = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=short)
        ref.process(x[:, :short])
        h1, h2 = _state(rs, nch), _state(ref, nch)
        assert np.array_equal(h1[0], h2[0]) and h1[1:] == h2[1:], what


@pytest.mark.parametrize("up,down", [(4, 5), (1, 8), (8, 1), (8191, 8192)] + GENERIC_RATIOS)
def test_a_short_out_capacity_is_refused_with_the_state_untouched(up, down):
    import phaze_amd
    from phaze_amd import capi
    k = case(up, down)
    x = k["x"][:1, :4 * k["T"] + 100]
    rs = phaze_amd.Resampler(up, down, max_samples=x.shape[1])
    first = rs.process(x[:, :k["T"]])
    before = rs.export_state(0)
    n_in = x.shape[1] - k["T"]
    want = rs.out_count(n_in)
    assert want == RM.count(up, down, x.shape[1]) - first.shape[1] > 0
    out = np.full(want, -5.0, np.float32)
    rest = np.ascontiguousarray(x[0, k["T"]:])
    n = C.c_int64(-1)
    rc = rs._L.pv_resample_process(rs._h, rest.ctypes.data_as(FP), 1, n_in, n_in, out.ctypes.data_as(FP), want, want - 1, C.byref(n))
    assert rc == capi.PV_ERR_ARGUMENT and "out_capacity" in rs._L.pv_resample_last_error(rs._h).decode()
    assert np.all(out == -5.0)
    after = rs.export_state(0)
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    y = np.concatenate([first, rs.process(rest[None, :])], axis=1)
    ref = phaze_amd.Resampler(up, down, max_samples=x.shape[1]).process(x)
    assert np.array_equal(y, ref)
    rs.reset()
    assert rs.export_state(0)[1:] == (0, 0) and np.array_equal(rs.process(x), ref)        # a reset handle is a fresh one


# ---- positions far from zero: (I, J) are int64, every launch derives its (n0, phase0) from them in 128-bit arithmetic (run_piece) ----

FAR_RATIOS = [(4, 5), (1, 8), (8, 1), (147, 160), (1024, 8191), (8191, 1024)]
FAR_TARGETS = [2 ** 24, 2 ** 31, 2 ** 32, 2 ** 40, 2 ** 62]


@pytest.mark.parametrize("up,down", FAR_RATIOS)
def test_a_stream_position_shifted_by_whole_periods_changes_no_bit(up, down):
    """For c > W, J(c + k M) = J(c) + k L and output J(c) + k L + j has the phase and the taps of output J(c) + j: a handle that imports A's history at
    (c + k M, J(c) + k L) must produce A's bits from then on, end with A's history, and count (k M, k L) further.  k: the smallest that puts the LARGER of
    the two counters just above 2^24, 2^31, 2^32, 2^40 and 2^62 (for L > M the output counter leads; past 2^63 it would leave int64, which is outside the
    contract).  Host form and device form on a user stream, both in random pieces of their own."""
    import phaze_amd
    import torch
    k_ = case(up, down)
    nch, L, M, W = 2, k_["L"], k_["M"], k_["W"]
    c = 2 * W + 7
    nin = k_["x"].shape[1] + c                                          # the ratio's usual length BEHIND the first c samples: more than three tiles from there
    x = _signals(nin, up * 7 + down)[:nch]
    assert RM.count(up, down, nin) - RM.count(up, down, c) > 3 * 1024
    rng = np.random.default_rng(up * 31 + down)
    a = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=nin)
    a.process(x[:, :c])
    start = [a.export_state(ch) for ch in range(nch)]
    Jc = start[0][2]
    assert (start[0][1], Jc) == (c, RM.count(up, down, c))
    ya = _feed_from(a, x[:, c:], _sizes(nin - c, lambda: int(rng.integers(1, 3000))))
    hist_a, Ia, Ja = _state(a, nch)
    stream = torch.cuda.Stream()
    d_in = torch.from_numpy(x[:, c:].copy()).cuda()
    for target in FAR_TARGETS:
        k = target // max(L, M) + 1
        assert max(k * L, k * M) > target and k * max(L, M) + 8 * nin < 2 ** 63
        for form in ("host", "device"):
            b = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=4096)
            for ch in range(nch):
                b.import_state(ch, start[ch][0], c + k * M, Jc + k * L)
            sizes = _sizes(nin - c, lambda: int(rng.integers(1, 4000)))
            if form == "host":
                yb = _feed_from(b, x[:, c:], sizes)
            else:
                b.set_stream(stream.cuda_stream)
                d_out = torch.full((nch, ya.shape[1] + 5), -77.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                at = done = 0
                for n in sizes:
                    got = b.process_device(d_in.data_ptr() + 4 * at, nch, n, nin - c, d_out.data_ptr() + 4 * done, ya.shape[1] + 5, ya.shape[1] - done)
                    at, done = at + n, done + got
                b.synchronize()
                yd = d_out.cpu().numpy()
                assert done == ya.shape[1] and np.all(yd[:, done:] == -77.0)
                yb = np.ascontiguousarray(yd[:, :done])
                b.set_stream(None)
            what = f"{form} form, k M = {k * M}, k L = {k * L}"
            assert yb.shape == ya.shape and np.array_equal(yb.view(np.uint32), ya.view(np.uint32)), what
            hist_b, Ib, Jb = _state(b, nch)
            assert np.array_equal(hist_b.view(np.uint32), hist_a.view(np.uint32)) and (Ib, Jb) == (Ia + k * M, Ja + k * L), what
            b.close()
    a.close()


def _feed_from(rs, x, sizes):
    """Feed x in host calls of the given sizes from wherever the handle stands, checking every count against the handle's own closed form."""
    at, parts = 0, []
    I0 = rs.export_state(0)[1]
    for n in sizes:
        want = RM.count(rs.up, rs.down, I0 + at + n) - RM.count(rs.up, rs.down, I0 + at)
        assert rs.out_count(n) == want
        parts.append(rs.process(x[:, at:at + n]))
        assert parts[-1].shape[1] == want
        at += n
    assert at == x.shape[1]
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("up,down", [(4, 5), (100, 97), (16, 125), (8191, 8192)])
def test_a_stream_picked_up_at_2_to_the_40_is_within_the_derived_bound_of_the_model(up, down):
    """A position that is no multiple of anything: I0 = 2^40 + 12345, J0 = J(I0), a random history.  The model's index arithmetic is Python / int64 and holds
    there (tests/test_resample_model.py checks it against a shifted run); the bound is the file's own, no sample left out."""
    import phaze_amd
    k = case(up, down)
    nch, x = 2, k["x"][:2]
    I0 = 2 ** 40 + 12345
    J0 = RM.count(up, down, I0)
    assert phaze_amd.resample_count(up, down, I0) == J0
    hist = (np.random.default_rng(up + down).standard_normal((nch, k["T"] - 1)) * 0.5).astype(np.float32)
    m = RM.ResampleModel(up, down, nch, k["taps"])
    m.hist[:], m.I, m.J = hist, I0, J0
    ym, bm = m.process(x, bound=True)
    assert ym.shape[1] == RM.count(up, down, I0 + x.shape[1]) - J0 >= 3 * 1024
    rs = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=x.shape[1])
    for ch in range(nch):
        rs.import_state(ch, hist[ch], I0, J0)
    y = rs.process(x)
    tol = (k["T"] + 1) * 2.0 ** -24 * bm
    err = np.abs(y.astype(np.float64) - ym)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{up}/{down} from 2^40 + 12345: worst |err| / bound = {worst:.3f}, max |err| = {err.max():.3e}")
    assert y.shape == ym.shape and np.all(err <= tol), (int(np.sum(err > tol)), worst)
    h2, I2, J2 = _state(rs, nch)
    assert np.array_equal(h2, m.hist) and (I2, J2) == (m.I, m.J) == (I0 + x.shape[1], J0 + y.shape[1])
    rs.close()


def test_one_device_call_longer_than_a_launch_piece_equals_two_calls():
    """The only test here that is large by necessity: pv_resample_process_device cuts a call into launches of at most 2^27 inputs (kPiece), and only a call
    longer than that runs the loop.  One channel at 1/8, 2^27 + 5000 samples made on the device (0.54 GB in, 67 MB out): one call of the whole against two
    calls split at 2^26 + 333 on a second handle.  Same samples, same counters; nothing but the counters and three booleans leaves the device.
    Measured on an MI355X: 1.4 ms of device work per handle, 0.19 s for the test.  The same at 8/1 would write 4.3 GB per handle on a card the suite
    shares; it is left out -- at 8/1 the launch differs from this one in its output count only, and that stays below 2^31 by kPiece's choice."""
    import time

    import phaze_amd
    import torch
    up, down, nin, cut = 1, 8, 2 ** 27 + 5000, 2 ** 26 + 333
    nout = RM.count(up, down, nin)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    d_in = torch.randn(nin, dtype=torch.float32, device="cuda", generator=gen)
    outs, counters = [], []
    for calls in ([nin], [cut, nin - cut]):
        rs = phaze_amd.Resampler(up, down, max_channels=1, max_samples=4096)
        d_out = torch.full((nout + 16,), -77.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        at = done = 0
        for n in calls:
            done += rs.process_device(d_in.data_ptr() + 4 * at, 1, n, nin, d_out.data_ptr() + 4 * done, nout + 16, nout - done)
            at += n
        rs.synchronize()
        dt = time.perf_counter() - t0
        print(f"1/8 over {nin} samples in {len(calls)} call(s): {dt * 1e3:.1f} ms")
        assert done == nout and bool(torch.all(d_out[nout:] == -77.0))
        outs.append(d_out)
        i, j = C.c_int64(), C.c_int64()
        assert rs._L.pv_resample_export_state(rs._h, 0, None, C.byref(i), C.byref(j)) == 0          # the counters alone: no sample leaves the device
        counters.append((i.value, j.value))
        rs.close()
    assert counters[0] == counters[1] == (nin, nout)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all()) and float(outs[0][:nout].abs().max()) > 0.1


def _f32_bound(taps):
    """(T + 1) 2^-24 max over phases of sum |h|: the derived bound for an input of magnitude <= 1."""
    return (taps.shape[1] + 1) * 2.0 ** -24 * float(np.max(np.abs(taps.astype(np.float64)).sum(axis=1)))


@pytest.mark.parametrize("up,down", TRM.RATIOS)
def test_passband_tones_follow_the_cosine_on_the_gpu(up, down):
    """The closed form directly, not through the model: gated at the model's own CPU-measured distance from the cosine plus the derived f32 bound."""
    import phaze_amd
    taps = phaze_amd.resample_design(up, down)[0]
    for frac in (0.01, 0.1, 0.5, 0.8):
        rs = phaze_amd.Resampler(up, down)
        gate = TRM.tone_error(up, down, frac) + _f32_bound(taps)
        err = TRM.tone_error(up, down, frac, process=rs.process)
        print(f"gpu passband {up}/{down} at {frac}: {err:.3e} (gate {gate:.3e})")
        assert err <= gate, (frac, err, gate)


@pytest.mark.parametrize("up,down", sorted(TRM.STOPBAND))
def test_a_tone_above_the_output_nyquist_is_removed_on_the_gpu(up, down):
    import phaze_amd
    taps = phaze_amd.resample_design(up, down)[0]
    rs = phaze_amd.Resampler(up, down)
    gate = TRM.alias_ratio(up, down) + _f32_bound(taps) * np.sqrt(2.0)          # the bound per sample, over the unit tone's RMS
    r = TRM.alias_ratio(up, down, process=rs.process)
    print(f"gpu stopband {up}/{down}: {r:.3e} (gate {gate:.3e})")
    assert r <= gate, (r, gate)
