"""The variable-ratio resampler kernel (VariResampler / pv_vari_*) on the GPU against the numpy model (tests/vari_model.py), and split invariance.

Tolerance against the model, DERIVED, u = 2^-24.  The model forms weights and sums in fp64 from the library's own table P and the same f32 input; its
own rounding is far inside one unit of what follows.  The kernel's weight is w^ = fl(fma(f^, d^, P[q])) with f^ = fl(rem * fl(1 / den)) (rem and den are
exact in f32) and d^ = fl(P[q + 1] - P[q]): three roundings on the product f d and one on the result, so |w^ - w| <= u |w| + 3 u |f d| <= 3 u m with
m = |w| + |f d| >= |w| -- the table differences are small beside the entries except next to a zero crossing of the prototype, where |w| alone would
not cover them, hence m.  A tap whose weight is exactly 0 adds nothing and rounds nothing, so with Tloc non-zero taps the numerator, Tloc fused
multiply-adds into one f32 accumulator, is within (Tloc + 3) u A of sum w x, A = sum m |x|, and the weight sum within (Tloc + 3) u S of D = sum w,
S = sum m.  The quotient of the two adds the relative errors and the division rounds once:
    |y_gpu - y| <= u [ (Tloc + 3) (A + |y| S) / |D| + |y| ]
to first order; the terms of second order are below (Tloc + 3) u S / D < 2^-13 of the bound and are covered by the factor 1 + 2^-10.  A, S, D and Tloc
come from the model for that very sample; 2^-149 stands for an output in the subnormal range.  No sample is left out.  Everything else is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import vari_model as VM

pytestmark = pytest.mark.gpu

NCH = 8
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int32)
U = 2.0 ** -24


def _counts(name):
    """(B, min_count, max_count, counts).  A tile holds at most 1024 outputs: every schedule has more than three tiles of output."""
    rng = np.random.default_rng(len(name) * 1009 + ord(name[0]))
    if name == "320-ramp":
        return 320, 200, 440, np.round(np.linspace(200, 440, 13)).astype(np.int32)
    if name == "320-random":
        return 320, 200, 440, rng.integers(200, 441, 13).astype(np.int32)
    if name == "320-alternate":
        return 320, 200, 440, np.tile([200, 440], 6).astype(np.int32)
    if name == "64-extremes":          # both 8:1 extremes; 150 blocks of 8 outputs put more than a hundred blocks into one tile
        return 64, 8, 512, np.concatenate([np.full(150, 8), np.full(3, 512), rng.integers(8, 513, 12), np.full(40, 9), [511, 8, 512]]).astype(np.int32)
    if name == "64-alternate":
        return 64, 8, 512, np.tile([8, 512], 7).astype(np.int32)
    if name == "1-edge":               # hs = 1: a block is one sample
        return 1, 1, 8, np.concatenate([rng.integers(1, 9, 700), np.full(300, 1), np.tile([1, 8], 60)]).astype(np.int32)
    if name == "4096-long":            # a block longer than a tile, the largest numerators (W = 256, c = 8192)
        return 4096, 512, 8192, np.array([8192, 512, 8191, 513], np.int32)
    raise KeyError(name)


CASES = ["320-ramp", "320-random", "320-alternate", "64-extremes", "64-alternate", "1-edge", "4096-long"]


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
    x[5] = np.cos(np.pi * n)
    x[6, 0] = x[6, nin - 1] = -1.0
    x[7] = np.where(n >= nin // 2, 1.0, 0.0)
    return x.astype(np.float32)


_CACHE = {}


def case(name):
    """Shared per schedule, computed once and never written: the input, the library's table, the model's output and its bound terms."""
    if name not in _CACHE:
        import phaze_amd
        B, lo, hi, counts = _counts(name)
        table = phaze_amd.vari_prototype()
        x = _signals(counts.size * B, B * 31 + counts.size)
        m = VM.VariModel(B, lo, hi, NCH, table)
        y, A, S, D, Tloc = m.process(x, counts, bound=True)
        tol = (U * ((Tloc + 3) * (A + np.abs(y) * S) / np.abs(D) + np.abs(y))) * (1.0 + 2.0 ** -10) + 2.0 ** -149
        for a in (x, counts, y, tol):
            a.setflags(write=False)
        assert counts.sum() > 3 * 1024 and np.all(D > 0.5)
        _CACHE[name] = dict(B=B, lo=lo, hi=hi, counts=counts, x=x, y=y, tol=tol, T=m.T, W=m.W, hist=m.hist.copy(), total=int(counts.sum()))
    return _CACHE[name]


def _make(k, nch, max_blocks=0):
    import phaze_amd
    return phaze_amd.VariResampler(k["B"], k["lo"], k["hi"], max_channels=nch, max_blocks=max_blocks)


def _process_strided(rs, x, counts, pad_in, pad_out):
    """One host call through the raw C entry point with channel strides longer than the rows."""
    nch, nin = x.shape
    cap = int(counts.sum())
    xin = np.full((nch, nin + pad_in), np.nan, np.float32)
    xin[:, :nin] = x
    out = np.full((nch, cap + pad_out), -77.0, np.float32)
    n = C.c_int64()
    rc = rs._L.pv_vari_process(rs._h, xin.ctypes.data_as(FP), nch, counts.size, counts.ctypes.data_as(IP), nin + pad_in, out.ctypes.data_as(FP), cap + pad_out, cap,
                               C.byref(n))
    assert rc == 0, rs._L.pv_vari_last_error(rs._h)
    assert n.value == cap and np.all(out[:, cap:] == -77.0)            # nothing written behind the row
    return out[:, :cap].copy()


def _state(rs, nch):
    st = [rs.export_state(c) for c in range(nch)]
    return np.stack([s[0] for s in st]), st[0][1], st[0][2]


@pytest.mark.parametrize("name", CASES)
def test_every_sample_is_within_the_derived_bound_of_the_model(name):
    k = case(name)
    for nch, pads in ((1, (0, 0)), (8, (1, 129))):
        rs = _make(k, nch, k["counts"].size)
        y = _process_strided(rs, k["x"][:nch], k["counts"], *pads)
        err = np.abs(y.astype(np.float64) - k["y"][:nch])
        worst = float(np.max(err / k["tol"][:nch]))
        print(f"{name} nch {nch}: worst |err| / bound = {worst:.3f}, max |err| = {err.max():.3e}")
        assert np.all(err <= k["tol"][:nch]), (nch, int(np.sum(err > k["tol"][:nch])), worst)
        hist, blocks, outputs = _state(rs, nch)
        assert np.array_equal(hist, k["hist"][:nch]) and (blocks, outputs) == (k["counts"].size, k["total"])
        rs.close()


def _feed(rs, x, counts, B, sizes):
    at, parts = 0, []
    for n in sizes:
        parts.append(rs.process(x[:, at * B:(at + n) * B], counts[at:at + n]))
        at += n
    assert at == counts.size
    return np.concatenate(parts, axis=1)


def _sizes(total, draw):
    out = []
    while total > 0:
        n = min(total, draw())
        out.append(n)
        total -= n
    return out


@pytest.mark.parametrize("name", CASES)
def test_any_split_of_a_stream_gives_the_same_bits(name):
    import torch
    k = case(name)
    nch, B, counts, total = 3, k["B"], k["counts"], k["total"]
    x = k["x"][[0, 1, 4]]
    nb = counts.size
    rng = np.random.default_rng(nb * 7919 + B)
    one = _make(k, nch, nb)
    whole = one.process(x, counts)
    hist, blocks, outputs = _state(one, nch)
    assert whole.shape == (nch, total) and (blocks, outputs) == (nb, total)

    def same(rs, y, what):
        assert y.shape == whole.shape and np.array_equal(y.view(np.uint32), whole.view(np.uint32)), what
        h2, b2, o2 = _state(rs, nch)
        assert np.array_equal(h2, hist) and (b2, o2) == (blocks, outputs), what

    # block by block (at most 64 blocks one by one, then the rest: the 1-sample shape has a thousand), and random splits with empty calls among them
    rs = _make(k, nch, nb)
    same(rs, _feed(rs, x, counts, B, [1] * min(nb, 64) + ([nb - 64] if nb > 64 else [])), "block by block")
    rs = _make(k, nch, nb)
    same(rs, _feed(rs, x, counts, B, _sizes(nb, lambda: int(rng.integers(0, max(2, nb // 3))))), "random splits")
    # host pieces: one call, staged through a buffer of two blocks
    rs = _make(k, nch, 2)
    same(rs, _feed(rs, x, counts, B, [nb]), "host pieces")
    # export / import hand-over mid-stream
    a, b = _make(k, nch, nb), _make(k, nch, nb)
    cut = nb // 2 + 1
    ya = a.process(x[:, :cut * B], counts[:cut])
    for c in range(nch):
        b.import_state(c, *a.export_state(c))
    same(b, np.concatenate([ya, b.process(x[:, cut * B:], counts[cut:])], axis=1), "export / import")
    # the device form on a user stream, in random pieces, padded strides
    rs = _make(k, nch)
    stream = torch.cuda.Stream()
    rs.set_stream(stream.cuda_stream)
    nin = nb * B
    d_in = torch.zeros((nch, nin + 7), dtype=torch.float32, device="cuda")
    d_in[:, :nin] = torch.from_numpy(x.copy()).cuda()
    d_out = torch.full((nch, total + 5), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    at = done = 0
    for n in _sizes(nb, lambda: int(rng.integers(1, max(2, nb // 2)))):
        got = rs.process_device(d_in.data_ptr() + 4 * at * B, nch, counts[at:at + n], nin + 7, d_out.data_ptr() + 4 * done, total + 5, total - done)
        assert got == int(counts[at:at + n].sum())
        at, done = at + n, done + got
    rs.synchronize()
    yd = d_out.cpu().numpy()
    assert np.all(yd[:, total:] == -77.0)                                # nothing written past sum(counts)
    same(rs, np.ascontiguousarray(yd[:, :total]), "device form")
    rs.set_stream(None)
    # a channel alone and the same channel among others
    solo = _make(k, 1, nb)
    assert np.array_equal(solo.process(x[1:2], counts).view(np.uint32), whole[1:2].view(np.uint32))
    # a reset handle is a fresh one
    one.reset()
    assert one.export_state(0)[1:] == (0, 0)
    same(one, one.process(x, counts), "after reset")


@pytest.mark.parametrize("name", ["320-ramp", "64-extremes"])
def test_bad_calls_are_refused_with_the_state_untouched(name):
    from phaze_amd import capi
    k = case(name)
    B, counts = k["B"], k["counts"]
    x = np.ascontiguousarray(k["x"][:1])
    rs = _make(k, 1, counts.size)
    cut = 3
    first = rs.process(x[:, :cut * B], counts[:cut])
    before = rs.export_state(0)
    rest, rc_counts = np.ascontiguousarray(x[0, cut * B:]), np.ascontiguousarray(counts[cut:])
    want = int(rc_counts.sum())
    out = np.full(want, -5.0, np.float32)
    n = C.c_int64(-1)

    def call(cnts, cap):
        return rs._L.pv_vari_process(rs._h, rest.ctypes.data_as(FP), 1, cnts.size, cnts.ctypes.data_as(IP), rest.size, out.ctypes.data_as(FP), want, cap, C.byref(n))

    assert call(rc_counts, want - 1) == capi.PV_ERR_ARGUMENT and "out_capacity" in rs._L.pv_vari_last_error(rs._h).decode()
    for bad in (k["lo"] - 1, k["hi"] + 1):
        c2 = rc_counts.copy()
        c2[2] = bad
        assert call(c2, want) == capi.PV_ERR_ARGUMENT and "block 2" in rs._L.pv_vari_last_error(rs._h).decode()
    assert rs._L.pv_vari_process(rs._h, rest.ctypes.data_as(FP), 1, rc_counts.size, None, rest.size, out.ctypes.data_as(FP), want, want, C.byref(n)) == capi.PV_ERR_ARGUMENT
    assert rs._L.pv_vari_process(rs._h, rest.ctypes.data_as(FP), 2, rc_counts.size, rc_counts.ctypes.data_as(IP), rest.size, out.ctypes.data_as(FP), want, want,
                                 C.byref(n)) == capi.PV_ERR_CAPACITY
    assert np.all(out == -5.0)
    after = rs.export_state(0)
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    y = np.concatenate([first, rs.process(rest[None, :], rc_counts)], axis=1)
    ref = _make(k, 1, counts.size).process(x, counts)
    assert np.array_equal(y, ref)


def test_passband_tones_follow_the_cosine_on_the_gpu():
    """The closed form directly, not through the model: gated at the model's own CPU-measured distance from the cosine plus the derived f32 bound for a
    unit input, (T + 3) u (A + |y| S) / D + u |y| with A <= S, |y| <= 1 and S <= 2.3 D (the prototype's negative lobes: S / D is 2.27 at most over every
    case of this file, on the model) -- 4.6 (T + 3) u + u."""
    import phaze_amd
    import test_vari_model as TVM
    table = phaze_amd.vari_prototype()
    for name in ("ramp", "64x8", "64x512"):
        B, lo, hi, _ = TVM.schedule(name)
        rs = phaze_amd.VariResampler(B, lo, hi)
        for frac in (0.1, 0.8):
            gate = TVM.tone_error(name, frac, table=table) + (4.6 * (rs.taps + 3) + 1) * U
            err = TVM.tone_error(name, frac, process=rs.process)
            rs.reset()
            print(f"gpu passband {name} at {frac}: {err:.3e} (gate {gate:.3e})")
            assert err <= gate, (name, frac, err, gate)


def test_one_device_call_longer_than_a_launch_piece_equals_two_calls():
    """Large by necessity, as its twin in tests/test_gpu_resample.py: pv_vari_process_device cuts a call into launches of at most 2^24 blocks (and 2^27
    inputs), and only a longer call runs that loop.  One channel, B = 8, 2^24 + 1000 blocks of alternating counts 1 / 2 made on the device (0.54 GB in,
    0.1 GB out): one call of the whole against two calls split at 2^23 + 333 on a second handle.  Same samples, same counters; nothing but the counters
    and three booleans leaves the device."""
    import phaze_amd
    import torch
    B, nb, cut = 8, 2 ** 24 + 1000, 2 ** 23 + 333
    counts = np.ones(nb, np.int32)
    counts[1::2] = 2
    total = int(counts.astype(np.int64).sum())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    d_in = torch.randn(nb * B, dtype=torch.float32, device="cuda", generator=gen)
    outs, counters = [], []
    for calls in ([nb], [cut, nb - cut]):
        rs = phaze_amd.VariResampler(B, 1, 2, max_channels=1, max_blocks=1)
        d_out = torch.full((total + 16,), -77.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        at = done = 0
        for n in calls:
            done += rs.process_device(d_in.data_ptr() + 4 * at * B, 1, counts[at:at + n], nb * B, d_out.data_ptr() + 4 * done, total + 16, total - done)
            at += n
        rs.synchronize()
        assert done == total and bool(torch.all(d_out[total:] == -77.0))
        outs.append(d_out)
        i, j = C.c_int64(), C.c_int64()
        assert rs._L.pv_vari_export_state(rs._h, 0, None, C.byref(i), C.byref(j)) == 0          # the counters alone: no sample leaves the device
        counters.append((i.value, j.value))
        rs.close()
    assert counters[0] == counters[1] == (nb, total)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all()) and float(outs[0][:total].abs().max()) > 0.1
