"""The sample-value axis of the resamplers, the pitch handles and the analysis paths on the GPU: NaN, +Inf, -Inf and extreme amplitudes in the input.

1. VariResampler (pv_vari_*).  RULE (pv_vari.h, NON-FINITE INPUT): output j is non-finite exactly when a non-finite input sample, carried history included,
   lies under a tap of j whose weight is non-zero; every other output has the value it would have with the bad samples replaced by 0.  The mask comes
   from tests/vari_model.py (reach=True: `non-zero` in the kernel's own f32 arithmetic), the values from the model on the zeroed input at the derived
   bound of tests/test_gpu_vari.py, unchanged.  Every call form of that file's split test is run: which zero taps a launch executes depends on the tile,
   so a kernel that lets 0 * NaN into the sum passes some forms and fails others.  The test asserts that the set Z of outputs with a bad sample only
   under ZERO weights is not empty: without Z the rule could not be told from `any bad sample under the T taps` (what the fp64 model does by default)
   nor from the tile-dependent behaviour.
2. Resampler (pv_resample_*).  RULE (pv_resample.h): every output runs all T taps of its phase row, so output j is non-finite exactly when its T-tap
   window holds a bad sample, zero taps included; split-invariant by construction.
3. PitchStretch and PitchGlide with a NaN and an Inf in the input are still their two stages run separately, bit for bit on every finite sample, with
   equal finite masks, in every cut; the output and both states are finite again from a position derived below.
4. PitchGlide.process_tuned and TimeStretch.onset_strength with a bad sample: the frames that hold it give zero records / zero counts.
5. Scaling by a power of two is exact: y(2^k x) == 2^k y(x) bit for bit for both resamplers at k = +-40 (the model checks that nothing leaves the
   normal range), track(2^k x) == track(x) at k = +-20, +-100 and at a peak of FLT_MAX (the largest exponent).
6. The overlap-add path (pv_psola_*, pv_tsm_*, pv_epoch_*) has this axis in tests/test_gpu_ola_ranges.py: exact scaling up to 2^122, inputs in the
   subnormal range against a derived bound, the epoch records under 2^k and at FLT_MAX, and positions and displacements up to 2^30 - 1."""
import ctypes as C

import numpy as np
import pytest

import f0_model as FM
import resample_model as RM
import transient_model as TM
import vari_model as VM
import test_gpu_f0 as TGF
import test_gpu_glide as TGG
import test_gpu_pitch as TGP
import test_gpu_resample as TGR
import test_gpu_vari as TGV

pytestmark = pytest.mark.gpu

KINDS = [np.nan, np.inf, -np.inf]                  # channels 1, 2, 3; channel 0 stays clean: channels are independent
FP = C.POINTER(C.c_float)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _poison(x, positions):
    """float32[4, n]: channel 0 as it is, channels 1 .. 3 with NaN, +Inf, -Inf at each of the positions."""
    x = np.array(x[:4], np.float32)
    for ch, v in enumerate(KINDS, start=1):
        x[ch, positions] = v
    return x


def _same_finite(y, first, what):
    ok = np.isfinite(first)
    assert np.array_equal(np.isfinite(y), ok), what
    assert np.array_equal(_bits(y)[ok], _bits(first)[ok]), what


# ---- 1. the variable-ratio resampler: the reach of a bad sample -------------------------------------------------------------------------------------

_VARI = {}


def vari_case(name):
    """Shared per schedule, computed once and never written.  Bad samples: inside the first T - 1 samples of the stream; on the first sample of a block
    with c >= B that follows a block with c < B, mid-stream; on the last sample before the block the hand-over form cuts at, which every form that ends
    a call there carries into the next call through the history."""
    if name not in _VARI:
        import phaze_amd
        B, lo, hi, counts = TGV._counts(name)
        nb = counts.size
        m = VM.VariModel(B, lo, hi, 4, phaze_amd.vari_prototype())
        b_mid = next(b for b in range(nb // 3, nb) if counts[b - 1] < B <= counts[b])
        cut = nb // 2 + 1
        positions = [m.T // 2, b_mid * B, cut * B - 1]
        far = np.diff(np.sort(positions + [nb * B]))
        assert positions[0] < m.T - 1 and counts[cut - 1] != counts[b_mid] and np.all(far > m.T)         # no output sees two of them
        x = _poison(TGV._signals(nb * B, B * 31 + nb)[[1, 0, 4, 3]], positions)
        y, A, S, D, Tloc, poisoned, near = m.process(x, counts, bound=True, reach=True)
        tol = (TGV.U * ((Tloc + 3) * (A + np.abs(y) * S) / np.abs(D) + np.abs(y))) * (1.0 + 2.0 ** -10) + 2.0 ** -149
        assert np.all(D > 0.5) and np.all(np.isfinite(y))
        for a in (x, counts, y, tol, poisoned, near):
            a.setflags(write=False)
        _VARI[name] = dict(B=B, lo=lo, hi=hi, counts=counts, x=x, y=y, tol=tol, poisoned=poisoned, near=near, T=m.T, W=m.W, cut=cut, total=int(counts.sum()),
                           positions=positions)
    return _VARI[name]


def _vari_forms(k):
    """(name, output, handle) of every call form of tests/test_gpu_vari.py::test_any_split_of_a_stream_gives_the_same_bits, and of two calls that meet
    right behind the third bad sample."""
    import torch
    nch, B, counts, total, x = 4, k["B"], k["counts"], k["total"], k["x"]
    nb = counts.size
    rng = np.random.default_rng(nb * 7919 + B)
    rs = TGV._make(k, nch, nb)
    yield "one call", rs.process(x, counts), rs
    rs = TGV._make(k, nch, nb)
    yield "block by block", TGV._feed(rs, x, counts, B, [1] * min(nb, 64) + ([nb - 64] if nb > 64 else [])), rs
    rs = TGV._make(k, nch, nb)
    yield "random splits", TGV._feed(rs, x, counts, B, TGV._sizes(nb, lambda: int(rng.integers(0, max(2, nb // 3))))), rs
    rs = TGV._make(k, nch, 2)
    yield "host pieces", TGV._feed(rs, x, counts, B, [nb]), rs
    rs = TGV._make(k, nch, nb)
    yield "two calls", TGV._feed(rs, x, counts, B, [k["cut"], nb - k["cut"]]), rs
    a, b = TGV._make(k, nch, nb), TGV._make(k, nch, nb)
    cut = k["cut"]
    ya = a.process(x[:, :cut * B], counts[:cut])
    for c in range(nch):
        hist, blocks, outputs = a.export_state(c)
        assert np.array_equal(_bits(hist), _bits(x[c, cut * B - (k["T"] - 1):cut * B]))       # the bad sample is the newest of the exported history
        b.import_state(c, hist, blocks, outputs)
    yield "export / import", np.concatenate([ya, b.process(x[:, cut * B:], counts[cut:])], axis=1), b
    rs = TGV._make(k, nch)
    stream = torch.cuda.Stream()
    rs.set_stream(stream.cuda_stream)
    nin = nb * B
    d_in = torch.zeros((nch, nin + 7), dtype=torch.float32, device="cuda")
    d_in[:, :nin] = torch.from_numpy(x.copy()).cuda()
    d_out = torch.full((nch, total + 5), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    at = done = 0
    for n in TGV._sizes(nb, lambda: int(rng.integers(1, max(2, nb // 2)))):
        got = rs.process_device(d_in.data_ptr() + 4 * at * B, nch, counts[at:at + n], nin + 7, d_out.data_ptr() + 4 * done, total + 5, total - done)
        at, done = at + n, done + got
    rs.synchronize()
    yd = d_out.cpu().numpy()
    assert done == total and np.all(yd[:, total:] == -77.0)
    rs.set_stream(None)
    yield "device form", np.ascontiguousarray(yd[:, :total]), rs


@pytest.mark.parametrize("name", ["320-alternate", "64-extremes"])
def test_vari_output_is_non_finite_exactly_under_the_non_zero_taps_in_every_call_form(name):
    k = vari_case(name)
    poisoned, near, x, T = k["poisoned"], k["near"], k["x"], k["T"]
    Z = near & ~poisoned
    print(f"{name}: {poisoned.sum(axis=1).tolist()} poisoned outputs per channel, {Z.sum(axis=1).tolist()} with a bad sample under zero weights only")
    assert not near[0].any() and all(poisoned[c].any() and Z[c].any() for c in (1, 2, 3))      # the test can tell the three behaviours apart
    last = max(int(np.flatnonzero(poisoned[c])[-1]) for c in (1, 2, 3))
    assert last + 1024 < k["total"]                                                            # more than a tile of output behind the last bad one
    first, failures = None, []
    for what, y, rs in _vari_forms(k):
        assert y.shape == poisoned.shape, what
        wrong = np.isfinite(y) == poisoned
        ok = ~poisoned & np.isfinite(y)
        err = np.abs(y.astype(np.float64) - k["y"])
        worst = float(np.max(err[ok] / k["tol"][ok]))
        print(f"{name}, {what}: {int(wrong.sum())} outputs off the mask ({int((wrong & Z).sum())} of them in Z), worst |err| / bound on the finite ones {worst:.3f}")
        if wrong.any():
            failures.append((what, int(wrong.sum()), np.argwhere(wrong)[:4].tolist()))
            continue
        assert np.all(err[ok] <= k["tol"][ok]), (what, worst)                                  # the value with the bad samples replaced by 0
        assert np.all(np.isfinite(y[:, last + 1:])), what                                      # finite from the first output outside the mask on
        if first is None:
            first = y
        _same_finite(y, first, what)
        hist, blocks, outputs = TGV._state(rs, 4)
        assert np.array_equal(_bits(hist), _bits(x[:, x.shape[1] - (T - 1):])) and (blocks, outputs) == (k["counts"].size, k["total"]), what
        rs.close()
    assert not failures, failures


# ---- 2. the fixed-ratio resampler: every output runs all its T taps ---------------------------------------------------------------------------------

RESAMPLE_RATIOS = [(16, 123), (16, 125)]           # the taps-in-LDS instance and the generic one, on the two sides of the LDS budget (tests/test_gpu_resample.py)
_RESAMPLE = {}


def resample_case(up, down):
    if (up, down) not in _RESAMPLE:
        k = TGR.case(up, down)
        L, M, W, T = k["L"], k["M"], k["W"], k["T"]
        nin = k["x"].shape[1]
        cut = nin // 2 + 13
        positions = [T // 2, (nin // 3) | 1, cut - 1]
        x = _poison(k["x"][[1, 0, 4, 3]], positions)
        zeroed = np.where(np.isfinite(x), x, np.float32(0.0))
        y, b = RM.ResampleModel(up, down, 4, k["taps"]).process(zeroed, bound=True)
        J = y.shape[1]
        n = np.arange(J, dtype=np.int64) * M // L                                  # output j reads x[n_j - W + 1 .. n_j + W]
        bad = np.concatenate([np.zeros((4, W - 1), bool), ~np.isfinite(x)], axis=1)
        csum = np.concatenate([np.zeros((4, 1), np.int64), np.cumsum(bad, axis=1)], axis=1)
        poisoned = csum[:, n + T] - csum[:, n] > 0                                  # bad[:, n_j + i], i = 0 .. T - 1
        taps = np.asarray(k["taps"]).reshape(L, T)
        for a in (x, y, b, poisoned):
            a.setflags(write=False)
        _RESAMPLE[(up, down)] = dict(x=x, y=y, b=b, poisoned=poisoned, cut=cut, T=T, W=W, J=J, zero_taps=int(np.count_nonzero(taps == 0.0)))
    return _RESAMPLE[(up, down)]


@pytest.mark.parametrize("up,down", RESAMPLE_RATIOS)
def test_resample_output_is_non_finite_exactly_where_its_window_holds_a_bad_sample(up, down):
    import phaze_amd
    import torch
    k = resample_case(up, down)
    x, poisoned, T, J, cut = k["x"], k["poisoned"], k["T"], k["J"], k["cut"]
    nch, nin = x.shape
    rng = np.random.default_rng(up + down)
    assert not poisoned[0].any() and all(poisoned[c].any() for c in (1, 2, 3)) and J > 3 * 1024
    forms = []
    rs = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=nin)
    forms.append(("one call", rs.process(x), rs))
    rs = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=nin)
    forms.append(("two calls", TGR._feed(rs, x, [cut, nin - cut], up, down), rs))                  # the third bad sample is the last of the first call
    rs = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=nin)
    forms.append(("random splits", TGR._feed(rs, x, TGR._sizes(nin, lambda: int(rng.choice([0, 1, T, int(rng.integers(1, 3000))]))), up, down), rs))
    rs = phaze_amd.Resampler(up, down, max_channels=nch, max_samples=257)
    forms.append(("host pieces", TGR._feed(rs, x, [nin], up, down), rs))
    rs = phaze_amd.Resampler(up, down, max_channels=nch)
    stream = torch.cuda.Stream()
    rs.set_stream(stream.cuda_stream)
    d_in = torch.zeros((nch, nin + 7), dtype=torch.float32, device="cuda")
    d_in[:, :nin] = torch.from_numpy(x.copy()).cuda()
    d_out = torch.full((nch, J + 5), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    at = done = 0
    for n in TGR._sizes(nin, lambda: int(rng.integers(1, 4000))):
        got = rs.process_device(d_in.data_ptr() + 4 * at, nch, n, nin + 7, d_out.data_ptr() + 4 * done, J + 5, J - done)
        at, done = at + n, done + got
    rs.synchronize()
    yd = d_out.cpu().numpy()
    assert done == J and np.all(yd[:, J:] == -77.0)
    rs.set_stream(None)
    forms.append(("device form", np.ascontiguousarray(yd[:, :J]), rs))
    tol = (T + 1) * 2.0 ** -24 * k["b"]
    for what, y, rs in forms:
        assert y.shape == poisoned.shape, what
        wrong = np.isfinite(y) == poisoned
        print(f"{up}/{down}, {what}: {int(wrong.sum())} outputs off the mask; the table holds {k['zero_taps']} zero taps")
        assert not wrong.any(), (what, int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
        ok = ~poisoned
        assert np.all(np.abs(y.astype(np.float64) - k["y"])[ok] <= tol[ok]), what
        _same_finite(y, forms[0][1], what)
        hist, I, Jn = TGR._state(rs, nch)
        assert np.array_equal(_bits(hist), _bits(x[:, nin - (T - 1):])) and (I, Jn) == (nin, J), what
        rs.close()


# ---- 3. the pitch and glide handles: still their two stages, and clean again ------------------------------------------------------------------------

def _last_frame_holding(at, N, s):
    """Frame m of a hop row reads the input [at[m + 1] - N, at[m + 1]): the last one that holds sample s."""
    return int(np.flatnonzero(at[1:] - N <= s)[-1])


def _stretched_clean_from(at, N, HS, s):
    """The first stretched sample no frame holding input sample s reaches, derived as tests/test_gpu_stretch.py::test_non_finite_input_recovers derives
    clean_from: the last such frame, the (N - 1) div hs frames after it that overlap it in the output, one more, times hs."""
    return (_last_frame_holding(at, N, s) + (N - 1) // HS + 1) * HS


def _bad_pair(x, at):
    """A NaN in channel 0 and an Inf in channel 1, on the last sample of frame 19 and inside frame 21: a cut at 20 frames carries them in the state."""
    x = x.copy()
    s_nan, s_inf = int(at[20]) - 1, int(at[21]) + 5
    x[0, s_nan], x[1, s_inf] = np.nan, np.inf
    return x, max(s_nan, s_inf)


def _finite_states(states):
    """_states of tests/test_gpu_glide.py / test_gpu_pitch.py: per channel the stretch's history and accumulator (f32), its two integer phase rows, the
    resampler's history (f32) and its counters."""
    assert len(states) % 6 == 0
    return all(np.all(np.isfinite(a.view(np.float32))) for i, a in enumerate(states) if i % 6 in (0, 1, 4))


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("kind", ["hops", "resets"])
@pytest.mark.parametrize("N,HS,LO,HI", TGG.SHAPES)
def test_glide_handle_with_bad_samples_is_its_two_stages_in_every_cut(N, HS, LO, HI, G, kind):
    import phaze_amd
    import torch
    nch, FRAMES = 2, TGG.FRAMES
    hops, resets = TGG._schedule(kind, np.random.default_rng(23 + G), HS, LO, HI)
    at = np.concatenate([[0], np.cumsum(hops.astype(np.int64))])
    x, s_bad = _bad_pair(TGG._input(N, nch, int(at[-1]), 5), at)
    ts = phaze_amd.TimeStretch(N, LO, HS, max_channels=nch, max_frames=FRAMES, channels_per_group=G)
    rs = phaze_amd.VariResampler(HS, LO, HI, max_channels=nch, max_blocks=FRAMES)
    mid = ts.process_hops(x, hops, resets)
    want = rs.process(mid, hops)
    want_state = TGG._states(ts, rs, nch)
    # clean again: the stretched signal from clean_from on, and every output whose T taps [n - T + 1, n] lie there (n = b hs + (k hs) div c)
    clean_from = _stretched_clean_from(at, N, HS, s_bad)
    T = rs.taps
    n_out = np.concatenate([b * HS + (np.arange(c, dtype=np.int64) * HS) // c for b, c in enumerate(hops.tolist())])
    clean = n_out - (T - 1) >= clean_from
    assert clean.sum() > 1024 and clean_from + T < FRAMES * HS
    assert not np.all(np.isfinite(mid)) and np.all(np.isfinite(mid[:, clean_from:]))
    assert not np.all(np.isfinite(want)) and np.all(np.isfinite(want[:, clean])) and _finite_states(want_state)

    def same(p, y, what):
        assert y.shape == want.shape, what
        _same_finite(y, want, what)
        got = TGG._states(p.stretch, p.resampler, nch)
        assert len(got) == len(want_state) and all(np.array_equal(a, b) for a, b in zip(got, want_state)), what

    for cuts in ([FRAMES], [1, 7, FRAMES - 8], [20, 2, 39], [3] * 20 + [1]):
        p = phaze_amd.PitchGlide(N, HS, LO, HI, max_channels=nch, max_frames=4, channels_per_group=G)
        parts, f0 = [], 0
        for nf in cuts:
            parts.append(p.process(x[:, at[f0]:at[f0 + nf]], hops[f0:f0 + nf], None if resets is None else resets[f0:f0 + nf]))
            f0 += nf
        same(p, np.concatenate(parts, axis=1), cuts)
        p.close()
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
    p.set_stream(None)
    for h in (p, ts, rs):
        h.close()


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("kind", ["fixed", "resets"])
@pytest.mark.parametrize("N,FLOOR,HS", TGP.SHAPES[:2])
def test_pitch_handle_with_bad_samples_is_its_two_stages_in_every_cut(N, FLOOR, HS, G, kind):
    import phaze_amd
    import torch
    nch, FRAMES = 2, TGP.FRAMES
    hops, resets = TGP._schedule(kind, np.random.default_rng(17 + G), N, FLOOR, HS)
    row = np.full(FRAMES, FLOOR, np.int32) if hops is None else hops
    at = np.concatenate([[0], np.cumsum(row.astype(np.int64))])
    x, s_bad = _bad_pair(TGP._input(N, nch, int(at[-1]), 5), at)
    ts = phaze_amd.TimeStretch(N, FLOOR, HS, max_channels=nch, max_frames=FRAMES, channels_per_group=G)
    rs = phaze_amd.Resampler(FLOOR, HS, max_channels=nch, max_samples=FRAMES * HS)
    mid = ts.process_hops(x, hops, resets)
    want = rs.process(mid)
    want_state = TGP._states(ts, rs, nch)
    # clean again: every output whose window [n_j - W + 1, n_j + W] starts at or behind clean_from, n_j = (j M) div L
    clean_from = _stretched_clean_from(at, N, HS, s_bad)
    L, M, W = rs.up, rs.down, rs.half_width
    clean = np.arange(want.shape[1], dtype=np.int64) * M // L - W + 1 >= clean_from
    assert clean.sum() > 1024
    assert not np.all(np.isfinite(mid)) and np.all(np.isfinite(mid[:, clean_from:]))
    assert not np.all(np.isfinite(want)) and np.all(np.isfinite(want[:, clean])) and _finite_states(want_state)

    def same(p, y, what):
        assert y.shape == want.shape, what
        _same_finite(y, want, what)
        got = TGP._states(p.stretch, p.resampler, nch)
        assert len(got) == len(want_state) and all(np.array_equal(a, b) for a, b in zip(got, want_state)), what

    for cuts in ([FRAMES], [1, 7, FRAMES - 8], [20, 2, 39], [3] * 20 + [1]):
        p = phaze_amd.PitchStretch(N, FLOOR, HS, max_channels=nch, max_frames=4, channels_per_group=G)
        parts, f0 = [], 0
        for nf in cuts:
            parts.append(p.process_hops(x[:, at[f0]:at[f0 + nf]], None if hops is None else hops[f0:f0 + nf], None if resets is None else resets[f0:f0 + nf]))
            f0 += nf
        same(p, np.concatenate(parts, axis=1), cuts)
        p.close()
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
    p.set_stream(None)
    for h in (p, ts, rs):
        h.close()


# ---- 4. the analysis paths ---------------------------------------------------------------------------------------------------------------------------

def test_process_tuned_with_a_nan_plans_the_frames_that_hold_it_as_unvoiced():
    """The 452 Hz two-harmonic tone of tests/test_gpu_f0.py with one NaN mid-signal.  The tracker's frames that hold it give zero records, which the
    planner reads as unvoiced; the hops are the model's plan of the model's records, the output is process(x, hops) bit for bit and is finite outside
    the reach of the NaN: before the first frame of the row that holds it, and from the stretch's clean_from plus the resampler's T - 1 on."""
    import phaze_amd
    N, HS, LO, HI = 1024, 256, 128, 512
    n, s = 24000, 12345
    x = TGF._two_harmonics(452.0, n)
    x[s] = np.nan
    g = phaze_amd.PitchGlide(N, HS, LO, HI, max_frames=96)
    y, hops = g.process_tuned(x, FM.SAMPLE_RATE)
    recs = FM.track(x, N, HS, 32, N)
    holding = np.array([m * HS <= s < m * HS + 2 * N for m in range(recs.shape[0])])
    assert holding.sum() == 2 * N // HS and np.all(recs[holding] == 0) and np.all(recs[~holding][:, 0] > 0)
    want_hops, _ = FM.tune_plan(recs, HS, N, FM.SAMPLE_RATE, HS, LO, HI, n)
    assert np.array_equal(hops, want_hops) and hops.dtype == np.int32
    total = int(hops.sum())
    g.reset()
    z = g.process(x[:total], hops)
    assert y.shape == z.shape == (total,) and np.array_equal(np.isfinite(y), np.isfinite(z)) and np.array_equal(_bits(y)[np.isfinite(y)], _bits(z)[np.isfinite(z)])
    at = np.concatenate([[0], np.cumsum(hops.astype(np.int64))])
    T = g.resampler.taps
    n_out = np.concatenate([b * HS + (np.arange(c, dtype=np.int64) * HS) // c for b, c in enumerate(hops.tolist())])
    first = int(np.flatnonzero(at[1:] > s)[0])                                # the first frame whose window holds s: its output starts at first * hs
    outside = (n_out < first * HS) | (n_out - (T - 1) >= _stretched_clean_from(at, N, HS, s))
    print(f"tuned with a NaN: {int((~np.isfinite(y)).sum())} non-finite outputs, {int((~outside).sum())} inside the derived reach")
    assert not np.all(np.isfinite(y)) and outside.sum() > total // 2 and np.all(np.isfinite(y[outside]))
    g.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("N,ha", [(256, 100), (1024, 256)])
def test_onset_strength_counts_nothing_on_the_frames_a_bad_sample_reaches(N, ha, bad):
    """RULE (include/phaze_amd.h, pv_onset_strength): c_m = 0 on every frame whose window holds a non-finite sample and on the first frame after
    those, whose previous magnitudes are not finite; every other frame is untouched.  Elsewhere the doubt rule of tests/test_gpu_transient.py."""
    import phaze_amd
    n = 40 * N
    x = TM.class_signal("bursts_tones", n, N, [7 * N + 137, 17 * N + 901, 29 * N + 333], seed=3).copy()
    s = 17 * N + 950                                                          # inside a burst: the clean signal counts onsets around here
    x[s] = bad
    T = n // ha
    m = np.arange(T)
    reached = ((m + 1) * ha - N <= s) & (s < (m + 1) * ha)                    # frame m's window is [(m + 1) ha - N, (m + 1) ha)
    reached[int(np.flatnonzero(reached)[-1]) + 1] = True
    with np.errstate(invalid="ignore"):
        c, d = TM.onset_strength(x, N, ha)
    assert np.all(c[reached] == 0) and np.all(d[reached] == 0)                # the model follows the rule
    ts = phaze_amd.TimeStretch(N, ha, N // 4, max_channels=1, max_frames=1)
    got = ts.onset_strength(x)[0]
    ts.close()
    assert got.shape == c.shape and np.all(got[reached] == 0), got[reached].tolist()
    assert np.all(np.abs(got.astype(np.int64) - c) <= d), np.nonzero(np.abs(got - c) > d)[0][:8]
    assert c[~reached].max() > 0.2 * (N // 2) and int(d.sum()) <= 0.01 * T     # the other frames still see the bursts; the doubt stays a rarity


# ---- 5. scaling by a power of two is exact -----------------------------------------------------------------------------------------------------------

def _scaled(x, k):
    y = np.ldexp(x, k)
    assert y.dtype == np.float32 and np.array_equal(np.ldexp(y, -k), x)                        # exact: nothing under- or overflows in the input
    return y


@pytest.mark.parametrize("name", ["320-alternate", "64-extremes"])
def test_vari_output_scales_exactly_with_a_power_of_two(name):
    """The weights do not depend on the signal, so every product, partial sum and the quotient of 2^k x is 2^k times that of x as long as none leaves
    the normal range.  Checked on the model, not assumed: the smallest non-zero |w_i x_i| times 2^-40 is normal, the largest sum |w_i x_i| / |D|
    times 2^40 is finite."""
    k = TGV.case(name)
    B, counts, x = k["B"], k["counts"], k["x"]
    m = VM.VariModel(B, k["lo"], k["hi"])
    smallest, largest = np.inf, 0.0
    for b in sorted(set(counts.tolist())):                                                     # one block per distinct count holds every weight row
        w, _ = VM.weights(B, b, (np.arange(b) * B) % b, m.W, m.table)
        aw = np.abs(w[w != 0.0])
        smallest, largest = min(smallest, float(aw.min())), max(largest, float(np.abs(w).sum(axis=1).max() / np.abs(w.sum(axis=1)).min()))
    ax = np.abs(x[x != 0.0]).astype(np.float64)
    print(f"{name}: smallest |w| {smallest:.3e}, smallest |x| {ax.min():.3e}, largest sum |w| / D {largest:.3f}")
    assert smallest * ax.min() * 2.0 ** -40 >= 2.0 ** -126 and largest * ax.max() * 2.0 ** 40 < 2.0 ** 127
    rs = TGV._make(k, TGV.NCH, counts.size)
    base = rs.process(x, counts)
    for e in (-40, 40):
        rs.reset()
        y = rs.process(_scaled(x, e), counts)
        assert np.array_equal(_bits(y), _bits(np.ldexp(base, e))), e
    rs.close()


@pytest.mark.parametrize("up,down", RESAMPLE_RATIOS)
def test_resample_output_scales_exactly_with_a_power_of_two(up, down):
    import phaze_amd
    k = TGR.case(up, down)
    x, taps = k["x"], np.abs(np.asarray(k["taps"], np.float64))
    ax = np.abs(x[x != 0.0]).astype(np.float64)
    print(f"{up}/{down}: smallest non-zero |h| {taps[taps > 0].min():.3e}, smallest |x| {ax.min():.3e}, largest sum |h x| {k['b'].max():.3f}")
    assert taps[taps > 0].min() * ax.min() * 2.0 ** -40 >= 2.0 ** -126 and k["b"].max() * 2.0 ** 40 < 2.0 ** 127
    rs = phaze_amd.Resampler(up, down, max_channels=TGR.NCH, max_samples=x.shape[1])
    base = rs.process(x)
    for e in (-40, 40):
        rs.reset()
        y = rs.process(_scaled(x, e))
        assert np.array_equal(_bits(y), _bits(np.ldexp(base, e))), e
    rs.close()


@pytest.mark.parametrize("shape", [TGF.SHAPES[0], TGF.SHAPES[3]], ids=[TGF.IDS[0], TGF.IDS[3]])
def test_f0_records_do_not_move_with_a_power_of_two(shape):
    """The records are an exact function of the block-scaled integers round(x 2^(11 - e)), e the exponent of the frame's peak: 2^k x has the same
    integers.  Up to a peak of FLT_MAX, the largest exponent there is (the subnormal end is in tests/test_gpu_f0.py)."""
    import phaze_amd
    W, hop, lo, ML, _ = shape
    F = 3
    x, want = TGF._model("tone", (W, hop, lo, ML, F))
    assert np.all(want[:, 0] > 0)
    top = np.ldexp(FM.tone("harm", ML / 3.3, x.size, float(np.nextafter(np.float32(1), np.float32(0)))), 128)
    assert top.dtype == np.float32 and np.all(np.isfinite(top)) and np.max(np.abs(top)) == np.finfo(np.float32).max
    rows = [x] + [_scaled(x, e) for e in (-100, -20, 20, 100)] + [top]
    trk = phaze_amd.F0Tracker(W, hop, lo, ML, max_channels=len(rows), max_frames=F)
    got = trk.track(np.stack(rows))
    dev = TGF._device_track(trk, np.stack(rows), F)
    trk.close()
    for c in range(5):
        assert np.array_equal(got[c], want) and np.array_equal(dev[c], want), c
    want_top = FM.track(top, W, hop, lo, ML)
    assert np.all(want_top[:, 0] > 0) and np.array_equal(got[5], want_top) and np.array_equal(dev[5], want_top)
