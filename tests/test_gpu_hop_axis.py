"""The pitch shifter along the hop axis: every power-of-two hop from 2 to N, N = 256 ... 8192, against the CPU oracle.  GPU box.

Most of the suite runs R = N / hop <= 16.  Small hops take other code: the LDS overlap-add ring of pv_wg_kernel (S_ROWS = 0, run-time R) at
N = 2048 / 4096 / 8192, pv_chain_kernel at N <= 1024, chunk halos of R - 1 frames that reach back before hop 0, calls shorter than R (the
history written at the end of a call comes partly from the previous state) and rotations tmod = (t0 + m hop) mod N that take N / hop values.
This file pins the dispatch of every cell, compares every cell with the oracle, and checks chunking, call splitting, streaming, the debug tap,
state hand-over and the generic kernel's LDS boundary at these shapes.
"""
import functools

import numpy as np
import pytest

import oracle_lib
import signals as S
from test_gpu_parity import REGRESSION_RMS

pytestmark = pytest.mark.gpu

PV_ERR_UNSUPPORTED = 3
GENERIC, STREAM_COPY, STREAM_EVENT_WAIT, PINNED, RESIDENT, NO_HDP = 1, 2, 8, 16, 32, 64

SIZES = (256, 512, 1024, 2048, 4096, 8192)
CELLS = [(N, N >> k) for N in SIZES for k in range(N.bit_length() - 1)]          # hop = N, N/2, ..., 2: 63 cells
SMALL = [(N, h) for N, h in CELLS if h < N // 8]                                   # R >= 16

# which kernel runs each cell, written out (not derived from the library): a silent change of dispatch fails test_dispatch_table
DISPATCH = {
    256: [(2, 256, "pv_chain_kernel")],
    512: [(2, 512, "pv_chain_kernel")],
    1024: [(2, 64, "pv_chain_kernel"), (128, 1024, "pv_wave_kernel_1024")],
    2048: [(2, 64, "pv_wg_kernel"), (128, 2048, "pv_wave2k_kernel")],
    4096: [(2, 256, "pv_wg_kernel"), (512, 4096, "pv_wg16_kernel")],
    8192: [(2, 512, "pv_wg_kernel"), (1024, 8192, "pv_wg16_kernel")],
}
LDS_CU = 160 * 1024
STATIC_LDS = 256

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for name, (err, where) in sorted(WORST.items()):
        print(f"\nhop axis: worst rms vs oracle on {name}: {err:.3e} ({where})")


def _expected(N, hop):
    for lo, hi, name in DISPATCH[N]:
        if lo <= hop <= hi:
            return name
    raise KeyError((N, hop))


def _pv(fft, hop, nch, T=1, **kw):
    import phaze_amd
    return phaze_amd.PhaseVocoder(fft_size=fft, hop_size=hop, max_channels=nch, max_hops=T, **kw)


def _shape(N, hop):
    R = N // hop
    return R, max(2 * R + 24, 48), (2 if R <= 512 else 1)


def _signal(nch, n, stream=0):
    """channel 0 tonal; channel 1 noise plus a strong component just below Nyquist (the last region reads the above-Nyquist residue)."""
    chans = [S.make_signal("tonal", 0, n, stream=stream)]
    if nch > 1:
        i = np.arange(n, dtype=np.float64)
        hi = 0.3 * np.sin(2 * np.pi * (0.488 * i)) + 0.05 * np.sin(2 * np.pi * 0.031 * i)
        chans.append((hi + S.make_signal("noise", 1, n, stream=stream).astype(np.float64) / 256).astype(np.float32))
    return np.stack(chans)


def _schedule(kind, T):
    if kind == "sweep":                                    # crosses f = 0.75 and f = 1: both scatters, both residue forms
        return (0.35 + (2.2 - 0.35) * np.arange(T) / max(T - 1, 1)).astype(np.float32)
    vals = np.array([0.3, 0.5, 0.75, 1.0, 1.5, 2.0], np.float32)                   # k-rate steps, each value twice per call
    return vals[(np.arange(T) // max(1, T // 12)) % 6]


@functools.lru_cache(maxsize=None)
def _case(N, hop, kind):
    """(x, pitch, oracle output) of a cell; cached: several tests compare with the same oracle run."""
    R, T, nch = _shape(N, hop)
    x = _signal(nch, T * hop)
    p = _schedule(kind, T)
    yo = oracle_lib.Oracle(N, hop, nch).process_planar(x, p)
    return x, p, yo


def _first_bad_hop(d, hop, tol):
    per_hop = np.sqrt(np.mean(d.reshape(d.shape[0], -1, hop) ** 2, axis=(0, 2)))
    bad = np.flatnonzero(~(per_hop < tol))
    return int(bad[0]) if bad.size else int(np.argmax(per_hop))


def _check_oracle(y, yo, hop, name, what):
    d = y.astype(np.float64) - yo
    if not np.all(np.isfinite(y)):
        pytest.fail(f"{what} kernel={name}: non-finite output from hop {_first_bad_hop(np.nan_to_num(d, nan=1.0, posinf=1.0, neginf=1.0), hop, REGRESSION_RMS)}")
    err = S.rms(d)
    if not err < REGRESSION_RMS:
        pytest.fail(f"{what} kernel={name}: rms {err:.3e} >= {REGRESSION_RMS:.0e}, first bad hop {_first_bad_hop(d, hop, REGRESSION_RMS)}")
    if err >= WORST.get(name, (-1.0, ""))[0]:
        WORST[name] = (err, what)
    return err


def _same_bits(a, b, hop, what):
    diff = np.any(a.view(np.uint32) != b.view(np.uint32), axis=0)
    if diff.any():
        i = int(np.flatnonzero(diff)[0])
        pytest.fail(f"{what}: first differing sample {i} (hop {i // hop}) of {int(diff.sum())}")


@pytest.mark.parametrize("fft,hop", CELLS, ids=[f"{N}-{h}" for N, h in CELLS])
def test_dispatch_table(fft, hop):
    pv = _pv(fft, hop, 1)
    info = pv.info()
    pv.close()
    name = _expected(fft, hop)
    assert info["kernel_name"] == name, (fft, hop, info["kernel_name"])
    assert info["overlaps"] == fft // hop
    if name in ("pv_chain_kernel", "pv_wg_kernel"):                   # the LDS-bound kernels: dynamic + static LDS of one workgroup fits a CU
        assert 0 < info["lds_bytes_per_workgroup"] and info["lds_bytes_per_workgroup"] + STATIC_LDS <= LDS_CU, info
    if name == "pv_wg_kernel":
        assert info["threads_per_workgroup"] == fft // 16                # eight elements per thread, G = N / 1024 waves


@pytest.mark.parametrize("kind", ["sweep", "steps"])
@pytest.mark.parametrize("fft,hop", CELLS, ids=[f"{N}-{h}" for N, h in CELLS])
def test_oracle_parity_every_cell(fft, hop, kind):
    R, T, nch = _shape(fft, hop)
    x, p, yo = _case(fft, hop, kind)
    pv = _pv(fft, hop, nch, T)
    y = pv.process_batch(x, p)
    name = pv.info()["kernel_name"]
    assert pv.time_cursor == T * hop
    pv.close()
    _check_oracle(y, yo, hop, name, f"{fft}/{hop} {kind} T={T} nch={nch}")


@pytest.mark.parametrize("fft,hop", SMALL, ids=[f"{N}-{h}" for N, h in SMALL])
def test_chunking_and_call_splits_are_bit_exact(fft, hop):
    """One chain per channel == frame-parallel chunks of R - 1, R, R + 1 frames (chunk 1 of R - 1 frames starts inside the first R - 1 hops:
    its halo reaches before hop 0 and it takes the carried accumulator) == calls of 1, R - 1, R + 1 hops and the rest (calls shorter than R), unchunked
    and in chunks of R - 1 frames."""
    R, T, nch = _shape(fft, hop)
    x, p, _ = _case(fft, hop, "sweep")
    pv = _pv(fft, hop, nch, T, frames_per_chunk=T)
    ref = pv.process_batch(x, p)
    pv.close()
    for F in (R - 1, R, R + 1, 0) + ((1, 3) if R <= 64 else ()):
        pv = _pv(fft, hop, nch, T, frames_per_chunk=F)
        y = pv.process_batch(x, p)
        pv.close()
        _same_bits(y, ref, hop, f"{fft}/{hop} frames_per_chunk={F}")
    cuts = np.cumsum([0, 1, R - 1, R + 1, T - 2 * R - 1])
    for F in (0, R - 1):                                   # F = R - 1: chunk 1 of the third call starts its halo at the call's first hop (carried accumulator)
        pv = _pv(fft, hop, nch, T, frames_per_chunk=F)
        parts = [pv.process_batch(x[:, a * hop:b * hop], p[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        assert pv.time_cursor == T * hop
        pv.close()
        _same_bits(np.concatenate(parts, axis=1), ref, hop, f"{fft}/{hop} calls of 1, R - 1, R + 1, rest, frames_per_chunk={F}")


GENERIC_CELLS = [(N, h) for N, h in SMALL if N >= 2048]


@pytest.mark.parametrize("fft,hop", GENERIC_CELLS, ids=[f"{N}-{h}" for N, h in GENERIC_CELLS])
def test_generic_kernel_is_a_second_implementation(fft, hop):
    """PV_FLAG_GENERIC_KERNEL runs pv_chain_kernel where the default runs the LDS ring (pv_wave2k_kernel at 2048/128).  Its LDS (16 (N/2 + 1) + 8 N + 4 (N - hop) + masks) draws a
    boundary at N = 8192: hop 512 needs 162 848 B of the 163 328 B the library allows it and runs; hop <= 256 is refused, the default handle is not."""
    import phaze_amd
    R, T, nch = _shape(fft, hop)
    if fft == 8192 and hop <= 256:
        with pytest.raises(phaze_amd.PvError) as e:
            _pv(fft, hop, nch, T, flags=GENERIC)
        assert e.value.status == PV_ERR_UNSUPPORTED and "LDS" in str(e.value), str(e.value)
        pv = _pv(fft, hop, nch, T)
        assert pv.info()["kernel_name"] == "pv_wg_kernel"
        pv.close()
        return
    x, p, yo = _case(fft, hop, "sweep")
    outs = {}
    for flags in (0, GENERIC):
        pv = _pv(fft, hop, nch, T, flags=flags)
        info = pv.info()
        outs[flags] = pv.process_batch(x, p)
        pv.close()
        assert info["kernel_name"] == ("pv_chain_kernel" if flags else _expected(fft, hop)), info["kernel_name"]
        if flags and fft == 8192:
            assert info["lds_bytes_per_workgroup"] == 162848
        _check_oracle(outs[flags], yo, hop, info["kernel_name"], f"{fft}/{hop} sweep T={T} nch={nch} flags={flags}")
    assert S.rms(outs[0].astype(np.float64) - outs[GENERIC]) < 1e-7


STREAM_CELLS = [(1024, 16), (2048, 32), (4096, 64), (8192, 256), (8192, 2)]


def _stream(fft, hop, nch, flags, x, p):
    pv = _pv(fft, hop, nch, 1, flags=flags)
    T = len(p)
    y = np.empty((nch, T * hop), np.float32)
    for m in range(T):
        blk = [np.ascontiguousarray(x[c, m * hop:(m + 1) * hop]) for c in range(nch)]
        outs = [np.zeros(hop, np.float32) for _ in range(nch)]
        assert pv.process([blk], [outs], {"pitchFactor": p[m:m + 1]}) is True
        for c in range(nch):
            y[c, m * hop:(m + 1) * hop] = outs[c]
    name = pv.info()["kernel_name"]
    pv.close()
    return y, name


@pytest.mark.parametrize("fft,hop", STREAM_CELLS, ids=[f"{N}-{h}" for N, h in STREAM_CELLS])
def test_streaming_quanta_on_the_ring_and_generic_kernels(fft, hop):
    """pv_process one hop at a time in every hand-over form: BAR writes (0), pinned input (16), copy nodes + stream wait (2|8), no HDP flush (64),
    and the resident flag (32), which these shapes do not support: accepted, ignored, same bits.  All == process_batch in one-hop calls == the oracle."""
    R, T, nch = _shape(fft, hop)
    T = max(T, 600)
    x = _signal(nch, T * hop, stream=5)
    p = _schedule("steps", T)
    base, name = _stream(fft, hop, nch, 0, x, p)
    assert name == _expected(fft, hop)
    for flags in (PINNED, STREAM_COPY | STREAM_EVENT_WAIT, NO_HDP, RESIDENT):
        y, nm = _stream(fft, hop, nch, flags, x, p)
        assert nm == name
        _same_bits(y, base, hop, f"{fft}/{hop} flags={flags}")
    pv = _pv(fft, hop, nch, 1)
    y = np.concatenate([pv.process_batch(x[:, m * hop:(m + 1) * hop], p[m:m + 1]) for m in range(T)], axis=1)
    pv.close()
    _same_bits(y, base, hop, f"{fft}/{hop} process_batch of one hop per call")
    yo = oracle_lib.Oracle(fft, hop, nch).process_planar(x, p)
    _check_oracle(base, yo, hop, name, f"{fft}/{hop} streamed T={T} nch={nch}")


TAP_CELLS = [(1024, 32), (2048, 16), (4096, 64), (8192, 512), (8192, 2)]


@pytest.mark.parametrize("fft,hop", TAP_CELLS, ids=[f"{N}-{h}" for N, h in TAP_CELLS])
def test_intermediates_match_the_oracle(fft, hop):
    """debug_frame (the tap instance of the kernel the handle runs) against Oracle.debug(): fp64 forward spectrum, peak set, magnitudes and the
    shifted spectrum, at the first frames, the frames around hop R and one later, for the tonal channel and the near-Nyquist one."""
    R, T, nch = _shape(fft, hop)
    frames = sorted({1, R - 1, R, R + 1, R + 7})
    T = frames[-1] + 1
    x = _signal(2, T * hop, stream=6)
    p = _schedule("steps", T)
    p[R] = 0.7                                             # f < 0.75 on the first frame after hop R: the residue is rebuilt
    H = fft // 2 + 1
    for c in range(2):
        pv = _pv(fft, hop, 1, T)
        assert pv.info()["kernel_name"] == _expected(fft, hop)
        o = oracle_lib.Oracle(fft, hop, 1)
        pos = 0
        for m in frames:
            if m > pos:
                pv.process_batch(x[c:c + 1, pos * hop:m * hop], p[pos:m])
                o.process_planar(x[c:c + 1, pos * hop:m * hop], p[pos:m])
            blk = x[c, m * hop:(m + 1) * hop]
            got = pv.debug_frame(0, blk, p[m])
            o.process([blk], p[m])
            ref = o.debug()
            pv.process_batch(blk[None], p[m:m + 1])
            pos = m + 1
            what = f"{fft}/{hop} ch {c} frame {m} f={p[m]}"
            Xr = ref["X"][0::2] + 1j * ref["X"][1::2]
            Xg = got["X"][0::2] + 1j * got["X"][1::2]
            scale = np.max(np.abs(Xr))
            assert scale > 0, what
            assert np.max(np.abs(Xg[:H] - Xr[:H])) < 1e-12 * scale, f"fp64 forward spectrum, {what}"
            assert np.array_equal(np.nonzero(got["flags"])[0], ref["peaks"]), f"peak set, {what}"
            np.testing.assert_allclose(got["mag"], ref["mag"], rtol=1e-6, err_msg=what)
            Yr = (ref["Y"][0::2] + 1j * ref["Y"][1::2])[:H]
            Yg = got["Y"][0::2] + 1j * got["Y"][1::2]
            assert np.max(np.abs(Yg[1:-1] - Yr[1:-1])) < 2e-6 * scale, f"shifted spectrum, {what}"
            if np.any(Xg[H:] != 0) and len(ref["peaks"]):   # residue rebuilt for this frame: compare where the reference reads it
                lp = int(ref["peaks"][-1])
                xs = lp * float(np.float32(p[m]))
                d = int(np.floor(xs) + (1 if xs - np.floor(xs) >= 0.5 else 0)) - lp
                if d < 0:
                    hi = min(fft, H - d)
                    assert np.max(np.abs(Xg[H:hi] - Xr[H:hi])) < 2e-6 * scale, f"above-Nyquist residue, {what}"
        pv.close()
        o.close()


HANDOVER_CELLS = [(2048, 8), (4096, 32), (8192, 4)]


@pytest.mark.parametrize("fft,hop", HANDOVER_CELLS, ids=[f"{N}-{h}" for N, h in HANDOVER_CELLS])
def test_export_import_at_small_hops(fft, hop):
    """A stream handed to a fresh handle after k hops (k = 1, k < R, k > R) continues with the bits of the uninterrupted run."""
    R, T, nch = _shape(fft, hop)
    x = _signal(nch, T * hop, stream=7)
    p = _schedule("sweep", T)
    pv = _pv(fft, hop, nch, T)
    ref = pv.process_batch(x, p)
    pv.close()
    for k in (1, R - 3, R + 5):
        a = _pv(fft, hop, nch, T)
        head = a.process_batch(x[:, :k * hop], p[:k])
        states = [a.export_state(c) for c in range(nch)]
        a.close()
        assert all(tc == k * hop for _, _, tc in states)
        b = _pv(fft, hop, nch, T)
        for c, (hist, acc, tc) in enumerate(states):
            b.import_state(c, hist, acc, tc)
        tail = b.process_batch(x[:, k * hop:], p[k:])
        b.close()
        _same_bits(np.concatenate([head, tail], axis=1), ref, hop, f"{fft}/{hop} handed over after {k} hops")


def _fuzz_case(rng):
    log2n = int(rng.integers(8, 14))
    N = 1 << log2n
    hop = N >> int(rng.integers(4, log2n))                 # R = 16 ... N/2
    R = N // hop
    nch = int(rng.integers(1, 4))
    tmax = max(4, min(2 * R + 24, (1 << 24) // (N * nch)))    # bounds the oracle's work per case
    T = int(rng.integers(1, tmax + 1))
    kind = ["noise", "tonal"][int(rng.integers(0, 2))]
    mode = int(rng.integers(0, 4))                         # the pitch classes of test_gpu_fuzz
    if mode == 0:
        p = rng.uniform(0.3, 3.0, size=T)
    elif mode == 1:
        p = np.full(T, rng.choice([0.5, 0.75, 1.0, 1.5, 2.0, 0.33, 2.5]))
    elif mode == 2:
        p = rng.uniform(0.05, 0.6, size=T)
    else:
        p = rng.choice([0.0, -1.0, 0.8, 1.2, np.nan, np.inf, -np.inf, 100.0, 1e-3], size=T)
    return N, hop, R, nch, T, kind, p.astype(np.float32)


@pytest.mark.parametrize("seed", range(10))
def test_fuzz_small_hops_against_oracle(seed):
    """Seeded: random N, hops with R >= 16 down to 2, channel counts, chunk lengths around R, call splits around R and pitch schedules."""
    rng = np.random.default_rng(4321 + seed)
    for _ in range(20):
        N, hop, R, nch, T, kind, p = _fuzz_case(rng)
        x = np.stack([S.make_signal(kind, c, T * hop, stream=seed) for c in range(nch)])
        fpc = int(rng.choice([0, 0, R - 1, R, R + 1] + ([1, 3] if R <= 64 else [])))     # (a chunk of F frames computes F + R - 1)
        pv = _pv(N, hop, nch, T, frames_per_chunk=fpc)
        parts, pos = [], 0
        while pos < T:
            n = min(T - pos, int(rng.choice([1, R - 1, R + 1, int(rng.integers(1, T - pos + 1))])))
            parts.append(pv.process_batch(x[:, pos * hop:(pos + n) * hop], p[pos:pos + n]))
            pos += n
        y = np.concatenate(parts, axis=1)
        name = pv.info()["kernel_name"]
        pv.close()
        yo = oracle_lib.Oracle(N, hop, nch).process_planar(x, p)
        _check_oracle(y, yo, hop, name, f"fuzz seed {seed}: {N}/{hop} nch={nch} T={T} {kind} fpc={fpc}")
