"""Where a long stream puts a PhaseVocoder handle: the 16-bit sequence number of the resident streaming protocol wrapping around, and a time cursor far
from zero -- past 2^24 (where fp32 stops counting samples), across 2^31 and 2^32, up to 2^62.  GPU box.

1. The wrap.  65535 + 2 P + 40 quanta through pv_process on every resident kernel.  Nobody allocates 66000 hops: input and pitch row repeat with a period
   of P quanta, P * hop a multiple of N and P >= 4 R.  A quantum's bits depend on its N-sample window, on the R - 1 frames pending in the accumulator, on
   its pitchFactor and on the cursor mod N only, so from quantum 2 P on quantum m must equal quantum P + (m mod P) of the record -- the first 2 P quanta of
   the same stream on a launch-form handle -- bit for bit.  A stale, repeated or skipped frame fails at a named quantum.
2. The cursor.  A shift of the time cursor by a multiple of N must not change one bit, in any call form, on any kernel, and the cursor must read back exactly.
3. Bit identity under a shift cannot see an error that depends on cursor mod N only: one comparison against the oracle at 2^26 + 3 hop, at the suite's gate.
   (Why 2^26 and not further: tests/test_rotation_error.py -- beyond about 2^27.3 samples the ORACLE's own rotation is off by more than 1e-7 rad.)

pv_info does not say whether a handle runs the resident form; the cases below are shapes for which pv_create's rule (family_resident_supported, at most 64
channel slots) puts PV_FLAG_PERSISTENT_STREAM on a resident kernel, and the kernel itself is confirmed by name.
"""
import ctypes as C
import time

import numpy as np
import pytest

import oracle_lib
import signals as S

pytestmark = pytest.mark.gpu

GENERIC, WG, PINNED, RESIDENT, HOST_CHANNELS, FP64 = 1, 4, 16, 32, 128, 256
FPT = C.POINTER(C.c_float)
P = 64                                         # period of the input and the pitch row, in quanta
CYCLE = 65535                                  # sequence numbers 1 .. 0xFFFF: quantum m (from 0) carries 1 + m mod 65535


def _pv(**kw):
    import phaze_amd
    return phaze_amd.PhaseVocoder(**kw)


class _Periodic:
    """One stream of period P quanta fed through the raw pv_process: every pointer array and pitch value is allocated once."""

    def __init__(self, fft, hop, nch, seed):
        assert (P * hop) % fft == 0 and P >= 4 * (fft // hop)
        rng = np.random.default_rng(seed)
        self.hop, self.nch = hop, nch
        self.x = (rng.standard_normal((nch, P, hop)) * 0.2).astype(np.float32)
        self.pitch = [C.c_float(float(v)) for v in rng.permutation(np.linspace(0.55, 1.9, P)).astype(np.float32)]     # both scatter routes, every residue
        self.out = np.zeros((nch, hop), np.float32)
        self.ips = {n: [(FPT * n)(*[self.x[c, i].ctypes.data_as(FPT) for c in range(n)]) for i in range(P)] for n in range(1, nch + 1)}
        self.ops = {n: (FPT * n)(*[self.out[c].ctypes.data_as(FPT) for c in range(n)]) for n in range(1, nch + 1)}

    def quantum(self, pv, m, nch=None):
        """Quantum m of the stream on `pv`: the bytes of its nch output hops.  Stops the test at an error status (nothing is retried)."""
        n = self.nch if nch is None else nch
        rc = pv._L.pv_process(pv._h, self.ips[n][m % P], self.ops[n], n, self.hop, self.pitch[m % P])
        if rc != 0:
            pytest.fail(f"quantum {m} (sequence number {1 + m % CYCLE}): pv_process returned {rc}: {pv._L.pv_last_error(pv._h).decode()}")
        return self.out[:n].tobytes()


_RECORDS = {}


def _record(fft, hop, kernel_flags):
    """(stream, the bytes of its first 2 P quanta on a launch-form handle that reads pinned memory): computed once per shape, shared, never written."""
    key = (fft, hop, kernel_flags)
    if key not in _RECORDS:
        s = _Periodic(fft, hop, 1, fft + hop)
        pv = _pv(fft_size=fft, hop_size=hop, max_channels=1, max_hops=1, flags=PINNED | kernel_flags)
        rec = [s.quantum(pv, m) for m in range(2 * P)]
        pv.close()
        # the premise of the periodic reference, on the record itself: the warmed-up stream repeats (quanta P/2 .. P-1 against P + P/2 .. 2 P - 1)
        assert rec[P // 2:P] == rec[P + P // 2:] and len(set(rec[P:])) == P
        _RECORDS[key] = (s, rec)
    return _RECORDS[key]


WRAP_CASES = [("pv_wave_kernel_1024", 1024, 256, RESIDENT), ("pv_wave2k_kernel", 2048, 512, RESIDENT), ("pv_wg16_kernel", 4096, 1024, RESIDENT),
              ("pv_wg16_kernel", 8192, 2048, RESIDENT), ("pv_wg_kernel", 8192, 2048, RESIDENT | WG), ("pv_wave_kernel_1024", 1024, 256, RESIDENT | PINNED)]
# 80 ms: every resident wave has left (idle time-out ~50 ms); 35 ms: inside the window in which they leave one by one.  In front of quantum 65534 (restart
# behind 0xFFFE, then the last number of the cycle), 65535 (restart behind 0xFFFF: the first quantum of the new cycle carries 1, and a restart from
# pv_process_end would pass 1 - 1 = 0) and 65536 (restart behind 1)
WRAP_PAUSES = {CYCLE - 1: 0.08, CYCLE: 0.035, CYCLE + 1: 0.08}


@pytest.mark.parametrize("pauses", [{}, WRAP_PAUSES], ids=["running", "paused"])
@pytest.mark.parametrize("kernel,fft,hop,flags", WRAP_CASES, ids=[f"{k}-{n}-{h}-{f}" for k, n, h, f in WRAP_CASES])
def test_the_sequence_number_wraps_without_a_stale_or_repeated_quantum(kernel, fft, hop, flags, pauses):
    """Every resident kernel at its smallest streaming shape, mono: 65703 quanta, so the number passes 0xFFFF -> 1 once, in running waves and (paused) across
    restarts on either side of it.  The test stops at the first quantum that returns an error (the library's own bounded wait) or differs.
    Measured on an MI355X, running / paused (the three pauses add 0.2 s), against 65703 x the mean per-quantum latency of bench_latency.py on the parent commit
    (same form and shape, mono; the gate is 3 x that for the ctypes call and the comparison):
        pv_wave_kernel_1024 1024/256            0.65 / 0.84 s    (8.9 us: 0.59 s)
        pv_wave2k_kernel    2048/512            1.10 / 1.29 s    (15.5 us: 1.02 s)
        pv_wg16_kernel      4096/1024           1.19 / 1.39 s    (16.0 us: 1.05 s)
        pv_wg16_kernel      8192/2048           1.78 / 2.00 s    (23.8 us: 1.56 s)
        pv_wg_kernel        8192/2048           1.42 / 1.60 s    (19.0 us: 1.25 s)
        pv_wave_kernel_1024 1024/256, pinned    0.76 / 0.95 s    (10.5 us: 0.69 s)"""
    s, rec = _record(fft, hop, flags & WG)
    pv = _pv(fft_size=fft, hop_size=hop, max_channels=1, max_hops=1, flags=flags)
    assert pv.info()["kernel_name"] == kernel
    total = CYCLE + 2 * P + 40
    t0 = time.perf_counter()
    for m in range(total):
        if m in pauses:
            time.sleep(pauses[m])
        got = s.quantum(pv, m)
        if got != (rec[m] if m < 2 * P else rec[P + m % P]):
            same_as = [k for k in range(P, 2 * P) if rec[k] == got]
            pytest.fail(f"quantum {m} (sequence number {1 + m % CYCLE}) differs from the record" + (f": it is quantum {same_as[0]} (mod {P}) of it" if same_as else ""))
    dt = time.perf_counter() - t0
    assert pv.time_cursor == total * hop
    pv.close()
    print(f"wrap {kernel} {fft}/{hop} flags {flags} {'paused' if pauses else 'running'}: {total} quanta in {dt:.2f} s ({dt / total * 1e6:.1f} us per quantum)")


@pytest.mark.parametrize("sat_out", [CYCLE - 1, CYCLE])
def test_a_channel_slot_that_sits_out_a_whole_cycle_is_waited_for(sat_out):
    """Can a slot sit out a whole cycle of sequence numbers and still hold a completion word equal to the live number, with no restart in between?
    By reading: yes.  With PV_FLAG_HOST_CHANNEL_BOOKKEEPING pv_process accepts a changed channel count without resetting anything, and nothing makes the
    host call pv_reset_channels_part in between (the Python and Node hosts do, which stops the waves; a host that wants the slot's state kept must not).
    The resident waves then stay.  A slot that is not part of a quantum carries its state across the flip and stores NO completion word, so its word keeps
    the number of the last quantum it took part in.  The numbers run 1 .. 65535, so after 65534 quanta without it the next quantum carries that very number
    again (65535 quanta, the figure the comment in pv_capi.hip gave, is one too many: 0 is skipped), and pv_process_end took the slot for complete without
    waiting for its wave.  pv_process_begin now clears the words whenever the numbers start over.
    What this test can and cannot show: the waves of a quantum finish within a microsecond of each other and the host only looks at slot 1 after slot 0's word
    has crossed PCIe, so the missing wait did not change an output on the MI355X -- this test passed before the fix as well.  It pins what must hold either way:
    two channels, then one for 65534 / 65535 quanta with the waves resident throughout, then two again, and the regained channel continues bit for bit like
    on a launch-form handle that sat out as many quanta mod P (same window, same pending frames, same cursor mod N)."""
    fft, hop, back = 1024, 256, 12
    s = _Periodic(fft, hop, 2, 77)
    short = P + sat_out % P
    ref = _pv(fft_size=fft, hop_size=hop, max_channels=2, max_hops=1, flags=PINNED | HOST_CHANNELS)
    for m in range(P):
        s.quantum(ref, m)
    for m in range(P, P + short):
        s.quantum(ref, m, 1)
    want = [s.quantum(ref, m) for m in range(P + short, P + short + back)]
    ref.close()
    pv = _pv(fft_size=fft, hop_size=hop, max_channels=2, max_hops=1, flags=RESIDENT | HOST_CHANNELS)
    assert pv.info()["kernel_name"] == "pv_wave_kernel_1024"
    for m in range(P):
        s.quantum(pv, m)
    for m in range(P, P + sat_out):
        s.quantum(pv, m, 1)
    for k in range(back):
        m = P + sat_out + k
        got = s.quantum(pv, m)
        assert got == want[k], f"quantum {k} after the channel came back (sequence number {1 + m % CYCLE})"
    pv.close()


# ---- 2. the cursor far from zero: a shift by a multiple of N changes no bit ----

CURSOR_CASES = [("pv_wave_kernel_1024", 1024, 256, 0), ("pv_wave2k_kernel", 2048, 512, 0), ("pv_wg16_kernel", 4096, 1024, 0), ("pv_wg16_kernel", 8192, 2048, 0),
                ("pv_wg_kernel", 2048, 32, 0), ("pv_wg_kernel", 2048, 512, WG), ("pv_chain_kernel", 1024, 256, GENERIC), ("pv_chain_kernel", 64, 16, GENERIC),
                ("pv_chain_kernel", 65536, 16384, GENERIC), ("pv_wave_kernel_1024", 1024, 256, FP64)]
CURSOR_IDS = [f"{k}-{n}-{h}-{f}" for k, n, h, f in CURSOR_CASES]


def _shifts(fft):
    """K: multiples of N; the two '- N' values make the cursor cross 2^31 and 2^32 inside the call."""
    return [2 ** 24, 2 ** 31 - fft, 2 ** 31, 2 ** 32 - fft, 2 ** 32, 2 ** 40, 2 ** 53, 2 ** 62]


def _cursor_input(fft, hop):
    R = fft // hop
    T = min(2 * R + 3, 64)
    rng = np.random.default_rng(fft * 3 + hop)
    x = (rng.standard_normal((2, T * hop)) * 0.2).astype(np.float32)
    # both scatter routes at every residue of the cursor (the fast paths tmod == 0 and tmod == N / 2 among them): 0.8 / 1.3 by half rounds, swapped every round;
    # with the four start cursors below a residue meets both even where T is a single round
    m = np.arange(T)
    pitch = np.where(((m // R) + (m % R >= max(R // 2, 1))) % 2 == 0, 0.8, 1.3).astype(np.float32) + (0.01 * rng.random(T)).astype(np.float32)
    return T, x, pitch


def _starts(fft, hop):
    R = fft // hop
    return sorted({0, hop, (R // 2) * hop, (R - 1) * hop})


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("kernel,fft,hop,flags", CURSOR_CASES, ids=CURSOR_IDS)
def test_a_cursor_shift_by_a_multiple_of_n_changes_no_bit_of_a_batch(kernel, fft, hop, flags):
    """process_batch and process_batch_device from c0 + K against the same call from c0."""
    import torch
    T, x, pitch = _cursor_input(fft, hop)
    pv = _pv(fft_size=fft, hop_size=hop, max_channels=2, max_hops=T, flags=flags)
    assert pv.info()["kernel_name"] == kernel
    d_x, d_p = torch.from_numpy(x).cuda(), torch.from_numpy(pitch).cuda()
    d_y = torch.empty_like(d_x)
    for c0 in _starts(fft, hop):
        base = None
        for K in [0] + _shifts(fft):
            assert K % fft == 0
            pv.reset()
            pv.time_cursor = c0 + K
            y = pv.process_batch(x, pitch)
            assert pv.time_cursor == c0 + K + T * hop
            pv.reset()
            pv.time_cursor = c0 + K
            d_y.zero_()
            torch.cuda.synchronize()
            pv.process_batch_device(d_x.data_ptr(), d_y.data_ptr(), 2, T, T * hop, d_p.data_ptr())
            pv.synchronize()
            assert pv.time_cursor == c0 + K + T * hop
            if base is None:
                base = _u32(y)
                assert np.any(y != 0)
            assert np.array_equal(_u32(y), base), f"process_batch: c0 {c0}, K {K}"
            assert np.array_equal(_u32(d_y.cpu().numpy()), base), f"process_batch_device: c0 {c0}, K {K}"
    pv.close()


def _quanta(pv, x, pitch, hop, first=0, count=None):
    T = len(pitch) if count is None else first + count
    y = np.empty((x.shape[0], (T - first) * hop), np.float32)
    for m in range(first, T):
        outs = [np.zeros(hop, np.float32) for _ in range(x.shape[0])]
        assert pv.process([[np.ascontiguousarray(x[c, m * hop:(m + 1) * hop]) for c in range(x.shape[0])]], [outs], {"pitchFactor": pitch[m:m + 1]}) is True
        for c in range(x.shape[0]):
            y[c, (m - first) * hop:(m - first + 1) * hop] = outs[c]
    return y


STREAM_CASES = [(k, n, h, f, r) for (k, n, h, f), r in zip(CURSOR_CASES, [True, True, True, True, False, False, False, False, False, True])]


@pytest.mark.parametrize("kernel,fft,hop,flags,resident", STREAM_CASES, ids=CURSOR_IDS)
def test_a_cursor_shift_changes_no_bit_of_a_stream_or_of_a_hand_over(kernel, fft, hop, flags, resident):
    """The streaming quantum in launch form and, where the shape has one, in resident form -- there the 8-bit residue field of the control word is all the
    waves see of the cursor -- and a stream handed from one handle to another at the large cursor (export / import), against the batch from c0."""
    T, x, pitch = _cursor_input(fft, hop)
    one = _pv(fft_size=fft, hop_size=hop, max_channels=2, max_hops=T, flags=flags)
    forms = [("launch", _pv(fft_size=fft, hop_size=hop, max_channels=2, max_hops=T, flags=flags | PINNED))]
    if resident:
        forms.append(("resident", _pv(fft_size=fft, hop_size=hop, max_channels=2, max_hops=T, flags=flags | RESIDENT)))
    other = _pv(fft_size=fft, hop_size=hop, max_channels=2, max_hops=T, flags=flags)
    for pv in [one, other] + [f[1] for f in forms]:
        assert pv.info()["kernel_name"] == kernel
    T1 = T // 2 + 1
    for c0 in _starts(fft, hop):
        one.reset()
        one.time_cursor = c0
        base = _u32(one.process_batch(x, pitch))
        for K in _shifts(fft):
            for what, pv in forms:
                pv.reset()
                pv.time_cursor = c0 + K
                y = _quanta(pv, x, pitch, hop)
                assert pv.time_cursor == c0 + K + T * hop
                assert np.array_equal(_u32(y), base), f"{what} form: c0 {c0}, K {K}"
            # the hand-over: T1 hops on one handle, the rest on another that imports what the first exports (cursor included)
            one.reset()
            one.time_cursor = c0 + K
            ya = one.process_batch(x[:, :T1 * hop], pitch[:T1])
            other.reset()
            for c in range(2):
                hist, acc, tc = one.export_state(c)
                assert tc == c0 + K + T1 * hop
                other.import_state(c, hist, acc, tc)
            assert other.time_cursor == c0 + K + T1 * hop
            yb = other.process_batch(x[:, T1 * hop:], pitch[T1:])
            assert other.time_cursor == c0 + K + T * hop
            assert np.array_equal(_u32(np.concatenate([ya, yb], axis=1)), base), f"export / import: c0 {c0}, K {K}"
    for pv in [one, other] + [f[1] for f in forms]:
        pv.close()


# ---- 3. against the oracle at a large cursor ----

@pytest.mark.parametrize("pf", [0.8, 1.5])
@pytest.mark.parametrize("signal", ["tonal", "noise"])
@pytest.mark.parametrize("kernel,fft,hop,flags", CURSOR_CASES, ids=CURSOR_IDS)
def test_the_kernel_follows_the_oracle_at_a_cursor_of_2_to_the_26(kernel, fft, hop, flags, signal, pf):
    """Gate: the suite's own 2e-7 RMS.  It holds out here because the oracle's rotation angle fl(fl(2 pi delta / N) t) is off by at most 2.4 * 2^-53 pi t =
    5.6e-8 rad at t = 2^26 (tests/test_rotation_error.py measures 3.7e-8), which on signals of RMS <= 0.5 adds less than 3e-8 to a figure of <= 1.5e-8."""
    T = 2 * (fft // hop) + 8
    cursor = 2 ** 26 + 3 * hop
    x = np.stack([S.make_signal(signal, c, T * hop) for c in range(2)])
    p = np.full(T, pf, np.float32)
    pv = _pv(fft_size=fft, hop_size=hop, max_channels=2, max_hops=T, flags=flags)
    assert pv.info()["kernel_name"] == kernel
    pv.time_cursor = cursor
    y = pv.process_batch(x, p)
    assert pv.time_cursor == cursor + T * hop
    pv.close()
    o = oracle_lib.Oracle(fft, hop, 2)
    o.time_cursor = cursor
    ref = o.process_planar(x, p)
    assert o.time_cursor == cursor + T * hop
    err = S.rms(y.astype(np.float64) - ref)
    print(f"{kernel} {fft}/{hop} flags {flags} {signal} f {pf} at cursor 2^26 + 3 hop: rms err {err:.3e}")
    assert np.any(ref != 0) and err < 2e-7
