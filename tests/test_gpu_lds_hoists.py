"""The N = 1024 frame with its LDS reads issued early (the routes of the f >= 1 scatter in one batch, the window rows in front of pass 3 of the inverse
transform, the twiddles in front of each radix-8): the reads moved, no value may have.

Every store predicate of the scatter and every rotation mode on the smallest shapes that reach them: hop 128 / 256 / 512 / 1024 (R = 8, 4, 2, 1: every
m mod R occurs in twelve hops), one and two channels, twelve hops in two batch calls of 7 and 5 with frames_per_chunk = 4 (chunk halos are crossed, the second
call starts from carried state).  pitchFactor 1.0 (no source moves), 1.25, 2.0 (more than half of the sources have a target >= N/2 + 1 and are dropped) and
a ramp 1.0 -> 2.0; inputs: tones plus noise, digital silence (no peak: every route is NOROUTE), one NaN sample in one window, and a tone on bin 256 (the
self-paired bin, which lane 0 alone stores).

The batch form must equal the hop-by-hop pv_process form bit for bit -- that form launches other instances of the same arithmetic -- and both hold the
bound of tests/test_gpu_parity.py against the oracle."""
import functools

import numpy as np
import pytest

import oracle_lib
import signals as S

N = 1024
T = 12
CALLS = (7, 5)
CHUNK = 4
REGRESSION_RMS = 2e-7        # tests/test_gpu_parity.py
PARITY_BAR_RMS = 1e-4
HOPS = [128, 256, 512, 1024]
PITCH = ["1.0", "1.25", "2.0", "ramp"]
INPUTS = ["tonal", "silence", "nan", "bin256"]


def _pitch(f):
    return np.linspace(1.0, 2.0, T).astype(np.float32) if f == "ramp" else np.full(T, float(f), np.float32)


@functools.lru_cache(maxsize=None)
def _input(kind, hop):
    """float32[2, T * hop] (read-only): channel 0 is the case's input, channel 1 a second tonal channel."""
    n = T * hop
    other = S.make_signal("tonal", 1, n)
    if kind == "tonal":
        x0 = S.make_signal("tonal", 0, n)
    elif kind == "silence":
        x0 = np.zeros(n, np.float32)
    elif kind == "nan":
        x0 = S.make_signal("tonal", 0, n).copy()
        x0[5 * hop + hop // 3] = np.nan
    else:
        i = np.arange(n, dtype=np.float64)
        x0 = (0.5 * np.sin(2 * np.pi * 0.25 * i) + S.make_signal("noise", 0, n).astype(np.float64) / 256).astype(np.float32)
    x = np.stack([x0, other])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _oracle(kind, hop, f, nch):
    with np.errstate(all="ignore"):
        y = oracle_lib.Oracle(N, hop, nch).process_planar(np.array(_input(kind, hop)[:nch]), _pitch(f))
    y.setflags(write=False)
    return y


def _batch(x, p, hop, nch):
    import phaze_amd
    pv = phaze_amd.PhaseVocoder(fft_size=N, hop_size=hop, max_channels=nch, max_hops=max(CALLS), frames_per_chunk=CHUNK)
    try:
        parts, pos = [], 0
        for n in CALLS:
            parts.append(pv.process_batch(x[:, pos * hop:(pos + n) * hop], p[pos:pos + n]))
            pos += n
        return np.concatenate(parts, axis=1), pv.info()["kernel_name"], pv.forward_stats()
    finally:
        pv.close()


def _hop_by_hop(x, p, hop, nch):
    import phaze_amd
    pv = phaze_amd.PhaseVocoder(fft_size=N, hop_size=hop, max_channels=nch, max_hops=1)
    try:
        y = np.zeros((nch, T * hop), np.float32)
        for m in range(T):
            outputs = [[np.zeros(hop, np.float32) for _ in range(nch)]]
            assert pv.process([[x[c, m * hop:(m + 1) * hop] for c in range(nch)]], outputs, {"pitchFactor": np.array([p[m]], np.float32)}) is True
            for c in range(nch):
                y[c, m * hop:(m + 1) * hop] = outputs[0][c]
        return y
    finally:
        pv.close()


def test_the_bin_256_input_has_its_peak_there():
    """(CPU) the strict test of the peak search, "greater than all four neighbours", holds at bin 256 of every window of that input."""
    for hop in HOPS:
        x = _input("bin256", hop)[0].astype(np.float64)
        w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)
        for start in range(0, T * hop - N + 1, hop):
            m = np.abs(np.fft.rfft(x[start:start + N] * w))
            assert m[256] > max(m[254], m[255], m[257], m[258]) and m[256] == m.max(), (hop, start)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("f", PITCH)
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("hop", HOPS)
def test_batch_equals_hop_by_hop_bit_for_bit_and_both_hold_the_parity_bound(hop, nch, f, kind):
    x, p = np.array(_input(kind, hop)[:nch]), _pitch(f)
    yb, name, (fp32_first_frames, _) = _batch(x, p, hop, nch)
    yh = _hop_by_hop(x, p, hop, nch)
    yo = _oracle(kind, hop, f, nch)
    what = (name, hop, nch, f, kind)
    assert "1024" in name, what
    # every frame of the batch calls went through an fp32-first instance (the instances whose forward transform is the packed one); whether a chain ran the
    # f >= 1 instance or the general one is decided on the device and not reported: tests/test_lds_wait_points.py holds the hoists in both kinds of instance's ISA
    assert fp32_first_frames >= nch * T, (what, fp32_first_frames)
    assert yb.tobytes() == yh.tobytes(), (what, int(np.count_nonzero(yb.view(np.uint32) != yh.view(np.uint32))))
    bad_ref = ~np.isfinite(yo)
    if kind == "nan":
        # the frames whose window holds the NaN are NaN in the reference and here, whole hops of channel 0 (tests/test_gpu_fuzz.py); every other sample holds the bound
        hops_ref = bad_ref[0].reshape(T, hop).any(axis=1)
        hops_got = (~np.isfinite(yb))[0].reshape(T, hop).any(axis=1)
        assert hops_ref.any() and np.array_equal(hops_ref, hops_got), (what, np.nonzero(hops_ref)[0], np.nonzero(hops_got)[0])
        assert not bad_ref[1:].any() and np.all(np.isfinite(yb[1:])), what
    else:
        assert not bad_ref.any() and np.all(np.isfinite(yb)), what
    err = S.rms((yb.astype(np.float64) - yo)[~bad_ref & np.isfinite(yb)])
    print(f"{what}: rms vs oracle {err:.3e}")
    assert err <= PARITY_BAR_RMS and err <= REGRESSION_RMS, (what, err)
    if kind == "silence":
        assert not yb[0].any(), what
