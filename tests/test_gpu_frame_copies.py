"""The fp32-first pitchFactor >= 1 batch instances of pv_wave_kernel_1024 with their packed helpers fused, wave-uniform factors taken from SGPRs and the register
transposes done without copies: statements were merged, operand classes changed and data moves differently -- no value may have changed.

N = 1024, hop 128 / 256 / 512 / 1024, 3 channels x 48 hops in one batch call with frames_per_chunk = 8: six chains per channel with halos, every m mod 4, and the chain
list of the device-side classification in use.  pitchFactor 1.0, 1.5, 2.0 and one row drawn per hop in [1, 2]: every chain is of the f >= 1 class.  Two signals of
bench.other_input: `white` (every frame class A: the fp32 transform, the fused split pass, the guard-band test) and `tonal80` (every frame class B: the out-of-line
fp64 transform, and the chain turns fp64-first), so both hot flows of the instance run.

Each case must equal, bit for bit -- output, history, accumulator, time cursor --, the same stream fed hop by hop to a PV_FLAG_PERSISTENT_STREAM handle: that handle runs
the general resident instance, whose code did not change.  And each holds the bound of tests/test_gpu_parity.py against the oracle."""
import functools

import numpy as np
import pytest

import oracle_lib
import signals as S
from test_gpu_parity import PARITY_BAR_RMS, REGRESSION_RMS

N = 1024
T = 48
NCH = 3
CHUNK = 8
HOPS = [128, 256, 512, 1024]
PITCH = ["1.0", "1.5", "2.0", "drawn"]
SIGNALS = ["white", "tonal80"]


@functools.lru_cache(maxsize=None)
def _pitch(f):
    p = np.random.default_rng(7).uniform(1.0, 2.0, T).astype(np.float32) if f == "drawn" else np.full(T, float(f), np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _input(kind, hop):
    """float32[NCH, T * hop] (read-only) of bench.other_input's class `kind`."""
    import torch
    import bench
    x = bench.other_input(torch, kind, NCH, T * hop, "cuda", hop).cpu().numpy().astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _oracle(kind, hop, f):
    y = oracle_lib.Oracle(N, hop, NCH).process_planar(np.array(_input(kind, hop)), np.array(_pitch(f)))
    y.setflags(write=False)
    return y


def _state(pv):
    return [pv.export_state(c) for c in range(NCH)]


def _batch(x, p, hop):
    import phaze_amd
    pv = phaze_amd.PhaseVocoder(fft_size=N, hop_size=hop, max_channels=NCH, max_hops=T, frames_per_chunk=CHUNK)
    try:
        y = pv.process_batch(x, p)
        return y, _state(pv), pv.forward_stats(), pv.info()["kernel_name"]
    finally:
        pv.close()


def _resident(x, p, hop):
    import phaze_amd
    pv = phaze_amd.PhaseVocoder(fft_size=N, hop_size=hop, max_channels=NCH, max_hops=1, flags=phaze_amd.FLAG_PERSISTENT_STREAM)
    try:
        y = np.zeros((NCH, T * hop), np.float32)
        for m in range(T):
            blk = [np.ascontiguousarray(x[c, m * hop:(m + 1) * hop]) for c in range(NCH)]
            outs = [np.zeros(hop, np.float32) for _ in range(NCH)]
            assert pv.process([blk], [outs], {"pitchFactor": p[m:m + 1]}) is True
            for c in range(NCH):
                y[c, m * hop:(m + 1) * hop] = outs[c]
        return y, _state(pv)
    finally:
        pv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SIGNALS)
@pytest.mark.parametrize("f", PITCH)
@pytest.mark.parametrize("hop", HOPS)
def test_batch_equals_the_resident_stream_bit_for_bit_and_holds_the_parity_bound(hop, f, kind):
    x, p = np.array(_input(kind, hop)), np.array(_pitch(f))
    yb, sb, (frames, fallbacks), name = _batch(x, p, hop)
    yr, sr = _resident(x, p, hop)
    what = (name, hop, f, kind)
    assert "1024" in str(name), what
    # every frame went through an fp32-first instance (a chain also computes the R - 1 frames of its halo)
    assert frames >= NCH * T, (what, frames)
    print(f"{what}: {frames} frames, {fallbacks} fell back to fp64")
    if kind == "white":
        assert fallbacks == 0, (what, frames, fallbacks)
    else:
        assert fallbacks == frames, (what, frames, fallbacks)
    assert yb.tobytes() == yr.tobytes(), (what, int(np.count_nonzero(yb.view(np.uint32) != yr.view(np.uint32))))
    for c in range(NCH):
        (hb, ab, tb), (hr, ar, tr) = sb[c], sr[c]
        assert hb.tobytes() == hr.tobytes() and ab.tobytes() == ar.tobytes() and tb == tr, (what, c, tb, tr)
    yo = _oracle(kind, hop, f)
    assert np.all(np.isfinite(yb)) and np.all(np.isfinite(yo)), what
    err = S.rms(yb.astype(np.float64) - yo)
    print(f"{what}: rms vs oracle {err:.3e}")
    assert err <= PARITY_BAR_RMS and err <= REGRESSION_RMS, (what, err)
