"""The output bits of the frame kernels, pinned: SHA-256 digests of the output and of every channel's exported state (history, accumulator, time
cursor) for every hand-written frame kernel and the generic one, against tests/golden/frame_bits_parent.json.

The parity tests compare the kernels with the oracle within a tolerance; this one pins the bits themselves, which "the same source expression"
does not: the residue's butterflies and the stage twiddles are open to FMA contraction, and which product of a complex multiply is fused can change
with the text around it.  A change that means to keep the bits passes as it is; one that means to change them records the
file again: `python tests/test_gpu_frame_bits.py --record tests/golden/frame_bits_parent.json`.

Each case is 24 hops in two calls of 15 and 9 on one handle, frames_per_chunk = 5 (chunk halos are crossed, the second call starts from carried
state).  Channel 0 is the input of test_residue_fast_and_general_paths -- a strong partial at 0.488 cycles per sample (bin 0.976 N/2), a low tone,
noise / 256 -- with both sines quantised to 2^-20 so that the last bit of the host's sin() does not enter; channel 1 is a tonal channel.  With
f < 1 the last region ends near N/2 (1 + 0.976 (1 - f)): f = 0.85 reads the residue's fast form, f <= 0.7 the re-run stage structure (beyond
N/2 + N/8 + 1), f = 0.3 both upper quarters.  That the case reaches the path is asserted on a tapped frame, not assumed.

The reference-width flavour's copies (build/exp/libphaze_fp64.so) run the same cases in a child process, the library being chosen at import."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_bits_parent.json")
FP64_LIB = os.path.join(ROOT, "build", "exp", "libphaze_fp64.so")
CALLS = (15, 9)
CHUNK = 5
# (fft, hop, pv_config.flags): the sizes are the kernels' own.  flags = 4 (PV_FLAG_WORKGROUP_KERNEL): the eight-element workgroup kernel
SHAPES = [(1024, 256, 0), (1024, 128, 0),                      # pv_wave_kernel_1024
          (2048, 512, 0), (2048, 128, 0),                      # pv_wave2k_kernel (hop 128: half-row layout)
          (4096, 1024, 0), (8192, 2048, 0),                    # pv_wg16_kernel
          (2048, 512, 4), (4096, 1024, 4), (8192, 2048, 4),    # pv_wg_kernel
          (4096, 256, 0), (2048, 128, 4),                      # pv_wg_kernel's LDS overlap-add ring
          (512, 128, 0), (16384, 4096, 0)]                     # pv_chain_kernel
FP64_SHAPES = [(1024, 256, 0), (4096, 1024, 0), (8192, 2048, 0)]
PITCH = ["1.25", "0.85", "0.7", "0.55", "0.3", "ramp"]
CASES = [(N, hop, fl, f) for N, hop, fl in SHAPES for f in PITCH]
FP64_CASES = [(N, hop, fl, f) for N, hop, fl in FP64_SHAPES for f in PITCH]
PARTS = ("output", "hist", "acc", "cursor")


def _name(N, hop, flags, f, fp64=False):
    return f"{'fp64-' if fp64 else ''}{N}-{hop}-flags{flags}-{f}"


def _input(n):
    import signals as S
    i = np.arange(n, dtype=np.float64)
    q = lambda v: np.round(v * 2.0 ** 20) / 2.0 ** 20
    hi = 0.3 * q(np.sin(2 * np.pi * (0.488 * i))) + 0.05 * q(np.sin(2 * np.pi * 0.031 * i))
    return np.stack([(hi + S.make_signal("noise", 0, n).astype(np.float64) / 256).astype(np.float32), S.make_signal("tonal", 1, n)])


def _pitch(f, T):
    if f == "ramp":
        return (0.4 + 1.85 * np.arange(T) / (T - 1)).astype(np.float32)
    return np.full(T, float(f), np.float32)


def digests(N, hop, flags, f):
    """({"call<i>.<part>": sha256 hex} of the two calls of one case, the tap's findings).  The tap runs the frame after the last call with the
    case's pitch factor (the ramp: none) and reports whether X is non-zero beyond the fast residue's reach and in the last quarter."""
    import phaze_amd
    T = sum(CALLS)
    x, p = _input((T + 1) * hop), _pitch(f, T)
    pv = phaze_amd.PhaseVocoder(fft_size=N, hop_size=hop, max_channels=2, max_hops=max(CALLS), frames_per_chunk=CHUNK, flags=flags)
    out, tap = {}, {"kernel": pv.info()["kernel_name"]}
    try:
        pos = 0
        for i, n in enumerate(CALLS):
            y = pv.process_batch(x[:, pos * hop:(pos + n) * hop], p[pos:pos + n])
            pos += n
            state = [pv.export_state(c) for c in range(2)]
            out[f"call{i}.output"] = hashlib.sha256(y.tobytes()).hexdigest()
            out[f"call{i}.hist"] = hashlib.sha256(b"".join(np.ascontiguousarray(s[0]).tobytes() for s in state)).hexdigest()
            out[f"call{i}.acc"] = hashlib.sha256(b"".join(np.ascontiguousarray(s[1]).tobytes() for s in state)).hexdigest()
            out[f"call{i}.cursor"] = hashlib.sha256(repr([int(s[2]) for s in state]).encode()).hexdigest()
        if f != "ramp":
            X = pv.debug_frame(0, x[0, T * hop:(T + 1) * hop], float(f))["X"]
            X = np.abs(X[0::2]) + np.abs(X[1::2])
            tap["beyond_fast"] = bool(np.any(X[N // 2 + N // 8 + 2:] != 0.0))
            tap["last_quarter"] = bool(np.any(X[3 * N // 4:] != 0.0))
    finally:
        pv.close()
    return out, tap


def _assert_path(N, hop, flags, f, tap):
    if f in ("0.7", "0.55", "0.3"):
        assert tap["beyond_fast"], f"{_name(N, hop, flags, f)}: the tapped frame did not run the residue's stage structure ({tap})"
    if f == "0.3":
        assert tap["last_quarter"], f"{_name(N, hop, flags, f)}: the tapped frame did not reach the last quarter ({tap})"


def _fp64_child(N, hop, flags):
    """The six pitch rows of one shape on the reference-width flavour: {pitch: [digests, tap]} from a child process that imports that library."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--digest", str(N), str(hop), str(flags)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PHAZE_LIB=FP64_LIB))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_these_cases():
    want = {_name(*c) for c in CASES} | {_name(*c, fp64=True) for c in FP64_CASES}
    got = _golden()
    assert set(got) == want
    for name, d in got.items():
        assert set(d) == {f"call{i}.{p}" for i in range(len(CALLS)) for p in PARTS}, name
        assert all(len(v) == 64 and set(v) <= set("0123456789abcdef") for v in d.values()), name


@pytest.mark.gpu
@pytest.mark.parametrize("N,hop,flags,f", CASES, ids=[_name(*c) for c in CASES])
def test_frame_bits_equal_the_recorded_ones(N, hop, flags, f):
    want = _golden()[_name(N, hop, flags, f)]
    got, tap = digests(N, hop, flags, f)
    _assert_path(N, hop, flags, f, tap)
    differ = sorted(k for k in want if got.get(k) != want[k])
    assert not differ and set(got) == set(want), f"{_name(N, hop, flags, f)} ({tap['kernel']}): differs from the recorded bits in {differ}"


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(FP64_LIB), reason="build/exp/libphaze_fp64.so not built (make -C phaze_amd/csrc fp64)")
@pytest.mark.parametrize("N,hop,flags", FP64_SHAPES, ids=[f"{N}-{hop}" for N, hop, _ in FP64_SHAPES])
def test_reference_width_flavour_bits_equal_the_recorded_ones(N, hop, flags):
    golden, rows = _golden(), _fp64_child(N, hop, flags)
    assert set(rows) == set(PITCH)
    for f in PITCH:
        got, tap = rows[f]
        want = golden[_name(N, hop, flags, f, fp64=True)]
        _assert_path(N, hop, flags, f, tap)
        differ = sorted(k for k in want if got.get(k) != want[k])
        assert not differ and set(got) == set(want), f"{_name(N, hop, flags, f, fp64=True)} ({tap['kernel']}): differs from the recorded bits in {differ}"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if len(sys.argv) == 5 and sys.argv[1] == "--digest":
        N, hop, flags = (int(v) for v in sys.argv[2:])
        import phaze_amd
        assert phaze_amd.library_path() == os.environ.get("PHAZE_LIB"), phaze_amd.library_path()
        print(json.dumps({f: digests(N, hop, flags, f) for f in PITCH}))
        sys.exit(0)
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_frame_bits.py --record PATH")
    rec = {}
    for c in CASES:
        rec[_name(*c)], tap = digests(*c)
        print(_name(*c), tap, flush=True)
        _assert_path(*c, tap)
    for N, hop, flags in FP64_SHAPES:
        for f, (d, tap) in _fp64_child(N, hop, flags).items():
            rec[_name(N, hop, flags, f, fp64=True)] = d
            print(_name(N, hop, flags, f, fp64=True), tap, flush=True)
            _assert_path(N, hop, flags, f, tap)
    with open(sys.argv[2], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} cases to {sys.argv[2]}")
