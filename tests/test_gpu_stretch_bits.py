"""The output bits of the time stretch, pinned: SHA-256 digests of the output and of every slot's carried state for all six kernel families (fixed
hop, schedule, linked fixed, linked schedule, resets unlinked, resets linked) at every size, against tests/golden/stretch_bits_parent.json.

The golden file was recorded on a build of the commit BEFORE the three copies of pass A / pass B were folded into one template (run this file as a
script on that build: `python tests/test_gpu_stretch_bits.py --record tests/golden/stretch_bits_parent.json`).  The family-against-family and
model tests compare kernels with each other and with Python within tolerances; this one pins the bits themselves, which "the same source expression"
does not (the forward transform's fp64 butterflies are open to FMA contraction, so a restructured kernel may legally round differently).

Every carried quantity of the design is an integer sum or a per-frame function of the input, so the bits do not depend on how a call is cut into
chains: the digests hold on a chip with any number of compute units.

Each case is two device-form calls on one handle: 41 frames (three chains of 16, 16 and 9 frames wherever the chip holds at least three workgroups
per channel, hs = N / 4 giving halo 3 and a minimum chain of 16) and then 7 frames from the carried state (one chain shorter than 4 (halo + 1)).
Reset flags sit on a chain's first frame, the frame before a chain boundary, one inside a halo and the last frame of each call."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stretch_bits_parent.json")
SIZES = [256, 512, 1024, 2048, 4096, 8192]
CALLS = (41, 7)
RESETS = ([0, 15, 16, 38, 40], [6])
# family -> (channels per group, channels, scheduled hops, resets)
FAMILIES = {"fixed": (1, 2, False, False), "schedule": (1, 2, True, False), "link2_fixed": (2, 4, False, False), "link2_schedule": (2, 4, True, False),
            "reset1": (1, 2, True, True), "reset2": (2, 4, True, True)}
# N = 1024 only: a group of 5 (the mix loads go out MIX_BATCH = 4 at a time), and two groups of 2 that each follow their own schedule row
EXTRA = {"link5_fixed": (5, 5, False, False), "link2_own_rows": (2, 4, "rows", False)}
CASES = [(N, f) for N in SIZES for f in FAMILIES] + [(1024, f) for f in EXTRA]
PARTS = ("output", "hist", "acc", "phi", "psi")


def _input(rng, nch, n):
    """Uniform noise in [-0.5, 0.5) plus one sine per channel so that peaks exist.  The sine is quantised to 2^-20 before it is scaled: exact in f32
    and independent of the last bit of the host's sin()."""
    noise = rng.random((nch, n), dtype=np.float32) - np.float32(0.5)
    t = np.arange(n, dtype=np.float64)
    tone = np.stack([np.round(np.sin(2.0 * np.pi * (0.031 + 0.007 * c) * t) * 2.0 ** 20) / 2.0 ** 20 * 0.25 for c in range(nch)])
    return noise + tone.astype(np.float32)


def digests(N, family):
    """{"call<i>.<part>": sha256 hex} of the two calls of one case."""
    import torch
    import phaze_amd
    G, nch, sched, resets = (FAMILIES.get(family) or EXTRA[family])
    ha, hs = N // 5, N // 4
    rng = np.random.default_rng(1000 * N + sorted(list(FAMILIES) + list(EXTRA)).index(family))
    ts = phaze_amd.TimeStretch(N, ha, hs, max_channels=nch, max_frames=max(CALLS), channels_per_group=G)
    out = {}
    try:
        for i, T in enumerate(CALLS):
            if sched == "rows":                                           # one row per group, repeated for the group's channels
                hops = np.repeat(rng.integers(ha, N // 3, (nch // G, T), endpoint=True), G, axis=0).astype(np.int32)
                n = int(hops.sum(axis=1).max())
            elif sched:
                hops = rng.integers(ha, N // 3, T, endpoint=True).astype(np.int32)
                n = int(hops.sum())
            else:
                hops, n = None, T * ha
            x = torch.from_numpy(_input(rng, nch, n)).cuda().contiguous()
            y = torch.full((nch, T * hs), -1234.5, dtype=torch.float32, device="cuda")
            if hops is None:
                ts.process_device(x.data_ptr(), y.data_ptr(), nch, T, n, T * hs)
            else:
                flags = None
                if resets:
                    flags = np.zeros(T, np.uint8)
                    flags[RESETS[i]] = 1
                ts.process_hops_device(x.data_ptr(), y.data_ptr(), nch, T, hops, n, T * hs, resets=flags)
            ts.synchronize()
            state = [ts.export_state(c) for c in range(nch)]
            out[f"call{i}.output"] = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()
            for j, part in enumerate(PARTS[1:]):
                out[f"call{i}.{part}"] = hashlib.sha256(b"".join(np.ascontiguousarray(s[j]).tobytes() for s in state)).hexdigest()
    finally:
        ts.close()
    return out


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_these_cases():
    want = {f"{N}-{f}": {f"call{i}.{p}" for i in range(len(CALLS)) for p in PARTS} for N, f in CASES}
    got = _golden()
    assert set(got) == set(want)
    for name, d in got.items():
        assert set(d) == want[name], name
        assert all(len(v) == 64 and set(v) <= set("0123456789abcdef") for v in d.values()), name


@pytest.mark.gpu
@pytest.mark.parametrize("N,family", CASES, ids=[f"{N}-{f}" for N, f in CASES])
def test_stretch_bits_equal_the_parent_commits(N, family):
    want = _golden()[f"{N}-{family}"]
    got = digests(N, family)
    differ = sorted(k for k in want if got.get(k) != want[k])
    assert not differ and set(got) == set(want), f"{N}-{family}: differs from the recorded bits in {differ}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_stretch_bits.py --record PATH")
    rec = {f"{N}-{f}": digests(N, f) for N, f in CASES}
    with open(sys.argv[2], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} cases to {sys.argv[2]}")
