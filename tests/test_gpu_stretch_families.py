"""GPU checks of the schedule, linked and reset kernels of the time stretch, and of onset strength, over the hop axis: the (analysis hop floor,
synthesis hop) edges that tests/test_gpu_stretch_edges.py runs through the fixed-hop kernels (halo = (N - 1) // hs from 1 to 255, floor = 1, N - 1
and N, hs = N / 2 and 1, hops that divide nothing), here through pv_tempo_process (the SCHED = true instances), pv_transient_process (pv_reset_pass_a /
scan / pass_b, unlinked and linked) and linked schedules (pv_link_pass_a / b), against tests/tempo_model.py and tests/transient_model.py; then two
properties that do not go through those models, the closed form of steady tones and the identity in a hold, at the same edges and over holds that
cross chain boundaries; and an onset-strength call whose chains outgrow the kernel's batch of counts.

Every gate is imported from the neighbouring modules.  Measured values are attached with record_property (visible with --junitxml)."""
import numpy as np
import pytest

import signals as S
import tones as TN
import transient_model as TM
from link_model import phase_fit, wrap
from tempo_model import TONE_SHAPES_EDGES, TempoModel, schedule, tone_schedule_input
from test_gpu_link import EDGES, PHASE
from test_gpu_stretch_edges import (GPU_TOL, PARITY_BLOCK, PARITY_GLOBAL, _frames, _matrix_signal, _pairs, assert_state, block_gate,
                                    state_shares)

pytestmark = pytest.mark.gpu
NS = (256, 512, 1024, 2048, 4096, 8192)
# the edges the group cases run at: the linked tests' own five, the two non-divisors' other one, one-sample hops, and hs = 1 where it exists
GROUP_EDGES = EDGES + ("255-64", "ha1", "hs1")
COUNT_BATCH = 256                                                     # pv_onset_strength_kernel: counts leave the workgroup this many frames at a time


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def _one_launch(ts, x, hops, resets=None):
    """The whole schedule in ONE launch whatever max_frames is (the device form is not staged in pieces), so the call has the chains of its length."""
    import torch
    nch, n = x.shape
    T = len(hops)
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros((nch, T * ts.synthesis_hop), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ts.process_hops_device(d_in.data_ptr(), d_out.data_ptr(), nch, T, hops, n, T * ts.synthesis_hop, resets=resets)
    ts.synchronize()
    return d_out.cpu().numpy()


# ---- 1. the parity matrix over the hop axis, per family -------------------------------------------------------------------------------------------------

def family_signal(N, n, G, kind):
    """float32[G, n].  One channel: the signal `kind`.  A group: three partials over a floor 80 dB down on even channels and noise on odd ones,
    channel c scaled 0.4 + 0.3 c and delayed by 17 c samples.  A group of 3 is noise in every channel: with the partials in two of three channels the
    model alone counts 2 doubtful frames of 64 and of 81 at N = 8192 (r1.25, hsN/2, r0.5), over the cap of 1 % and one frame."""
    if G == 1:
        return _matrix_signal(kind, N, n)[None, :]
    rows = [(_matrix_signal("partials", N, n + 17 * G) if c % 2 == 0 and G != 3 else S.make_signal("noise", c, n + 17 * G))[17 * c:17 * c + n]
            for c in range(G)]
    return np.stack([np.float32(0.4 + 0.3 * c) * r for c, r in enumerate(rows)]).astype(np.float32)


def family_case(N, name, G, kind, sched, flags):
    """(floor, hs, T, hops, resets or None, hist float32[G, N - floor], x float32[G, sum hops]): the edge `name` of _pairs(N) as (floor, hs), over
    T = _frames frames (>= 3 chains at the shortest chain length F0 = 4 (halo + 1)), started MID-STREAM: hist is the signal before the call (from
    silence the first frames of a small hop are all near-ties).  With flags: resets at [0, 5, F0 - 2, F0, F0 + 1, 2 F0 - 1, T - 1] and a run of
    max(hs, floor) hops over [F0 - 2, F0 + 3): a hold at unit tempo where the floor allows it, at the floor otherwise."""
    floor, hs = _pairs(N)[name]
    T = _frames(N, floor, hs)
    F0 = 4 * ((N - 1) // hs + 1)
    hops = schedule(sched, floor, N, T, seed=N)
    resets = None
    if flags:
        hops[F0 - 2:F0 + 3] = max(hs, floor)
        resets = np.zeros(T, np.uint8)
        resets[[0, 5, F0 - 2, F0, F0 + 1, 2 * F0 - 1, T - 1]] = 1
    n = int(hops.sum())
    xh = family_signal(N, N - floor + n, G, kind)
    return floor, hs, T, hops, resets, xh[:, :N - floor], xh[:, N - floor:]


def family_model(N, floor, hs, G, hops, resets, hist, x):
    """(reference output, the model after the run): TempoModel for one channel without flags (it keeps the conditioning state_shares needs),
    TransientModel otherwise; both from the imported history and with the doubtful frames tracked."""
    if G == 1 and resets is None:
        m = TempoModel(N, floor, hs, track_doubt=True)
        m.hist[0] = hist[0].copy()
        return m.process_hops(x, hops), m
    m = TM.TransientModel(N, floor, hs, G, G, track_doubt=True)
    for c in range(G):
        m.hist[c] = hist[c].copy()
    return m.process_hops(x, hops, resets), m


SCHEDULE_CASES = [(N, name, "random") for N in NS for name in _pairs(N)] + [(N, name, "alt") for N in NS for name in ("ha1", "100-97")]
RESET_CASES = [(N, name, 1) for N in NS for name in _pairs(N)] + [(N, name, G) for G in (2, 3) for N in NS for name in GROUP_EDGES if name in _pairs(N)]
LINK_CASES = [(N, name, G) for G in (2, 3, 8) for N in NS for name in GROUP_EDGES if name in _pairs(N)]


def _family(N, name, G, kind, sched, flags, record_property):
    import phaze_amd
    floor, hs, T, hops, resets, hist, x = family_case(N, name, G, kind, sched, flags)
    ref, m = family_model(N, floor, hs, G, hops, resets, hist, x)
    nd = int(np.count_nonzero(m.doubtful[0]))
    # a condition on the input, from the model alone: the block gate may leave out the blocks of at most 1 % of the frames, and one frame more
    assert nd <= 0.01 * T + 1, (nd, T)
    ts = phaze_amd.TimeStretch(N, floor, hs, max_channels=G, max_frames=1, channels_per_group=G)
    for c in range(G):
        ts.import_state(c, hist=hist[c])
    y = _one_launch(ts, x, hops, resets)
    st = [ts.export_state(c) for c in range(G)]
    g = _rel(y, ref)
    b = max(block_gate(y[c], ref[c], N, hs, m.doubtful[0])[0] for c in range(G))
    phi_share = float(np.mean(st[0][2] == m.phi[0]))
    shares = state_shares(ts, m, T, hs, floor) if G == 1 and not flags else {}
    ts.close()
    for k, v in {"global": g, "block": b, "doubtful": nd, "frames": T, "phi_share": phi_share, **shares}.items():
        record_property(k, v)
    print(f"N={N} {name} G={G} {sched}{' resets' if flags else ''}: T {T} global {g:.3e} block {b:.3e} doubtful {nd} phi {phi_share:.4f}")
    assert g <= PARITY_GLOBAL, (g, b, nd)
    assert b <= PARITY_BLOCK, (g, b, nd)
    assert phi_share >= 0.99, phi_share
    for c in range(G):
        _, _, phi, psi = st[c]
        assert np.array_equal(phi, st[0][2]) and np.array_equal(psi, st[0][3]), c        # every slot of a group carries the group's phases
        if flags:
            assert np.array_equal(phi, psi), c                          # the call ends on a flagged frame: psi == q in every bin, bit for bit
    if shares:
        assert_state(shares)


@pytest.mark.parametrize("N,name,sched", SCHEDULE_CASES)
def test_schedule_parity_over_the_hop_axis(N, name, sched, record_property):
    """One channel through the SCHED = true instances of pass A / pass B: uniform random hops in [floor, N] (at haN the constant schedule at hop N), and
    floor and N in turn (the largest per-frame jumps) at floor = 1 and 100."""
    _family(N, name, 1, "noise", sched, False, record_property)


@pytest.mark.parametrize("N,name,G", RESET_CASES)
def test_reset_parity_over_the_hop_axis(N, name, G, record_property):
    """pv_reset_pass_a / scan / pass_b, unlinked at every edge and linked (G = 2, 3) at GROUP_EDGES, with resets on both sides of the first two chain
    boundaries at the shortest chain length and on the last frame."""
    _family(N, name, G, "tonal", "random", True, record_property)


@pytest.mark.parametrize("N,name,G", LINK_CASES)
def test_linked_schedule_parity_over_the_hop_axis(N, name, G, record_property):
    """pv_link_pass_a / b on a schedule (the SCHED = true instances), groups of 2, 3 and 8."""
    _family(N, name, G, None, "random", False, record_property)


# ---- 2. closed forms that do not go through the models ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ramp", "random", "alt"])
@pytest.mark.parametrize("sid", list(TONE_SHAPES_EDGES))
def test_tones_closed_form_under_schedules_at_the_hop_edges(sid, kind, record_property):
    import phaze_amd
    N, floor, hs, freqs, amps = TONE_SHAPES_EDGES[sid]
    hops, x = tone_schedule_input(N, floor, hs, freqs, amps, kind)
    ts = phaze_amd.TimeStretch(N, floor, hs, max_channels=1, max_frames=1)
    y = _one_launch(ts, x[None, :], hops)[0]
    ts.close()
    ratio, res = TN.tone_fit(y, N, floor, hs, freqs, amps)
    err = max(float(np.max(np.abs(ratio - 1.0))), res)
    record_property("tone_err", err)
    print(f"tones {sid} {kind}: {err:.3e}")
    assert err <= GPU_TOL, (ratio, res)


@pytest.mark.parametrize("sid", list(TONE_SHAPES_EDGES))
def test_tones_linked_pair_under_a_schedule_at_the_hop_edges(sid, record_property):
    """One partial in a linked pair, amplitudes 0.5 / 0.2, phases 0.4 / 2.1, random hops: each channel passes the closed form on its own amplitude and
    the fitted inter-channel phase is 2.1 - 0.4."""
    import phaze_amd
    N, floor, hs, freqs, _ = TONE_SHAPES_EDGES[sid]
    hops, x = TM.tone_pair_input(N, floor, hs, freqs[0])
    ts = phaze_amd.TimeStretch(N, floor, hs, max_channels=2, max_frames=1, channels_per_group=2)
    y = _one_launch(ts, x, hops)
    ts.close()
    worst = 0.0
    for c in range(2):
        ratio, res = TN.tone_fit(y[c], N, floor, hs, freqs, [TM.PAIR_AMPS[c]])
        worst = max(worst, float(np.max(np.abs(ratio - 1.0))), res)
    p = phase_fit(y, N, floor, hs, freqs)
    dphi = float(np.abs(wrap(p[1] - p[0] - (TM.PAIR_PHASES[1] - TM.PAIR_PHASES[0]))).max())
    record_property("tone_err", worst)
    record_property("phase_err", dphi)
    print(f"linked pair of tones {sid}: tone error {worst:.3e} phase error {dphi:.3e} rad")
    assert worst <= GPU_TOL, worst
    assert dphi <= PHASE, dphi


def _long_hold(N, ha, hs, nch, G):
    """(J, F): the fewest held frames with which a one-launch call of this chip has its reset in chain 0 and the hold still running at the first
    frames of chains 1 AND 2 (frames F and 2 F): only the scan's composition of "set to v" with the chains' "add v" pairs carries the reset's value
    that far."""
    import phaze_amd
    floor = min(ha, hs)
    J, pre = TM.hold_base(N, ha, hs)
    probe = phaze_amd.TimeStretch(N, floor, hs, max_channels=nch, max_frames=1, channels_per_group=G)
    for _ in range(8):
        F, _halo = probe.chain_layout(nch, 2 * pre + J + 1)
        if pre + J >= 2 * F + 1:
            break
        J = 2 * F + 1 - pre
    probe.close()
    assert pre < F and pre + J >= 2 * F + 1 and 2 * pre + J + 1 > 2 * F, (pre, J, F)
    return J, F


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("N,ha,hs", TM.HOLD_SHAPES)
def test_hold_identity_over_chain_boundaries(N, ha, hs, G, record_property):
    """tests/test_gpu_transient.py's hold identity with a hold that spans two chain boundaries of one launch (unlinked, and a linked pair of independent
    noises where BOTH channels are their own input in the hold).  Gate: 4 x the model's value for the same case, computed here; without the flag > 0.5."""
    import phaze_amd
    J, F = _long_hold(N, ha, hs, G, G)
    _, pre = TM.hold_base(N, ha, hs)
    hops, resets, r = TM.hold_schedule(N, ha, hs, pre, J)
    n = int(hops.sum())
    x = np.stack([np.random.default_rng(11 + c).standard_normal(n).astype(np.float32) * np.float32(1.0 - 0.5 * c) for c in range(G)])
    floor = min(ha, hs)
    ref = TM.TransientModel(N, floor, hs, G, G).process_hops(x, hops, resets)
    ts = phaze_amd.TimeStretch(N, floor, hs, max_channels=G, max_frames=1, channels_per_group=G)
    y = _one_launch(ts, x, hops, resets)
    ts.reset()
    y0 = _one_launch(ts, x, hops)
    ts.close()
    for c in range(G):
        got, want = TM.hold_identity(y[c], x[c], hops, N, hs, r, J), TM.hold_identity(ref[c], x[c], hops, N, hs, r, J)
        without = TM.hold_identity(y0[c], x[c], hops, N, hs, r, J)
        record_property(f"gpu{c}", got)
        record_property(f"model{c}", want)
        print(f"long hold N={N} ha={ha} hs={hs} G={G} channel {c}: {J} held frames, chains of {F}: gpu {got:.3e} model {want:.3e} without {without:.3f}")
        assert got <= 4 * want, (c, got, want)
        assert without > 0.5, (c, without)


# ---- 3. onset strength: chains longer than the batch of counts --------------------------------------------------------------------------------------------

def test_onset_strength_chains_longer_than_two_count_batches(record_property):
    """64 mono groups at N = 256, ha = 8 leave each group few chains, so a chain holds F >= 2 COUNT_BATCH + 3 frames, F not a multiple of COUNT_BATCH:
    the kernel's batch of counts is flushed full twice, wraps, and is flushed partly filled.  F comes from the handle (onset_chain_layout).  Four
    distinct signals tiled over the 64 channels: tiled rows are equal bit for bit, and the four agree with the model within each frame's doubt count
    (tests/test_gpu_transient.py's rule; the allowances sum to <= 1 % of the frames)."""
    import phaze_amd
    N, ha, nch = 256, 8, 64
    ts = phaze_amd.TimeStretch(N, ha, N // 4, max_channels=nch, max_frames=1)
    T = 2 * COUNT_BATCH + 3
    while True:
        F = ts.onset_chain_layout(nch, T)
        if F >= 2 * COUNT_BATCH + 3 and F % COUNT_BATCH and F < T:
            break
        T += 2 * COUNT_BATCH + 3
        assert T < 4000 * COUNT_BATCH, (T, F)
    n = T * ha
    names = ["bursts_noise", "bursts_tones", "noise", "vibrato"]
    four = np.stack([TM.class_signal(nm, n, N, [n // 5 + 137, n // 2 + 901, 4 * n // 5 + 333], seed=3 + i) for i, nm in enumerate(names)])
    got = ts.onset_strength(np.tile(four, (nch // 4, 1)))
    ts.close()
    assert got.shape == (nch, T)
    for c in range(4, nch):
        assert np.array_equal(got[c], got[c % 4]), c
    tot = 0
    for i in range(4):
        c, d = TM.onset_strength(four[i], N, ha)
        bad = np.nonzero(np.abs(got[i].astype(np.int64) - c) > d)[0]
        assert bad.size == 0, (names[i], bad[:8], got[i][bad[:8]], c[bad[:8]])
        tot += int(d.sum())
    record_property("frames", T)
    record_property("frames_per_chain", F)
    record_property("allowance", tot)
    print(f"onset strength, {nch} groups: {T} frames in chains of {F}, allowance {tot} bins")
    assert tot <= 0.01 * 4 * T, (tot, T)
