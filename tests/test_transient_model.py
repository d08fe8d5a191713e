"""CPU checks of the transient model (tests/transient_model.py): identity in a hold that starts with a reset, agreement with TempoModel / LinkModel
without resets, the planner's properties, and the onset rule on five signal classes."""
import numpy as np
import pytest

import transient_model as TM
from link_model import LinkModel
from tempo_model import TempoModel, positions, schedule

HOLD_GATE = 2e-7          # relative RMS: 4 x the 5.4e-8 the prototype measured, the margin this project gives f32 rounding elsewhere
HOLD_POWER = 0.5          # without the reset the same comparison must exceed this (1.2 .. 1.4 measured)


def hold_gate(N, hs):
    """HOLD_GATE, and where many frames overlap the f32 accumulator's own rounding: an output sample is the sum of ceil(N / hs) frames, one f32
    addition each, and every addition rounds by up to 2^-24 of a partial sum no larger than the result; independent roundings add in RMS, so the
    accumulator alone leaves 2^-24 sqrt(ceil(N / hs)): 9.5e-7 at 256 / 1, 6.7e-7 at 8192 / 64, 3.4e-7 at 512 / 16, below HOLD_GATE up to 11 frames."""
    return max(HOLD_GATE, 2.0 ** -24 * np.sqrt(-(-N // hs)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _hold_case(N, ha, hs, seed=1):
    J, pre = TM.hold_base(N, ha, hs)
    hops, resets, r = TM.hold_schedule(N, ha, hs, pre, J)
    x = np.random.default_rng(seed).standard_normal(int(hops.sum())).astype(np.float32)
    return hops, resets, r, J, x


@pytest.mark.parametrize("N,ha,hs", TM.HOLD_SHAPES)
def test_a_hold_that_starts_with_a_reset_is_the_input(N, ha, hs, record_property):
    """Reset at frame r, hops = hs for r .. r + J, Gaussian noise: every output sample that only frames r .. r + J write is g(n) x[n + delta].
    Measured 4.2e-8 .. 5.5e-8 with the reset where at most 11 frames overlap, 8.8e-8 at 512 / 16, 1.8e-7 at 8192 / 64 and 2.4e-7 at 256 / 1
    (gate: hold_gate), and 1.2 .. 1.4 without."""
    hops, resets, r, J, x = _hold_case(N, ha, hs)
    floor = min(ha, hs)
    y = TM.TransientModel(N, floor, hs).process_hops(x[None], hops, resets)[0]
    y0 = TM.TransientModel(N, floor, hs).process_hops(x[None], hops, None)[0]
    with_reset, without = TM.hold_identity(y, x, hops, N, hs, r, J), TM.hold_identity(y0, x, hops, N, hs, r, J)
    record_property("with_reset", with_reset)
    record_property("without", without)
    print(f"hold identity N={N} ha={ha} hs={hs}: {with_reset:.3e} with the reset, {without:.3f} without")
    assert with_reset <= hold_gate(N, hs), with_reset
    assert without > HOLD_POWER, without


@pytest.mark.parametrize("N,floor,hs", [(256, 32, 80), (1024, 205, 320)])
def test_no_resets_is_the_tempo_model_bit_for_bit(N, floor, hs):
    T = 40
    hops = schedule("random", floor, N, T, seed=2)
    x = np.random.default_rng(3).standard_normal((2, int(hops.sum()))).astype(np.float32)
    a, b = TM.TransientModel(N, floor, hs, 2), TempoModel(N, floor, hs, 2)
    for resets in (None, np.zeros(T, np.uint8)):
        a, b = TM.TransientModel(N, floor, hs, 2), TempoModel(N, floor, hs, 2)
        assert np.array_equal(_bits(a.process_hops(x, hops, resets)), _bits(b.process_hops(x, hops)))
        assert np.array_equal(a.phi, b.phi) and np.array_equal(a.psi, b.psi) and np.array_equal(_bits(a.acc), _bits(b.acc))


def test_no_resets_on_groups_is_the_link_model_bit_for_bit():
    N, floor, hs, T = 512, 64, 160, 30
    hops = schedule("ramp", floor, N, T)
    x = np.random.default_rng(4).standard_normal((4, int(hops.sum()))).astype(np.float32)
    a, b = TM.TransientModel(N, floor, hs, 4, 2), LinkModel(N, floor, hs, 4, 2)
    assert np.array_equal(_bits(a.process_hops(x, hops)), _bits(b.process_hops(x, hops)))
    assert np.array_equal(a.phi, b.phi) and np.array_equal(a.psi, b.psi)


def test_a_reset_at_frame_zero_of_a_fresh_model_changes_nothing_but_psi():
    """One frame on a fresh model, with and without the flag: phi, hist and the rule "no peak, no sound" are the same, and psi is q instead of the
    first advance.  On a silent first frame that is the whole difference: output and accumulator are zero either way."""
    N, floor, hs = 1024, 256, 320
    for x in (np.random.default_rng(5).standard_normal((1, floor)).astype(np.float32), np.zeros((1, floor), np.float32)):
        a, b = TM.TransientModel(N, floor, hs), TM.TransientModel(N, floor, hs)
        ya, yb = a.process_hops(x, [floor], [1]), b.process_hops(x, [floor], None)
        assert np.array_equal(a.phi, b.phi) and np.array_equal(_bits(a.hist[0]), _bits(b.hist[0]))
        assert np.array_equal(a.psi, a.phi) and not np.array_equal(a.psi, b.psi)
        if not np.any(x):
            assert not np.any(ya) and not np.any(yb) and not np.any(a.acc) and not np.any(b.acc)


def test_psi_equals_phi_after_a_reset_and_through_a_unit_tempo_hold():
    N, ha, hs = 1024, 256, 320
    hops, resets, r, J, x = _hold_case(N, ha, hs)
    m = TM.TransientModel(N, ha, hs)
    S = positions(hops)
    for f in range(r + J + 1):
        m.group_frame(0, [x[S[f]:S[f + 1]]], bool(resets[f]))
        if f >= r:
            assert np.array_equal(m.psi[0], m.phi[0]), f                   # floor((2 d hs + hs) / (2 hs)) = d: the advance telescopes exactly
    m.group_frame(0, [x[S[r + J + 1]:S[r + J + 2]]], False)
    assert not np.array_equal(m.psi[0], m.phi[0])                          # the hop moved: the stretch resumes


# ---- the planner ----------------------------------------------------------------------------------------------------------------------------

PLAN_SHAPES = [(1024, 256, 205, 320, None), (1024, 256, 205, 384, 0), (2048, 512, 300, 300, None), (1024, 341, 200, 256, None), (256, 100, 64, 97, 16),
               (4096, 1024, 512, 1536, None)]          # (N, ha, floor, hs, lead): stretches and two speed-ups (hs < ha)


@pytest.mark.parametrize("release", [None, 0])
@pytest.mark.parametrize("N,ha,floor,hs,lead", PLAN_SHAPES)
def test_planner_properties(N, ha, floor, hs, lead, release):
    L = N // 8 if lead is None else lead
    kappa = max(1, ha // 8)
    assert ha - kappa >= floor                                              # the catch-up can run both ways in these shapes
    rng = np.random.default_rng(N + hs)
    for trial in range(20):
        n = int(rng.integers(20 * N, 60 * N))
        onsets = np.sort(rng.integers(0, n - 2 * N, int(rng.integers(0, 8))))
        hops, resets, held = TM.transient_plan(onsets, n, N, ha, floor, hs, lead, release)
        S = positions(hops)
        assert hops.size and np.all((hops >= floor) & (hops <= N))
        assert S[-1] <= n and S[-1] + N > n - N                             # within the input, and it does not stop early
        assert np.all(hops[held] == hs)
        starts = held & ~np.concatenate([[False], held[:-1]])
        assert np.array_equal(resets.astype(bool), starts)                 # the first frame of each run, and only it
        for o in onsets:                                                    # in [L, N - L) of at least one held window
            inside = (o >= S[1:] - N + L) & (o < S[1:] - L)
            assert np.any(inside & held), (o, trial)
        # after a run, |debt| is back below kappa within ceil(|debt| / kappa) + 1 frames unless another run starts first
        debt = S[:-1] - np.arange(hops.size) * ha                           # before each frame
        ends = np.nonzero(held[:-1] & ~held[1:])[0] + 1                     # first frame after each run
        for e in ends:
            need = -(-abs(int(debt[e])) // kappa) + 1
            later = np.nonzero(held[e:])[0]
            stop = e + (later[0] if later.size else hops.size - e)
            if e + need < stop:
                assert abs(int(debt[e + need])) < kappa and debt[e + need] == 0, (e, need, debt[e:e + need + 1])


def test_planner_refuses_a_synthesis_hop_below_the_floor():
    with pytest.raises(ValueError):
        TM.transient_plan([1000], 50000, 1024, 256, 205, 200)


# ---- the onset rule ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,ha", [(1024, 256), (2048, 256), (4096, 1024)])
@pytest.mark.parametrize("name", sorted(TM.SIGNAL_CLASSES))
def test_onset_rule_finds_the_planted_onsets_and_nothing_else(N, ha, name, record_property):
    """tau = 0.4.  Every planted burst is found within one frame of where it starts; nothing else is reported after the first N / ha + 1 frames
    (the start of the buffer is itself an onset: frame -1 is silent)."""
    n = 40 * N
    planted = [7 * N + 137, 17 * N + 901, 29 * N + 333]
    x = TM.class_signal(name, n, N, planted, seed=3)
    c, _ = TM.onset_strength(x, N, ha)
    D = c / (N // 2 - 1)
    found = TM.onsets_from_strength(c, N, ha, 0.4)
    late = found[found >= (N // ha + 1) * ha]
    record_property("max_D", float(D[N // ha + 1:].max()))
    print(f"{name} {N}/{ha}: max D after the start {D[N // ha + 1:].max():.3f}, onsets {late.tolist()}")
    if TM.SIGNAL_CLASSES[name][1]:
        assert late.size == len(planted), (late, planted)
        assert np.all(np.abs(late - np.array(planted)) <= ha), (late, planted)
    else:
        assert late.size == 0, late
    if name == "noise" and (N, ha) == (1024, 256):
        assert 0.1 < D[N // ha + 1:].max() <= 0.25                         # 0.198 measured against tau = 0.4 (DESIGN.md "Phase resets")


# ---- the GPU tests' inputs, checked here before a GPU is asked ------------------------------------------------------------------------------

def _gpu_shapes():
    from test_gpu_transient import SHAPES
    return SHAPES


@pytest.mark.parametrize("N,G,nch", _gpu_shapes())
def test_gpu_parity_inputs_leave_out_at_most_one_percent_of_frames(N, G, nch):
    """The doubtful frames (stretch_model.doubtful_frame) of the inputs tests/test_gpu_transient.py compares with the model."""
    from test_gpu_transient import _parity_inputs
    f, hs, T, hops, r, x = _parity_inputs(N, G, nch)
    m = TM.TransientModel(N, f, hs, nch, G, track_doubt=True)
    m.process_hops(x, hops, r)
    nd = sum(int(np.count_nonzero(d)) for d in m.doubtful)
    assert nd <= 0.01 * T * (nch // G), nd


def test_gpu_onset_inputs_have_at_most_one_percent_near_ties():
    """The bins within 2 f32 ulps of either comparison of the onset count, over the inputs of the GPU test: <= 1 % of frames x 1 bin."""
    from test_gpu_transient import ONSET_SHAPES, _onset_input
    for N, ha in ONSET_SHAPES:
        tot, frames = 0, 0
        for name in sorted(TM.SIGNAL_CLASSES):
            c, d = TM.onset_strength(_onset_input(N, name), N, ha)
            tot, frames = tot + int(d.sum()), frames + c.size
        assert tot <= 0.01 * frames, (N, ha, tot, frames)


def _family_cases():
    import test_gpu_stretch_families as F
    cases = [(N, name, 1, "noise", sched, False) for N, name, sched in F.SCHEDULE_CASES]
    cases += [(N, name, G, "tonal", "random", True) for N, name, G in F.RESET_CASES] + [(N, name, G, None, "random", False) for N, name, G in F.LINK_CASES]
    return [c for c in cases if c[0] <= 512]


@pytest.mark.parametrize("N,name,G,kind,sched,flags", _family_cases())
def test_gpu_family_inputs_leave_out_at_most_one_percent_of_frames_and_one(N, name, G, kind, sched, flags):
    """The cap of tests/test_gpu_stretch_families.py on the model's doubtful frames, at the sizes that run here in seconds (N <= 512)."""
    import test_gpu_stretch_families as F
    floor, hs, T, hops, resets, hist, x = F.family_case(N, name, G, kind, sched, flags)
    _, m = F.family_model(N, floor, hs, G, hops, resets, hist, x)
    assert np.count_nonzero(m.doubtful[0]) <= 0.01 * T + 1
