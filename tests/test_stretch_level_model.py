"""Parity at level for the time stretch, CPU side (tests/stretch_level_model.py): the float32 restatement's own figures against the fp64 models are pinned and
reproduced -- the GPU gate of tests/test_gpu_stretch_level.py is 4 x these --, errors planted in the models' own output pass today's gates
(test_gpu_stretch_edges.PARITY_GLOBAL and block_gate at PARITY_BLOCK) and miss the new one by orders of magnitude, the corpus has the dynamics the GPU test relies on,
and the doubtful frames stay under their cap for every case the GPU file runs, counted by the model alone.  No kernel is involved."""
import numpy as np
import pytest

import level_model as LM
import stretch_level_model as SL
from link_model import LinkModel
from stretch_model import StretchModel, doubtful_frame
from tempo_model import TempoModel
from test_gpu_stretch_edges import PARITY_BLOCK, PARITY_GLOBAL, _rel, block_gate

SIZES = sorted(SL.RESTATEMENT_FIGURES)
SHAPES = [(N, ha, hs) for N, ha, hs, _, _ in SL.FIXED_SHAPES]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("N", SIZES)
def test_restatement_figures_are_pinned_and_reproduced(N):
    """Over the fixed-hop and family cases of one FFT size.  The model the restatement drives (TransientModel) gives the bits of the model each family is defined by;
    blocks with L == 0 are exact zeros in the restatement too (finite figures)."""
    worst = np.zeros(2)
    for cid in SL.case_list():
        if cid[1] != N:
            continue
        c = SL.case(*cid)
        y, yref = SL.restate_case(c)
        assert np.array_equal(_bits(yref), _bits(c.ref)), cid
        rr, mm = LM.hop_metrics(y, c.ref, c.L, c.hs)
        assert np.isfinite(rr.max()) and np.isfinite(mm.max()), cid
        print(f"restatement {SL.case_id(cid)}: worst rms/L {rr.max():.3e}  max/L {mm.max():.3e}")
        worst = np.maximum(worst, [rr.max(), mm.max()])
    k_rms, k_max = SL.RESTATEMENT_FIGURES[N]
    print(f"restatement N={N}: worst rms/L {worst[0]:.3e} (pinned {k_rms:.2e})  max/L {worst[1]:.3e} (pinned {k_max:.2e})")
    assert worst[0] <= k_rms and worst[1] <= k_max
    assert worst[0] >= k_rms / 1.25 and worst[1] >= k_max / 1.25, "the pinned figures are stale"


def test_the_default_models_are_untouched_by_the_restatement():
    """restate reads the models' decisions and integers; it changes nothing in them: a fixed hop, a schedule and a linked schedule give the same bits before and after."""
    c = SL.case("fixed", 256, 64, 80, "quiet_mid")
    before = StretchModel(c.N, c.ha, c.hs, c.nch).process(c.x)
    SL.restate_case(c)
    assert np.array_equal(_bits(StretchModel(c.N, c.ha, c.hs, c.nch).process(c.x)), _bits(before))
    c = SL.case("sched", 256, 64, 80, "burst")
    assert np.array_equal(_bits(TempoModel(c.N, c.ha, c.hs, c.nch).process_hops(c.x, c.hops)), _bits(SL.restate_case(c)[1]))
    c = SL.case("link2s", 256, 64, 80, "fade")
    assert np.array_equal(_bits(LinkModel(c.N, c.ha, c.hs, c.nch, 2).process_hops(c.x, c.hops)), _bits(SL.restate_case(c)[1]))


def _old_gates(y, c):
    """(worst channel's relative RMS, worst block RMS relative to the whole reference's) -- the two numbers every stretch kernel was held by."""
    g = max(_rel(y[ch], c.ref[ch]) for ch in range(c.nch))
    b = max(block_gate(y[ch], c.ref[ch], c.N, c.hs, c.doubt[ch])[0] for ch in range(c.nch))
    return g, b


@pytest.mark.parametrize("N,ha,hs", [(1024, 256, 320), (256, 7, 8), (4096, 1024, 1280), (512, 32, 256)])
def test_the_gap_is_real(N, ha, hs):
    """Three defects planted in a copy of the reference's own output of `fade`: 1 % of gain where the level is 100 dB or more under the channel's loudest, zeros where
    it is 130 dB or more under, a constant 1e-9.  Each copy passes PARITY_GLOBAL and block_gate at PARITY_BLOCK and misses the new gate by orders of magnitude."""
    c = SL.case("fixed", N, ha, hs, "fade")
    k_rms, k_max = SL.gate(N)
    assert 0 < k_rms < 1e-6 and 0 < k_max < 1e-5
    top = c.L.max(axis=1, keepdims=True)
    per_sample = lambda mask: np.repeat(mask, hs, axis=1)
    ref64 = c.ref.astype(np.float64)
    planted = {
        "x 1.01 at -100 dB": np.where(per_sample(c.L <= 1e-5 * top), ref64 * 1.01, ref64).astype(np.float32),
        "zero at -130 dB": np.where(per_sample(c.L <= 10.0 ** -6.5 * top), 0.0, ref64).astype(np.float32),
        "+ 1e-9": (ref64 + 1e-9).astype(np.float32),
    }
    assert not SL.block_failures(c.ref, c.ref, c.L, hs, k_rms, k_max, c.skip)[0]
    for what, y in planted.items():
        assert np.any(_bits(y) != _bits(c.ref)), what
        g, b = _old_gates(y, c)
        fails, (wr, wm) = SL.block_failures(y, c.ref, c.L, hs, k_rms, k_max, c.skip)
        print(f"{N}/{ha}/{hs} {what}: global {g:.2e} (gate {PARITY_GLOBAL:.0e})  block {b:.2e} (gate {PARITY_BLOCK:.0e})  rms/L {wr:.2e} (gate {k_rms:.1e})  "
              f"max/L {wm:.2e} (gate {k_max:.1e})  {len(fails)} blocks miss")
        assert g <= PARITY_GLOBAL and b <= PARITY_BLOCK, (what, g, b)
        assert fails and wr >= 100 * k_rms and wm >= 100 * k_max, (what, wr, wm)


@pytest.mark.parametrize("N,ha,hs", SHAPES)
def test_the_corpus_has_dynamics(N, ha, hs):
    """Per shape and family: at least a third of the blocks of `fade` lie 80 dB or more under that channel's loudest block, `burst` has at least two blocks with
    L == 0 per channel and the reference is exactly 0 there, and at the shortest chain length a stream has three chains,
    one starting in the quiet stretch of `fade` and one inside the silence of `burst` (the GPU test checks the same against the length the handle reports)."""
    families = ["fixed"] + [f for f in SL.FAMILIES if (N, ha, hs) in SL.FAMILY_SHAPES and "fade" in SL.FAMILIES[f]]
    F0 = SL.chain_floor(N, hs)
    for family in families:
        c = SL.case(family, N, ha, hs, "fade")
        starts = np.arange(F0, c.T, F0)
        assert starts.size >= 2, (family, c.T, F0)
        quiet = c.L <= 1e-4 * c.L.max(axis=1, keepdims=True)
        share = quiet.mean(axis=1)
        print(f"{family} {N}/{ha}/{hs}: {c.T} frames, share of fade's blocks 80 dB under the loudest {share.min():.2f}")
        assert np.all(share >= 1 / 3), (family, share)
        assert np.any(np.all(quiet[:, starts], axis=0)), family
        b = SL.case(family, N, ha, hs, "burst")
        zero = b.L == 0
        assert np.all(zero.sum(axis=1) >= 2), family
        assert np.any(np.all(zero[:, starts], axis=0)), family
        assert SL.zero_blocks_exact(b.ref, b.L, hs), family
        assert 0 < b.cuts[1] < b.cuts[2] < b.T and np.all(zero[:, b.cuts[1]]) and np.all(quiet[:, c.cuts[2]]), (family, b.cuts)
        if b.resets is not None:
            m = np.flatnonzero(b.resets)
            assert list(m) == [b.B + 2, b.T // 2] and np.all(b.silent[:, m[0] - 1]) and not np.any(b.silent[:, m[0]]), m
    for name in SL.FIXED_SHAPES[SHAPES.index((N, ha, hs))][4]:
        c = SL.case("fixed", N, ha, hs, name)
        assert 1e-9 < np.max(np.abs(c.x)) < 1e9, name
        assert SL.zero_blocks_exact(c.ref, c.L, hs) and np.all(np.isfinite(c.ref)), name


def test_a_frame_of_digital_silence_is_not_doubtful_here():
    """stretch_model.doubtful_frame calls a frame whose magnitudes are all 0 doubtful (every comparison ties), which in `burst` alone is far over the cap; no transform
    can decide such a frame differently, and the new tests do not count it.  doubtful_frame itself is unchanged."""
    assert doubtful_frame(np.zeros(129, np.float32))
    c = SL.case("fixed", 1024, 256, 320, "burst")
    raw, nf = int(c.doubt_raw.sum()), c.doubt_raw.size
    assert np.all(c.doubt_raw[c.silent]) and int(c.silent.sum()) == raw - SL.doubt_count(c)[0]
    assert raw > SL.doubt_cap(nf) >= SL.doubt_count(c)[0], (raw, nf)
    # a silent frame is silent in the model: no peak, an all-zero output frame
    m = StretchModel(c.N, c.ha, c.hs, 1)
    t = int(np.flatnonzero(c.silent[0])[0])
    for i in range(t + 1):
        m.frame(0, c.x[0, i * c.ha:(i + 1) * c.ha])
    assert not np.any(m.last["mag"]) and m.last["peaks"][0] < 0


@pytest.mark.parametrize("cid", SL.case_list(), ids=SL.case_id)
def test_doubtful_frames_stay_under_the_cap(cid):
    """At most 1 % of a case's frames plus one are doubtful and not silent, counted by the model alone; the blocks they reach are all the GPU test may leave out."""
    c = SL.case(*cid)
    nd, nf = SL.doubt_count(c)
    print(f"{SL.case_id(cid)}: {nd} doubtful of {nf} frames, {int(c.skip.sum())} of {c.skip.size} blocks left out")
    assert nd <= SL.doubt_cap(nf), (nd, nf)
    assert int(c.skip.sum()) <= nd * c.G * (SL.halo_of(c.N, c.hs) + 1)
    assert not np.any(c.skip & (c.L == 0))


@pytest.mark.parametrize("cid", SL.SCALING_CASES, ids=SL.case_id)
def test_scaling_by_a_power_of_two_is_exact_in_the_model(cid):
    """The conditions of the GPU scaling test, from the model: with the input scaled by 2^+-20 every value a kernel rounds to float32 stays in the normal range, and
    the model itself scales bit for bit (its phases are equal: the doubtful flags and the output of the scaled runs are those of the unscaled one)."""
    c = SL.case(*cid)
    lo, hi = SL.scaling_conditions(c, (-20, 0, 20))
    print(f"{SL.case_id(cid)}: smallest {lo:.3e}, largest {hi:.3e}")
    assert float(np.finfo(np.float32).tiny) <= lo and hi < float(np.finfo(np.float32).max)
    for k in (-20, 20):
        y, raw = SL.reference(c.family, c.N, c.ha, c.hs, np.ldexp(c.x, k), c.hops, c.resets)
        assert np.array_equal(_bits(y), _bits(np.ldexp(c.ref, k))), k
        assert np.array_equal(raw, c.doubt_raw), k
