"""Parity at level for the time stretch, GPU side: every output block of hs samples of every channel of the stretch kernels (every pv_stretch_pass_a / pass_b family:
fixed hop, schedule, resets, linked) against the fp64 models at that block's own level L(c, b) (tests/stretch_level_model.py: the largest rms of the windowed input
frames whose overlap-add reaches the block), on signals with dynamics -- a fade to -140 dB and back, a burst followed by digital silence and a -100 dB tone, a -100 dB
channel next to a full-scale one, the same 2^20 up and down, one partial over a -110 dB floor.  Each stream has at least three chains, with a chain boundary inside the
quiet stretch of `fade` and one inside the silence of `burst`; the fixed hop also runs cut into three calls, one cut in that silence and one at the bottom of the fade.

The gate is 4 x the figures the float32 restatement of the synthesis half reaches against the models on the CPU (stretch_level_model.RESTATEMENT_FIGURES, pinned and
reproduced by tests/test_stretch_level_model.py); it is never fitted to a kernel.  Blocks that a doubtful non-silent frame reaches are left out, as
test_gpu_stretch_edges.block_gate does; the model alone counts those frames, at most 1 % of a case's frames plus one.  Every block with L == 0 must be exactly 0.
Scaling the input by 2^+-20 must scale the output, hist and acc bit for bit and leave phi and psi alone.  Each test prints the worst rms / L and max / L it saw and
attaches them with record_property (DESIGN.md section 8 records them)."""
import numpy as np
import pytest

import stretch_level_model as SL
from test_gpu_stretch_families import _one_launch

pytestmark = pytest.mark.gpu

FIXED = [c for c in SL.case_list() if c[0] == "fixed"]
FAMILY = [c for c in SL.case_list() if c[0] != "fixed"]
SCALING = SL.SCALING_CASES
QUIET = 1e-4                                                                  # the quiet stretch of a fade: blocks 80 dB or more under the channel's loudest


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _handle(c):
    import phaze_amd
    return phaze_amd.TimeStretch(c.N, c.ha, c.hs, max_channels=c.nch, max_frames=c.T, channels_per_group=c.G)


def _run(ts, c, x):
    """The whole stream in one launch."""
    if c.hops is None:
        return ts.process(x)
    return _one_launch(ts, np.array(x), c.hops, c.resets)                      # (a writable copy: the corpus is read-only)


def _layout(ts, c):
    """The chains of the one-launch form, from the handle: at least three, one boundary inside the quiet stretch of a fade, one inside the silence of burst."""
    F, halo = ts.chain_layout(c.nch, c.T)
    assert halo == SL.halo_of(c.N, c.hs)
    starts = np.arange(F, c.T, F)
    assert starts.size >= 2, (F, c.T, "fewer than three chains")
    if c.signal in ("fade", "scaled_up", "scaled_down"):
        assert np.any(np.all(c.L[:, starts] <= QUIET * c.L.max(axis=1, keepdims=True), axis=0)), (F, "no chain starts in the quiet stretch of the fade")
    if c.signal == "burst":
        assert np.any(np.all(c.L[:, starts] == 0, axis=0)), (F, c.B, "no chain starts inside the silence of burst")
    return F, starts.size + 1


def _hold(c, y, form, record_property):
    """Every block of every channel of y at the gate of its N; none left out but those a doubtful non-silent frame reaches."""
    k_rms, k_max = SL.gate(c.N)
    assert np.all(np.isfinite(y)), (SL.case_id(c.id), form)
    assert SL.zero_blocks_exact(y, c.L, c.hs), (SL.case_id(c.id), form, "a block with L == 0 is not exactly 0")
    fails, (wr, wm) = SL.block_failures(y, c.ref, c.L, c.hs, k_rms, k_max, c.skip)
    left_out = int(c.skip.sum())
    print(f"stretch level {SL.case_id(c.id)} {form}: worst rms/L {wr:.3e} (gate {k_rms:.2e})  max/L {wm:.3e} (gate {k_max:.2e})  "
          f"blocks left out {left_out} of {c.skip.size}")
    record_property(f"{form}_rms_over_L", wr)
    record_property(f"{form}_max_over_L", wm)
    assert not fails, (SL.case_id(c.id), form, f"{len(fails)} blocks miss the gate; (channel, block, rms/L, max/L):", fails[:6])


def _case(cid, record_property):
    c = SL.case(*cid)
    c.id = cid
    nd, nf = SL.doubt_count(c)
    assert nd <= SL.doubt_cap(nf), (nd, nf)                                   # a condition on the input, from the model alone (the CPU test holds it too)
    record_property("frames", c.T)
    record_property("doubtful", nd)
    return c


@pytest.mark.parametrize("cid", FIXED, ids=SL.case_id)
def test_fixed_hop_every_block_at_its_own_level(cid, record_property):
    """TimeStretch.process in one call, and the same stream cut into three calls (inside the silence of burst, at the bottom of fade): the three calls give the bits of
    the one call, and both are held to the gate."""
    c = _case(cid, record_property)
    ts = _handle(c)
    try:
        F, chains = _layout(ts, c)
        record_property("chains", chains)
        one = _run(ts, c, c.x)
        _hold(c, one, "one_call", record_property)
        ts.reset()
        three = np.concatenate([ts.process(c.x[:, a * c.ha:b * c.ha]) for a, b in zip(c.cuts[:-1], c.cuts[1:])], axis=1)
        assert np.array_equal(_bits(three), _bits(one)), (cid, "three calls differ from one", c.cuts)
        _hold(c, three, "three_calls", record_property)
    finally:
        ts.close()


@pytest.mark.parametrize("cid", FAMILY, ids=SL.case_id)
def test_families_every_block_at_their_own_level(cid, record_property):
    """A random schedule in [floor, N] against TempoModel; the same with resets on the first frame after the silence and at the bottom of the fade against
    TransientModel; linked groups against LinkModel, G = 3 at the fixed hop (the -100 dB channel rotated by the angles the full-scale one sets) and G = 2 on the
    schedule.  L is per channel from the channel's own frames; doubt is judged on the mix."""
    c = _case(cid, record_property)
    ts = _handle(c)
    try:
        F, chains = _layout(ts, c)
        record_property("chains", chains)
        y = _run(ts, c, c.x)
        _hold(c, y, "one_launch", record_property)
    finally:
        ts.close()


@pytest.mark.parametrize("cid", SCALING, ids=SL.case_id)
def test_a_power_of_two_scales_the_output_bit_for_bit(cid, record_property):
    """process(ldexp(x, k)) == ldexp(process(x), k) for k = +-20, bit for bit; the exported phi and psi are equal, hist and acc scaled.  A power of two commutes with the
    f32 window product, the fp64 forward and fp32 inverse transforms, the f32 squared magnitudes, the peak decisions and the integer phases, as long as nothing leaves
    the float32 normal range: the model says so first."""
    c = _case(cid, record_property)
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    lo, hi = SL.scaling_conditions(c, (-20, 0, 20))
    assert tiny <= lo and hi < huge, (lo, hi)
    ts = _handle(c)
    try:
        runs = {}
        for k in (0, -20, 20):
            ts.reset()
            y = _run(ts, c, np.ldexp(c.x, k))
            runs[k] = (y, [ts.export_state(s) for s in range(c.nch)])
        y0, st0 = runs[0]
        _hold(c, y0, "unscaled", record_property)
        nz = np.abs(y0[y0 != 0])
        assert nz.min() * 2.0 ** -20 >= tiny and nz.max() * 2.0 ** 20 < huge
        for k in (-20, 20):
            y, st = runs[k]
            for s in range(c.nch):
                (hist0, acc0, phi0, psi0), (hist, acc, phi, psi) = st0[s], st[s]
                dphi = np.flatnonzero(phi != phi0)
                assert dphi.size == 0, (cid, k, s, "phi differs", dphi[:8], phi[dphi[:8]], phi0[dphi[:8]])
                dpsi = np.flatnonzero(psi != psi0)
                assert dpsi.size == 0, (cid, k, s, "psi differs", dpsi[:8])
                assert np.array_equal(_bits(hist), _bits(np.ldexp(hist0, k))), (cid, k, s, "hist")
                assert np.array_equal(_bits(acc), _bits(np.ldexp(acc0, k))), (cid, k, s, "acc")
            bad = np.argwhere(_bits(y) != _bits(np.ldexp(y0, k)))
            print(f"stretch scaling {SL.case_id(cid)} k={k}: {bad.shape[0]} of {y.size} output samples differ")
            record_property(f"differing_samples_k{k}", int(bad.shape[0]))
            assert bad.shape[0] == 0, (cid, k, "first differing (channel, sample):", bad[:4].tolist())
    finally:
        ts.close()
