"""CPU checks of the variable-tempo model (tests/tempo_model.py) that the GPU kernels are held to, and of phaze_amd.tempo_hops.

A schedule of per-frame analysis hops must reduce to the fixed-hop model (tests/stretch_model.py) wherever it is constant, chain like fixed-hop handles
handed over through their state, keep the closed form of stationary tones (tests/tones.py) under any schedule, and place every frame's window where
its prefix sum says: input that switches signal at sample P shows the new signal only in output written by frames whose windows reach P."""
import numpy as np
import pytest

import tones as TN
from stretch_model import StretchModel
from tempo_model import TONE_SHAPES, TONE_SHAPES_EDGES, TempoModel, positions, schedule, switch_bounds, tone_schedule_input


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _noise(n, seed):
    return (np.random.default_rng(seed).standard_normal(n) * 0.3).astype(np.float32)


# ---- the schedule against the fixed hop, bit for bit ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,floor,c,hs", [(256, 48, 64, 80), (1024, 205, 256, 320), (1024, 1, 300, 256), (2048, 256, 512, 640), (512, 100, 512, 97)])
def test_constant_schedule_is_the_fixed_hop_model(N, floor, c, hs):
    """Every hop c > floor: from zero state the windows are those of a handle created with analysis_hop = c, and so is every bit."""
    T = 40
    x = _noise(T * c, N + c)[None, :]
    tm = TempoModel(N, floor, hs)
    y = tm.process_hops(x, np.full(T, c))
    fm = StretchModel(N, c, hs)
    ref = fm.process(x)
    assert np.array_equal(_bits(y), _bits(ref))
    assert np.array_equal(tm.phi[0], fm.phi[0]) and np.array_equal(tm.psi[0], fm.psi[0]) and np.array_equal(_bits(tm.acc[0]), _bits(fm.acc[0]))
    assert np.array_equal(_bits(tm.hist[0][-(N - c):] if c < N else tm.hist[0][:0]), _bits(fm.hist[0]))
    assert tm.hist[0].size == N - floor


def _chained(N, hs, segments, x):
    """Fixed-hop models run one after the other, each taking acc / phi / psi from the one before; hist is rebuilt from the stream (zeros ++ x), since a
    handle with a larger hop holds fewer samples of history than the next one needs."""
    stream = np.concatenate([np.zeros(N, np.float32), x])
    out, prev, at = [], None, 0
    for c, T in segments:
        m = StretchModel(N, c, hs)
        if prev is not None:
            m.acc[0], m.phi[0], m.psi[0] = prev.acc[0], prev.phi[0], prev.psi[0]
        m.hist[0] = stream[N + at - (N - c):N + at]
        out.append(m.process(x[None, at:at + T * c]))
        at += T * c
        prev = m
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("N,floor,hs,c1,c2", [(256, 32, 80, 40, 128), (256, 32, 80, 128, 40), (1024, 205, 320, 205, 320), (1024, 205, 320, 320, 205),
                                              (2048, 100, 512, 1024, 2048), (2048, 100, 512, 2048, 101), (8192, 1024, 2048, 1024, 3000)])
def test_step_schedule_is_two_chained_fixed_models(N, floor, hs, c1, c2):
    T1, T2 = 17, 19
    x = _noise(T1 * c1 + T2 * c2, N + c1 + c2)
    y = TempoModel(N, floor, hs).process_hops(x[None, :], np.array([c1] * T1 + [c2] * T2))
    ref = _chained(N, hs, [(c1, T1), (c2, T2)], x)
    assert np.array_equal(_bits(y), _bits(ref))


def test_all_floor_schedule_is_process():
    N, floor, hs, T = 1024, 256, 320, 30
    x = _noise(T * floor, 3)[None, :]
    a = TempoModel(N, floor, hs)
    assert np.array_equal(_bits(a.process_hops(x, np.full(T, floor))), _bits(StretchModel(N, floor, hs).process(x)))
    b = TempoModel(N, floor, hs)                                     # and process() on the tempo model is that schedule
    assert np.array_equal(_bits(b.process(x)), _bits(StretchModel(N, floor, hs).process(x)))


# ---- stationary tones under any schedule --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ramp", "random", "alt"])
@pytest.mark.parametrize("sid", list(TONE_SHAPES) + list(TONE_SHAPES_EDGES))
def test_tones_closed_form_under_schedules(sid, kind):
    """The synthesis phase of a steady partial advances by f hs / N per frame whatever ha_m is, so the fixed-hop gate of 3e-6 holds: also at the hop
    edges (halo 1 .. 255, hs = 1, hs = N / 2, hops that divide nothing)."""
    N, floor, hs, freqs, amps = {**TONE_SHAPES, **TONE_SHAPES_EDGES}[sid]
    TN.check_partials(N, freqs)
    hops, x = tone_schedule_input(N, floor, hs, freqs, amps, kind)
    y = TempoModel(N, floor, hs).process_hops(x[None, :], hops)[0]
    ratio, res = TN.tone_fit(y, N, floor, hs, freqs, amps)
    assert np.all(np.abs(ratio - 1.0) <= 3e-6), ratio
    assert res <= 3e-6, res


# ---- the time map -------------------------------------------------------------------------------------------------------------------------------------

def switch_input(N, f1, f2, P, n):
    """0.5 cos at f1 bins before sample P, 0.5 cos at f2 bins from P on (float32[n])."""
    k = np.arange(n, dtype=np.float64)
    return np.where(k < P, 0.5 * np.cos(2 * np.pi * f1 * k / N + 0.4), 0.5 * np.cos(2 * np.pi * f2 * k / N + 1.3)).astype(np.float32)


def amplitudes(y, N, hs, lo, hi, freqs):
    """Fitted amplitude of each partial (under the envelope g) over y[lo, hi)."""
    g = TN.envelope(N, hs, y.size)[lo:hi]
    k = np.arange(lo, hi, dtype=np.float64)
    B = np.stack([c for f in freqs for c in (g * np.cos(2 * np.pi * f * k / N), g * np.sin(2 * np.pi * f * k / N))], axis=1)
    coef, *_ = np.linalg.lstsq(B, np.asarray(y[lo:hi], np.float64), rcond=None)
    return np.hypot(coef[0::2], coef[1::2])


# Measured on the model: the other partial's amplitude is <= 2e-8 of 0.5 on either side of the bounds and its own within 3.3e-8 of 0.5.  With either
# bound moved one synthesis hop into the transition, the other partial already reads 2.7e-7 .. 6.3e-4 (and 1.7e-3 .. 1.4e-2 at N / 2 for one side).
SWITCH_GATE = 1e-7


def time_map_check(y, N, hs, S, P, f1, f2):
    """(f2 share before the first bound, f1 share after the second, the own partial's amplitude error on each side).  Each side is measured over at
    least 2 N output samples past the onset and before the last N."""
    b1, b2 = switch_bounds(S, N, hs, P)
    lo, _ = TN.steady_range(N, 1, hs, 0)
    lo = min(lo, b1 - 2 * N)
    hi = y.size - N
    assert b1 - lo >= 2 * N and hi - b2 >= 2 * N, (lo, b1, b2, hi)
    a = amplitudes(y, N, hs, lo, b1, [f1, f2]) / 0.5
    b = amplitudes(y, N, hs, b2, hi, [f1, f2]) / 0.5
    return float(a[1]), float(b[0]), float(max(abs(a[0] - 1), abs(b[1] - 1)))


@pytest.mark.parametrize("N,floor,hs,kind", [(1024, 205, 320, "ramp"), (1024, 64, 256, "random"), (2048, 256, 512, "alt"), (256, 16, 64, "random")])
def test_time_map_follows_the_prefix_sums(N, floor, hs, kind):
    f1, f2 = N * 0.0629 + 0.37, N * 0.15 + 0.21
    T = 24 * N // hs + 40
    hops = schedule(kind, floor, N, T, seed=N)
    S = positions(hops)
    P = int(S[T // 2]) + 37
    x = switch_input(N, f1, f2, P, int(S[-1]))
    y = TempoModel(N, floor, hs).process_hops(x[None, :], hops)[0]
    f2_before, f1_after, own = time_map_check(y, N, hs, S, P, f1, f2)
    assert f2_before <= SWITCH_GATE and f1_after <= SWITCH_GATE, (f2_before, f1_after)
    assert own <= 1e-6, own                                          # each side does hold its own partial (the gain ripple of g is in the basis)


def test_time_map_gate_sees_a_misplaced_window():
    """The same gate on a model whose windows sit at (m + 1) floor - N, the fixed hop's place (hops kept in the advance), fails: the gate is not vacuous."""
    N, floor, hs = 1024, 205, 320
    f1, f2 = N * 0.0629 + 0.37, N * 0.15 + 0.21
    T = 24 * N // hs + 40
    hops = schedule("ramp", floor, N, T)
    S = positions(hops)
    P = int(S[T // 2]) + 37
    x = switch_input(N, f1, f2, P, int(S[-1]))
    stream = np.concatenate([np.zeros(2 * N, np.float32), x])
    tm = TempoModel(N, floor, hs)
    ys = []
    for m in range(T):
        e, h = 2 * N + (m + 1) * floor, int(hops[m])
        tm.hist[0] = stream[e - h - (N - floor):e - h]                # frame m's window becomes stream[e - N, e)
        ys.append(tm.frame(0, stream[e - h:e]))
    f2_before, f1_after, _ = time_map_check(np.concatenate(ys), N, hs, S, P, f1, f2)
    assert max(f2_before, f1_after) > 100 * SWITCH_GATE, (f2_before, f1_after)


# ---- tempo_hops ---------------------------------------------------------------------------------------------------------------------------------------

def test_tempo_hops_range_drift_and_carry():
    import phaze_amd
    hs, lo, hi = 320, 205, 1024
    rng = np.random.default_rng(7)
    tempo = np.concatenate([np.linspace(lo / hs, 1.0, 300), rng.uniform(lo / hs, hi / hs, 500), np.full(100, 1.25), np.full(50, hi / hs)])
    hops, carry = phaze_amd.tempo_hops(tempo, hs, lo, hi)
    assert hops.dtype == np.int32 and hops.shape == tempo.shape
    assert hops.min() >= lo and hops.max() <= hi
    drift = np.cumsum(hops.astype(np.int64)) - np.cumsum(tempo * hs)
    assert np.max(np.abs(drift)) <= 0.5 + 1e-9, np.max(np.abs(drift))                # within one sample at every frame (half, by rounding)
    assert abs(carry + drift[-1]) <= 1e-6                                              # the carry is what the hops still owe
    assert np.all(hops[800:900] == 400)                                                # tempo 1.25 at hs 320
    # cut anywhere: continuing with the carry gives the same hops as one call
    for cut in (1, 299, 301, 777):
        a, ca = phaze_amd.tempo_hops(tempo[:cut], hs, lo, hi)
        b, cb = phaze_amd.tempo_hops(tempo[cut:], hs, lo, hi, carry=ca)
        assert np.array_equal(np.concatenate([a, b]), hops) and cb == carry, cut
    h1, c1 = phaze_amd.tempo_hops(1.0, 256, 256, 256)
    assert h1.tolist() == [256] and c1 == 0.0
    with pytest.raises(ValueError):
        phaze_amd.tempo_hops([0.5], hs, lo, hi)                                        # 160 samples: below the floor
    with pytest.raises(ValueError):
        phaze_amd.tempo_hops([4.0], hs, lo, hi)                                        # above N
