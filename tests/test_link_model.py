"""CPU checks of the linked-channel model (tests/link_model.py): G = 1 is the unlinked model bit for bit, a group of identical channels is the mono
output bit for bit, the sum of a group's outputs is the mono stretch of its mix, the inter-channel phase of steady partials is kept (the unlinked
model scales it by hs / ha), and an anti-phase pair is silent."""
import numpy as np
import pytest

import signals as S
import tones as TN
from link_model import LinkModel, mix, phase_fit, stereo_partials, wrap
from stretch_model import StretchModel
from tempo_model import TempoModel, schedule


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def _noise(nch, n, seed=0):
    return np.stack([S.lcg_noise(seed + 17 * c + 1, n, 0.5) for c in range(nch)]).astype(np.float32)


@pytest.mark.parametrize("N,ha,hs", [(256, 64, 80), (512, 128, 96), (1024, 256, 320)])
def test_one_channel_groups_are_the_unlinked_model(N, ha, hs):
    T = 40
    x = _noise(3, T * ha)
    y = LinkModel(N, ha, hs, 3, 1).process(x)
    ref = StretchModel(N, ha, hs, 3).process(x)
    assert np.array_equal(y.view(np.uint32), ref.view(np.uint32))
    hops = schedule("random", ha, N, T, seed=3)
    xs = _noise(3, int(hops.sum()), seed=5)
    ys = LinkModel(N, ha, hs, 3, 1).process_hops(xs, hops)
    rs = TempoModel(N, ha, hs, 3).process_hops(xs, hops)
    assert np.array_equal(ys.view(np.uint32), rs.view(np.uint32))


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("kind", ["noise", "tonal"])
def test_identical_channels_give_the_mono_output(G, kind):
    """The mix is exactly G x (G a power of two), and every step up to q and the peak flags is invariant under that scale."""
    N, ha, hs, T = 512, 128, 160, 40
    one = (S.make_signal(kind, 0, T * ha) if kind == "tonal" else _noise(1, T * ha)[0])[None, :]
    y = LinkModel(N, ha, hs, 2 * G, G).process(np.repeat(one, 2 * G, axis=0))
    ref = StretchModel(N, ha, hs).process(one)[0]
    for c in range(2 * G):
        assert np.array_equal(y[c].view(np.uint32), ref.view(np.uint32)), c


def _panned(N, n, nch, seed=0):
    """Two partials with a different gain and phase in every channel."""
    rng = np.random.default_rng(seed)
    f = [round(N * 0.0629) + 0.37, round(N * 0.15) + 0.81]
    amps = rng.uniform(0.1, 0.5, (nch, 2))
    ph = rng.uniform(0, 0.5, (nch, 2)) + np.arange(nch)[:, None] * np.array([1.6, 2.3])     # channel offsets well away from 0 (mod 2 pi)
    return stereo_partials(N, f, amps, ph, n), f, amps, ph


@pytest.mark.parametrize("G,kind", [(2, "partials"), (3, "noise"), (8, "noise"), (8, "partials")])
def test_downmix_is_the_mono_stretch_of_the_mix(G, kind):
    N, ha, hs, T = 1024, 256, 320, 96
    x = _panned(N, T * ha, G)[0] if kind == "partials" else _noise(G, T * ha, seed=G)
    u = mix(x, G)
    mono = StretchModel(N, ha, hs).process(u)[0]
    y = LinkModel(N, ha, hs, G, G).process(x)
    unl = StretchModel(N, ha, hs, G).process(x)
    linked = _rel(y.astype(np.float64).sum(axis=0), mono)
    unlinked = _rel(unl.astype(np.float64).sum(axis=0), mono)
    assert linked <= 1e-6, (linked, unlinked)
    assert unlinked > 0.1, (linked, unlinked)                          # the check discriminates


@pytest.mark.parametrize("N,ha,hs", [(1024, 256, 320), (2048, 512, 256)])
def test_inter_channel_phase_of_steady_partials_is_kept(N, ha, hs):
    lo, _ = TN.steady_range(N, ha, hs, 0)
    T = -(-(lo + 9 * N) // hs)
    x, f, amps, ph = _panned(N, T * ha, 2, seed=1)
    dphi_in = wrap(ph[1] - ph[0])
    y = LinkModel(N, ha, hs, 2, 2).process(x)
    p = phase_fit(y, N, ha, hs, f)
    err = np.abs(wrap(p[1] - p[0] - dphi_in))
    assert err.max() <= 1e-7, err
    # amplitude ratios between the channels are kept as well
    r = [TN.tone_fit(y[c], N, ha, hs, f, amps[c])[0] for c in range(2)]
    assert np.max(np.abs(r[1] / r[0] - 1)) <= 1e-6, r
    # the unlinked model scales the difference by hs / ha
    pu = phase_fit(StretchModel(N, ha, hs, 2).process(x), N, ha, hs, f)
    eu = wrap(pu[1] - pu[0] - dphi_in)
    assert np.allclose(np.abs(eu), np.abs(wrap((hs / ha - 1) * dphi_in)), atol=1e-4), (eu, dphi_in)
    assert np.abs(eu).max() > 0.1


def test_anti_phase_pair_is_silent():
    """L = -R: the mix is zero, it has no peak, and every frame of the group is silent (the limit of a sum reference)."""
    N, ha, hs, T = 512, 128, 160, 24
    one = S.make_signal("tonal", 0, T * ha)
    x = np.stack([one, -one])
    m = LinkModel(N, ha, hs, 2, 2)
    y = m.process(x)
    assert not np.any(y) and all(m.peakless[0])
    assert np.any(StretchModel(N, ha, hs, 2).process(x))


def test_schedules_and_groups_beside_groups():
    """Two stereo groups under one shared schedule: each group is its own two-channel model, and its phases are the mono model's on its mix."""
    N, ha, hs, T = 512, 96, 160, 40
    hops = schedule("random", ha, N, T, seed=7)
    x = _noise(4, int(hops.sum()), seed=11)
    m = LinkModel(N, ha, hs, 4, 2)
    y = m.process_hops(x, hops)
    for g in range(2):
        mg = LinkModel(N, ha, hs, 2, 2)
        assert np.array_equal(mg.process_hops(x[2 * g:2 * g + 2], hops).view(np.uint32), y[2 * g:2 * g + 2].view(np.uint32))
        mono = TempoModel(N, ha, hs)
        mono.process_hops(mix(x[2 * g:2 * g + 2], 2), hops)
        assert np.array_equal(mono.phi[0], m.phi[g]) and np.array_equal(mono.psi[0], m.psi[g])
