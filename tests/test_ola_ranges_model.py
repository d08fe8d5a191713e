"""The far ends of the position and sample ranges of the overlap-add path on the CPU: what tests/test_gpu_ola_ranges.py asks of the kernels, asked first of
the models (tests/psola_model.py, tests/tsm_model.py) and of a plain float32 restatement of the kernel arithmetic (tests/ola_f32.py).

1. TRANSLATION.  Shifting a far table by K (t += K, D += K, out_first = K) changes no input position n - D: check_grains and check_span accept it, tiles()
   gives the same grain ranges and source ranges, and TM.process returns the same y and tol EXACTLY, for K up to K_far = 2^30 - 1 - max(t, D, NOUT).  The
   same for psola_model with the input placed at [K, K + n) of a longer buffer.
2. SMALL MAGNITUDES.  With the input scaled by 2^-125 (normal samples, subnormal products) and 2^-140 (everything subnormal) the restatement stays within
   tol(subnormal="derived") on every sample; with subnormal numbers flushed it does not; and at 2^-140 at least a third of the covered outputs have
   |y| > 4 tol, so the gate cannot pass by being loose.
3. SCALING CONDITIONS under which y(2^k x) == 2^k y(x) bit for bit (ola_f32.scaling_conditions), asserted from the model and the tables."""
import numpy as np
import pytest

import ola_f32 as OF
import psola_model as PM
import test_gpu_psola as TGP
import test_gpu_tsm as TGT
import tsm_model as TM

NOUT = TGT.NOUT
KS = (1, 1023, (1 << 20) + 17)
TSM_SMALL = ("small", "tiny", "slow")
PSOLA_SMALL = ("tiny", "voice")
SMALL_SCALES = (-125, -140)
TSM_SCALED = ("small", "big", "slow")
PSOLA_SCALED = ("tiny", "alternate", "voice")
SCALE_KS = (-20, 20, 100)


def k_far(g):
    """The largest shift of a far table that keeps centres, displacements and the call's last output below 2^30."""
    g = np.asarray(g, np.int64).reshape(-1, 4)
    return (1 << 30) - 1 - int(max([NOUT] + g[:, 0].tolist() + g[:, 2].tolist()))


def shifted(g, K):
    """The far table g moved by K outputs: it reads the same input."""
    s = np.array(g, np.int64).reshape(-1, 4)
    s[:, 0] += K
    s[:, 2] += K
    return np.ascontiguousarray(s, np.int32)


def psola_shifted(g, K):
    """The psola table g moved by K: with the input moved by K as well it reads the same samples."""
    s = np.array(g, np.int64).reshape(-1, 4)
    s[:, 0] += K
    return np.ascontiguousarray(s, np.int32)


def tsm_input(name):
    """(max_period, max_rate, far grains, x) of a table of test_gpu_tsm, the input of its case()."""
    mp, R, nin, g = TGT._grains(name)
    return mp, R, g, TGT._signals(nin, 7 + len(name))


def psola_input(name):
    mp, n, g = TGP._grains(name)
    return mp, g, TGP._signals(n, 7 + len(name))


def scaled(x, k):
    """2^k x in float32, rounded where it is subnormal."""
    y = np.ldexp(x, k)
    assert y.dtype == np.float32
    return y


def scaling_tables():
    """(x, far grains, NOUT) of the six tables whose outputs must scale exactly."""
    out = []
    for name in PSOLA_SCALED:
        _, g, x = psola_input(name)
        out.append((x, TM.from_psola(g), NOUT))
    for name in TSM_SCALED:
        _, _, g, x = tsm_input(name)
        out.append((x, g, NOUT))
    return out


_COND = {}


def scaling_conditions():
    if not _COND:
        _COND.update(OF.scaling_conditions(scaling_tables()))
    return _COND


# ---- 1. translation -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", TGT.CASES)
def test_a_shifted_far_table_gives_the_models_output_and_bound_exactly(name):
    mp, R, g, x = tsm_input(name)
    y0, tol0, p0 = TM.process(x, g, 0, NOUT, bound=True)
    tiles0 = TM.tiles(g, mp, 0, NOUT)
    far = k_far(g)
    assert far > (1 << 30) - (1 << 20)
    print(f"{name}: K_far = 2^30 - {(1 << 30) - far}, {'odd' if far & 1 else 'even'}")
    for K in KS + (far,):
        s = shifted(g, K)
        assert TM.check_grains(s, mp) is None and TM.check_span(s, mp, R, K, NOUT) is None
        assert np.array_equal(TM.tiles(s, mp, K, NOUT), tiles0)                                  # the same grain ranges, src0 and src_count
        y, tol, p = TM.process(x, s, K, NOUT, bound=True)
        assert np.array_equal(y, y0) and np.array_equal(tol, tol0) and np.array_equal(p, p0), K


@pytest.mark.parametrize("name", TGP.CASES)
def test_a_psola_table_moved_with_its_input_gives_the_models_output_and_bound_exactly(name):
    mp, g, x = psola_input(name)
    y0, tol0, _ = PM.process(x, g, 0, NOUT, bound=True)
    for K in KS:
        xk = np.zeros((x.shape[0], K + x.shape[1]), np.float32)
        xk[:, K:] = x
        s = psola_shifted(g, K)
        assert PM.check_grains(s, mp) is None
        y, tol, _ = PM.process(xk, s, K, NOUT, bound=True)
        assert np.array_equal(y, y0) and np.array_equal(tol, tol0), K


# ---- 2. small magnitudes ------------------------------------------------------------------------------------------------------------------------

def small_case(kind, name, k):
    """(max_period, max_rate or None, far grains, the table as its handle takes it, the input scaled by 2^k)."""
    if kind == "tsm":
        mp, R, g, x = tsm_input(name)
        far = g
    else:
        mp, g, x = psola_input(name)
        R, far = None, TM.from_psola(g)
    xs = scaled(x, k)
    return mp, R, far, g, xs


SMALL_CASES = [("tsm", n) for n in TSM_SMALL] + [("psola", n) for n in PSOLA_SMALL]


@pytest.mark.parametrize("k", SMALL_SCALES)
@pytest.mark.parametrize("kind,name", SMALL_CASES)
def test_the_f32_restatement_meets_the_derived_bound_in_the_subnormal_range_and_a_flushing_one_does_not(kind, name, k):
    mp, R, far, g, xs = small_case(kind, name, k)
    ax = np.abs(xs[xs != 0])
    if k == -125:
        assert np.median(ax) >= 2.0 ** -126                                                    # the samples are normal, their products are not
    else:
        assert ax.max() < 2.0 ** -126                                                          # everything is subnormal
    y, tol, poisoned, G, den = TM.process(xs, far, 0, NOUT, bound=True, subnormal="derived")
    if kind == "psola":                                                                       # the two models agree on the term
        yp, tolp, _, Gp, denp = PM.process(xs, g, 0, NOUT, bound=True, subnormal="derived")
        assert np.array_equal(yp, y) and np.array_equal(tolp, tol) and np.array_equal(Gp, G) and np.array_equal(denp, den)
    covered = G > 0
    assert covered.sum() > NOUT // 2 and not poisoned.any()
    # never above the hand count 2^-150 (G / D + 67), which takes |d_g| >= 1
    y1, tol1, _ = TM.process(xs, far, 0, NOUT, bound=True)
    sub = tol[:, covered] - (tol1[:, covered] - 2.0 ** -149 * (1.0 + (G[covered] + 3 + 64) / den[covered]))
    assert np.all(sub <= 2.0 ** -150 * (G[covered] / den[covered] + 67.0) * (1 + 1e-9))
    got = OF.process(xs, far, 0, NOUT)
    err = np.abs(got.astype(np.float64) - y)
    worst = float(np.max(err[:, covered] / tol[:, covered]))
    strong = float(np.mean(np.abs(y[:, covered]) > 4.0 * tol[:, covered]))
    print(f"{kind} {name} 2^{k}: worst |err| / tol = {worst:.3f}, max |err| = {err.max():.3e} = {err.max() * 2.0 ** 149:.2f} * 2^-149, |y| > 4 tol on {strong:.2f} of the covered outputs")
    assert np.all(err <= tol), (k, int(np.sum(err > tol)), worst)                              # no sample left out
    assert np.all(got[:, ~covered] == 0.0) and not np.any(np.signbit(got[:, ~covered]))
    if k == -140:
        assert strong >= 1.0 / 3.0, strong
    flushed = OF.process(xs, far, 0, NOUT, flush=True)
    ferr = np.abs(flushed.astype(np.float64) - y)
    print(f"    flushed: {int(np.sum(ferr > tol))} samples beyond tol, worst |err| / tol = {float(np.max(ferr[:, covered] / tol[:, covered])):.1f}")
    assert np.any(ferr > tol)


def test_the_restatement_is_within_the_bound_at_ordinary_amplitudes_too():
    """The restatement is the kernels' arithmetic: at O(1) it stays within the default bound that the GPU tests use."""
    for kind, name in (("tsm", "small"), ("psola", "tiny")):
        mp, R, far, g, x = small_case(kind, name, 0)
        y, tol, _ = TM.process(x, far, 0, NOUT, bound=True)
        err = np.abs(OF.process(x, far, 0, NOUT).astype(np.float64) - y)
        print(f"{kind} {name}: worst |err| / tol = {float(np.max(err[tol > 0] / tol[tol > 0])):.3f}")
        assert np.all(err <= tol)


# ---- 3. the conditions of exact scaling ---------------------------------------------------------------------------------------------------------

def test_the_conditions_of_exact_power_of_two_scaling_hold():
    c = scaling_conditions()
    print({k: (f"{v:.4g}" if isinstance(v, float) else v) for k, v in c.items()})
    assert c["smallest"] * 2.0 ** -20 >= 2.0 ** -126
    assert c["largest"] * 2.0 ** c["k_top"] < 2.0 ** 128 <= c["largest"] * 2.0 ** (c["k_top"] + 1)
    assert c["k_top"] >= 120
    # the restatement itself scales exactly at the two ends of what the device is asked for
    x, g, nout = scaling_tables()[0]
    base = OF.process(x, g, 0, nout)
    for k in (SCALE_KS[0], c["k_top"]):
        assert np.array_equal(OF.process(scaled(x, k), g, 0, nout).view(np.uint32), np.ldexp(base, k).view(np.uint32)), k
