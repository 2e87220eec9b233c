"""tests/ssim_emul.py -- the numpy restatement of the SSIM / MS-SSIM definition of include/rcb.h (N4, 414) that rcb_ssim is held to
bit for bit -- against an INDEPENDENT evaluation: scipy.signal.correlate2d with the 11 x 11 outer-product window (no
separability, another order of additions), direct means, reshape-sums.  Every check is a named function of an evaluator, so that
the mutants at the end -- the evaluator with one step broken -- each show which check notices.

The per-position bound 1e-10: two fp64 evaluation orders of the filters differ by about 24 * 2^-53 * L^2 / C2 = 3e-12 through the
cancellation in the variances; a wrong tap, constant or normalisation moves values by 1e-4 or more."""
import math

import numpy as np
import pytest
from scipy.signal import correlate2d

import ssim_emul as E

from recombiner_amd import utils

DEPTH_L = [255, 511, 4095, 65535]
FAMILIES = ["noise", "smooth", "complement", "rows"]


def family(name, L, shape=(24, 29, 2), seed=0):
    """the four input families -> integer arrays (a, b) of `shape` with values in 0 .. L"""
    rng = np.random.default_rng(seed)
    H, W, C = shape
    if name == "noise":
        return rng.integers(0, L + 1, shape), rng.integers(0, L + 1, shape)
    if name == "smooth":
        yy, xx, cc = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
        a = np.rint(L * (0.5 + 0.4 * np.sin(yy / 7.0 + cc) * np.cos(xx / 5.0))).astype(np.int64)
        return a, np.clip(a + rng.integers(-3, 4, shape), 0, L)
    if name == "complement":
        a = rng.integers(0, 2, shape) * L
        return a, L - a
    if name == "rows":
        b = np.full(shape, L, dtype=np.int64)
        b[1::2] -= 1
        return np.full(shape, L, dtype=np.int64), b
    raise ValueError(name)


def independent_maps(a, b, L):
    """(ssim, cs) per position by a full 2-D correlation with the outer-product window"""
    g = np.array([math.exp(-((k - 5) ** 2) / 4.5) for k in range(11)])
    w2 = np.outer(g / g.sum(), g / g.sum())
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    a, b = a.astype(np.float64), b.astype(np.float64)

    def f(v):
        return np.stack([correlate2d(v[..., c], w2, mode="valid") for c in range(v.shape[-1])], axis=-1)
    ma, mb = f(a), f(b)
    saa, sbb, sab = f(a * a) - ma * ma, f(b * b) - mb * mb, f(a * b) - ma * mb
    cs = (2 * sab + c2) / (saa + sbb + c2)
    return (2 * ma * mb + c1) / (ma * ma + mb * mb + c1) * cs, cs


# ---------------------------------------------------------------------------------------------------
# the named checks
# ---------------------------------------------------------------------------------------------------
def check_scipy(ev, families=FAMILIES, depths=DEPTH_L):
    worst = 0.0
    for name in families:
        for L in depths:
            a, b = family(name, L)
            got, want = ev.maps(a, b, L), independent_maps(a, b, L)
            for g, w in zip(got, want):
                assert g.shape == w.shape == (14, 19, 2)
                worst = max(worst, float(np.abs(g - w).max()))
                assert np.abs(g - w).max() <= 1e-10, (name, L, float(np.abs(g - w).max()))
    return worst


def check_constants(ev):
    for L in DEPTH_L:
        c1, c2 = ev.constants(L)
        assert c1 == (0.01 * L) ** 2 and c2 == (0.03 * L) ** 2 and c2 > c1


def check_window(ev):
    w = ev.window()
    assert w.dtype == np.float64 and w.shape == (11,)
    assert abs(float(w.sum()) - 1.0) <= 2e-16 and np.array_equal(w, w[::-1]) and int(np.argmax(w)) == 5
    assert np.array_equal(w.view(np.int64), utils.ssim_window().view(np.int64))


def check_pool(ev):
    rng = np.random.default_rng(3)
    for H, W in ((8, 6), (9, 7), (11, 12), (1, 5)):
        q = rng.integers(0, 65536, (H, W, 3))
        want = q[:H // 2 * 2, :W // 2 * 2].reshape(H // 2, 2, W // 2, 2, 3).sum(axis=(1, 3))
        got = ev.pool(q)
        assert got.shape == want.shape and np.array_equal(got, want)


def check_identity(ev, shape=(177, 191, 3)):
    a = np.random.default_rng(5).integers(0, 256, shape)
    maps = ev.scale_maps(a, a, 255, 5)
    assert len(maps) == 5
    for s, (ssim, cs) in enumerate(maps):
        assert ssim.shape == ((shape[0] >> s) - 10, (shape[1] >> s) - 10, shape[2])
        assert np.all(ssim == 1.0) and np.all(cs == 1.0), s
    sums = ev.sums(a, a, 255, 5)
    for s in range(5):
        assert sums[s] == [[ev.positions(shape[0], shape[1], s) * E.FX] * 2] * shape[2]


def _direct_figures(maps, weights=E.MS_WEIGHTS):
    ssim = float(maps[0][0].mean())
    per = []
    for c in range(maps[0][0].shape[-1]):
        means = [float(maps[s][1][..., c].mean()) for s in range(4)] + [float(maps[4][0][..., c].mean())]
        per.append(np.prod([max(m, 0.0) ** w for m, w in zip(means, weights)]))
    return ssim, float(np.mean(per))


def check_figures(ev):
    """the figures from the fixed-point sums against direct fp64 means of the evaluator's own maps; the channels differ, so a
    mean over the channels taken before the product is another number"""
    rng = np.random.default_rng(11)
    H, W = 176, 180
    a = rng.integers(0, 256, (H, W, 3))
    b = a.copy()
    b[..., 0] = np.clip(a[..., 0] + rng.integers(-2, 3, (H, W)), 0, 255)
    b[..., 1] = np.clip(a[..., 1] + rng.integers(-40, 41, (H, W)), 0, 255)
    b[..., 2] = rng.integers(0, 256, (H, W))
    ref = E.Evaluator()
    want_ssim, want_ms = _direct_figures(ref.scale_maps(a, b, 255, 5))
    sums = ref.sums(a, b, 255, 5)
    got_ssim, got_ms = ev.ssim_figure(sums, H, W), ev.msssim_figure(sums, H, W)
    assert abs(got_ssim - want_ssim) <= 1e-11 and abs(got_ms - want_ms) <= 1e-11, (got_ssim - want_ssim, got_ms - want_ms)
    return sums, got_ssim, got_ms


CHECKS = dict(scipy=check_scipy, constants=check_constants, window=check_window, pool=check_pool, identity=check_identity,
              figures=check_figures)


# ---------------------------------------------------------------------------------------------------
# the evaluator passes every check
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("L", DEPTH_L)
def test_maps_agree_with_the_2d_correlation(name, L):
    worst = check_scipy(E.Evaluator(), [name], [L])
    print(f"{name} L={L}: worst |separable - correlate2d| = {worst:.3g}")


def test_constants_and_window():
    check_constants(E.Evaluator())
    check_window(E.Evaluator())
    assert utils.ssim_constants(utils.SampleFormat.u8()) == E.constants(255)
    for depth in (9, 12, 16):
        assert utils.ssim_constants(utils.SampleFormat.u16(depth)) == E.constants(E.level_max(2, depth))
    for fmt in (utils.SampleFormat.f32(), utils.SampleFormat.s16()):
        with pytest.raises(ValueError):
            utils.ssim_constants(fmt)


def test_identical_operands_give_exactly_one_at_all_five_scales():
    check_identity(E.Evaluator())


def test_pooling_is_the_floor_block_sum():
    check_pool(E.Evaluator())
    # two halvings = the 4 x 4 block sum with the trailing rows / columns dropped at EACH halving (11 -> 5 -> 2)
    q = np.random.default_rng(4).integers(0, 4096, (11, 13, 1))
    assert np.array_equal(E.pool(E.pool(q)), q[:8, :12].reshape(2, 4, 3, 4, 1).sum(axis=(1, 3)))


def test_msssim_needs_176_per_side():
    z = np.zeros((175, 300, 1), dtype=np.int64)
    with pytest.raises(ValueError):
        E.scale_maps(z, z, 255, 5)
    with pytest.raises(ValueError):
        E.msssim_figure([[[0, 0]]] * 5, 175, 300)
    with pytest.raises(ValueError):
        utils.msssim_from_sums(np.zeros((1, 5, 1, 2), dtype=np.int64), 175, 300)
    with pytest.raises(ValueError):
        utils.msssim_from_sums(np.zeros((1, 4, 1, 2), dtype=np.int64), 176, 176)       # four scales are no MS-SSIM
    z = np.zeros((176, 176, 1), dtype=np.int64)
    assert len(E.scale_maps(z, z, 255, 5)) == 5
    one = np.asarray(E.sums(z, z, 255, 5), dtype=np.int64)[None]
    assert utils.msssim_from_sums(one, 176, 176).tolist() == [1.0] and E.msssim_figure(E.sums(z, z, 255, 5), 176, 176) == 1.0


def test_figures_from_the_sums():
    sums, ssim, ms = check_figures(E.Evaluator())
    arr = np.asarray(sums, dtype=np.int64)[None]
    # the package's figure functions are the evaluator's, as floats
    assert utils.ssim_from_sums(arr, 176, 180).tolist() == [ssim]
    assert utils.msssim_from_sums(arr, 176, 180).tolist() == [ms]
    assert utils.ssim_from_sums(np.concatenate([arr, arr])[:, :1], 176, 180).tolist() == [ssim, ssim]
    assert 0.0 < ms < 1.0 and 0.0 < ssim < 1.0
    # a negative mean cs (an image against its complement) is clamped to 0 before the power
    a, b = family("complement", 255, (176, 176, 1))
    neg = E.sums(a, b, 255, 5)
    assert neg[0][0][1] < 0 and E.msssim_figure(neg, 176, 176) == 0.0
    assert utils.msssim_from_sums(np.asarray(neg, dtype=np.int64)[None], 176, 176).tolist() == [0.0]


# ---------------------------------------------------------------------------------------------------
# mutants: the evaluator with one step broken, and the check that notices
# ---------------------------------------------------------------------------------------------------
class TapOffByOne(E.Evaluator):
    def filter_axis(self, v, w, axis):
        return super().filter_axis(v, np.roll(w, 1), axis)


class ConstantsExchanged(E.Evaluator):
    def constants(self, L):
        c1, c2 = super().constants(L)
        return c2, c1


class WindowNotNormalised(E.Evaluator):
    def window(self):
        k = np.arange(11, dtype=np.float64)
        return np.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2))


class CeilPooling(E.Evaluator):
    def pool(self, q):
        q = np.asarray(q).astype(np.int64)
        q = np.pad(q, ((0, q.shape[0] % 2), (0, q.shape[1] % 2), (0, 0)))
        return super().pool(q)


class CsWithoutTheFactor(E.Evaluator):
    def cs_numerator(self, sab, c2):
        return sab + c2


class ChannelMeanFirst(E.Evaluator):
    def msssim_figure(self, sums, H, W):
        C = len(sums[0])
        means = [sum(float(sums[s][c][1 if s < 4 else 0]) / float(E.FX) / float(self.positions(H, W, s)) for c in range(C)) / C
                 for s in range(5)]
        return self.channel_figure(means)


MUTANTS = [(TapOffByOne, "scipy"), (ConstantsExchanged, "constants"), (ConstantsExchanged, "scipy"), (WindowNotNormalised, "window"),
           (WindowNotNormalised, "scipy"), (CeilPooling, "pool"), (CsWithoutTheFactor, "identity"), (CsWithoutTheFactor, "scipy"),
           (ChannelMeanFirst, "figures")]


@pytest.mark.parametrize("mutant,check", MUTANTS, ids=[f"{m.__name__}-{c}" for m, c in MUTANTS])
def test_a_broken_evaluator_is_caught(mutant, check):
    kw = dict(families=["smooth"], depths=[255]) if check == "scipy" else {}
    with pytest.raises(AssertionError):
        CHECKS[check](mutant(), **kw)
    CHECKS[check](E.Evaluator(), **kw)                       # (the same check, with the same arguments, passes the evaluator)
