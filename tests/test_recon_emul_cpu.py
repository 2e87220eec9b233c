"""The premises of the rcb_recon_finish tests (tests/test_hip_recon.py), checked on the CPU: the evaluator tests/recon_emul.py
stitches as the product cuts, its figures are utils.metric's up to the rounding of numpy's float32 mean, and the special inputs
used on the GPU (ties, the 8-bit lattice, dyadic values) are what the GPU tests take them for."""
import math

import numpy as np
import pytest
import torch

import recon_emul as E
from recombiner_amd import utils

F32 = np.float32
U24 = 2.0 ** -24                 # unit roundoff of fp32


# ---- the bounds the GPU tests share ------------------------------------------------------------------------------------------
def psnr_bound_db(n, psnr_max=60.0):
    """|utils.metric - metric_from_sse| for a PSNR over n elements, in dB, derived from utils.metric's own float32 evaluation
    (metric_from_sse is fp64 throughout: its error is ~1e-15 and is covered by the slack of the last term):
      * numpy's float32 pairwise mean of n positive terms: each term (d^2, one rounding) and each of the ceil(log2 n) levels of
        additions and the final division contribute one rounding: relative error <= (ceil(log2 n) + 2) * 2^-24 in the mse;
        PSNR = -10 log10(mse), so 10 log10(1 + e) = 4.3430 e dB.  Below 1e-5 dB for every n used here (n < 2^30).
      * np.sqrt and the division max_value / sqrt in float32: 2^-24 relative each in the amplitude: 8.6859 * 2^-24 dB each;
      * np.log10 in float32 (within 1 ulp of a result of magnitude <= psnr_max / 20) and the product 20 * . (half an ulp of the
        result <= psnr_max): 20 * ulp32(psnr_max / 20) + ulp32(psnr_max) / 2."""
    mean = 10.0 * math.log10(1.0 + (math.ceil(math.log2(n)) + 2) * U24)
    assert mean < 1e-5
    chain = 2 * 20.0 * math.log10(1.0 + U24)
    ulp = lambda v: 2.0 ** (math.floor(math.log2(v)) - 23)      # noqa: E731
    return mean + chain + 20.0 * ulp(psnr_max / 20.0) + 0.5 * ulp(psnr_max)


def rmsd_bound_abs(n, amp, rmsd):
    """absolute bound on |batch_RMSD - metric_from_sse(protein)| for |original|, |compressed| <= amp (the PSNR bound with the
    square root, plus the fp32 roundings of the * 25 -- which are relative to the VALUES, not to their difference, hence absolute):
      * utils.batch_RMSD rounds 25 * o and 25 * c to fp32 (2 roundings: error <= 2^-24 * 25 amp each) and their difference (one
        more rounding, <= 2^-24 * 50 amp): its scaled difference D = 25 (o - c) is off by <= 4 * 25 amp * 2^-24, while the device
        forms d = o - c in fp32 (one rounding, 2 amp * 2^-24, times 25): together e_D <= 6 * 25 amp * 2^-24 per element;
      * the root-mean-square is 1-Lipschitz in the elementwise perturbation's root-mean-square: |rms(D + e) - rms(D)| <= rms(e)
        <= e_D; times sqrt(3);
      * the float32 mean, x 3 and square root: relative (ceil(log2 n) + 2 + 1) * 2^-24 in the mean-square, half of it in the root,
        plus one rounding of the root."""
    e_d = 6 * 25.0 * amp * U24
    rel = 0.5 * (math.ceil(math.log2(n)) + 3) * U24 + U24
    return math.sqrt(3.0) * e_d + rel * rmsd


GEOMS = [((5,), (7,), 1), ((2, 3), (4, 5), 3), ((1, 2, 2), (3, 2, 4), 3), ((2, 2), (3, 3), 20)]


# ---- stitching -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn,ps,C", GEOMS)
def test_stitching_inverts_the_products_cut_back(pn, ps, C):
    """the evaluator's stitch is the inverse of the cut-back of utils.map_lpe_to_inr_inputs (1-D, 2-D, 3-D): the product's function,
    given an identity `upsample_net`, cuts stitched grids into patches; stitching its result gives the grids back, and its result is
    the evaluator's own cut"""
    nd, n_data, S = len(pn), 2, 1
    G = [a * b for a, b in zip(pn, ps)]
    rng = np.random.RandomState(0)
    whole = rng.rand(n_data, *G, C).astype(F32)
    held = {}

    def fake_net(z):            # channel-first in, channel-first out: hand the stitched grids through
        held["shape"] = tuple(z.shape)
        return torch.from_numpy(whole).movedim(-1, 1)

    N = n_data * int(np.prod(pn))
    lat = torch.zeros(S, N, int(np.prod(ps)) * C)
    pe = utils.map_lpe_to_inr_inputs(fake_net, lat, C, list(ps), [1] * nd, True, list(pn), nd)        # [N, S, P, C]
    assert held["shape"] == (n_data, C, *G)
    patches = pe[:, 0].contiguous().numpy()
    assert patches.shape == (N, int(np.prod(ps)), C)
    assert np.array_equal(E.stitch(patches, pn, ps), whole)
    assert np.array_equal(E.cut(whole, pn, ps), patches)
    # the layout of the header: row n = patch n % prod(pn) (row-major) of datapoint n / prod(pn); pixel p row-major in the patch
    n, p = N - 2, int(np.prod(ps)) - 3
    dpt, pidx = divmod(n, int(np.prod(pn)))
    b, i = np.unravel_index(pidx, pn), np.unravel_index(p, ps)
    assert np.array_equal(patches[n, p], whole[(dpt,) + tuple(bb * s + ii for bb, s, ii in zip(b, ps, i))])


def test_stitch_without_geometry_is_the_identity():
    a = np.arange(2 * 5 * 3, dtype=F32).reshape(2, 5, 3)
    assert E.stitch(a) is a or np.array_equal(E.stitch(a), a)


# ---- agreement with utils.metric -------------------------------------------------------------------------------------------------
def _case(dataset, seed=0):
    rng = np.random.RandomState(seed)
    shape = {"cifar": (3, 32 * 32, 3), "kodak": (6, 20, 3), "video": (4, 24, 3), "audio": (5, 7, 1), "protein": (3, 96, 3)}[dataset]
    y = rng.rand(*shape).astype(F32)
    pred = (y + 0.05 * rng.randn(*shape)).astype(F32)
    return y, pred


@pytest.mark.parametrize("dataset", ["cifar", "kodak", "video", "audio", "protein"])
def test_evaluator_figures_agree_with_utils_metric(dataset):
    """metric_from_sse on the evaluator's fp64 sums against utils.metric on the same arrays, within the bounds derived above"""
    y, pred = _case(dataset)
    mode = 0 if utils.METRIC_ROUNDS[dataset] else 1
    r = E.finish(pred, y, mode=mode)
    n = y[0].size
    got = utils.metric_from_sse(r["sse"], n, dataset)
    want = utils.metric(y, pred, dataset)
    if dataset == "protein":
        assert got.shape == want.shape == (y.shape[0],)
        err = np.abs(got - want.astype(np.float64))
        bound = np.array([rmsd_bound_abs(n, 1.3, g) for g in got])
        print("protein RMSD", got, "max |diff| / bound", (err / bound).max())
        assert (err <= bound).all()
        return
    n_mean = n if dataset == "cifar" else y.size
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    print(dataset, "PSNR", got, "max |diff| %.3g dB, bound %.3g dB" % (err.max(), psnr_bound_db(n_mean)))
    assert np.shape(got) == np.shape(want) and isinstance(got, float) == isinstance(want, float)
    assert err.max() <= psnr_bound_db(n_mean)
    assert np.all(np.asarray(got) < 60.0)                       # (the bound's psnr_max)


def test_metric_from_sse_rejects_an_unknown_dataset():
    with pytest.raises(ValueError):
        utils.metric_from_sse(np.ones(2), 4, "mnist")


# ---- the special inputs -----------------------------------------------------------------------------------------------------------
def test_tie_inputs_are_ties_with_both_parities():
    x, k = E.tie_inputs()
    assert x.dtype == F32 and np.all((x > 0) & (x < 1))
    prod = x * F32(255)
    assert prod.dtype == F32 and np.array_equal(prod.astype(np.float64), k + 0.5)
    print("ties: %d inputs, %d with even k, %d with odd k" % (len(x), int((k % 2 == 0).sum()), int((k % 2 == 1).sum())))
    assert len(x) >= 32 and (k % 2 == 0).any() and (k % 2 == 1).any()
    q, _ = E.round8(x)
    assert np.array_equal(q, np.where(k % 2 == 0, k, k + 1))     # half to even: what np.round gives, not floor(p + 0.5)
    assert np.array_equal(q, np.round(np.clip(x, 0, 1) * 255))


def test_lattice_survives_a_second_rounding():
    k = np.arange(256)
    v = (k.astype(F32) / F32(255)).astype(F32)
    assert np.array_equal(np.rint(v * F32(255)), k)
    q, v2 = E.round8(v)
    assert np.array_equal(q, k) and np.array_equal(v2, v)


def test_dyadic_terms_are_exact_in_any_order():
    """mode-1 terms of dyadic inputs are exact multiples of 2^-12 and every partial sum stays below 2^40 units (< 2^53): any
    summation order gives the same fp64"""
    y, t = E.dyadic((2, 5000, 3), 1), E.dyadic((2, 5000, 3), 2)
    tm = E.terms(y, t)
    units = tm * 4096.0
    assert np.array_equal(units, np.round(units)) and units.max() <= 2 ** 14
    assert units.sum(axis=None) < 2.0 ** 40 and (2 ** 21) * (2 ** 14) < 2 ** 40          # (the largest datapoint the GPU test sums)
    flat = tm.reshape(2, -1)
    rng = np.random.RandomState(0)
    for row in flat:
        ref = math.fsum(row)                   # exact; pairwise, reversed and sequential sums of a permutation give the same
        assert ref == row.sum() == row[::-1].sum() == row[rng.permutation(row.size)].cumsum()[-1]


def test_evaluator_edge_values():
    x = np.array([-0.0, 0.0, 1.0, np.inf, -np.inf, np.nan, 1.5, -3.0, 0.5], dtype=F32).reshape(1, -1, 1)
    r = E.finish(x, np.zeros_like(x), mode=0)
    assert r["u8"].reshape(-1).tolist() == [0, 0, 255, 255, 0, 0, 255, 0, 128]
    assert r["n_bad"].tolist() == [3] and np.isnan(r["sse"][0])
