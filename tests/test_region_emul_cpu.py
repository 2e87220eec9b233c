"""The premises of tests/region_emul.py, the evaluator tests/test_hip_regions.py holds rcb_recon_regions to (include/rcb.h, N4 417),
and the host side of the feature; no GPU:

  1. partition: the regions' exact terms together are the terms rcb_recon_finish_fmt sums over the same extent -- math.fsum of
     their concatenation equals extent_emul.finish_crop's / sample16_emul.finish_whole's sse EXACTLY (fsum is correctly rounded) --
     the counts add up to prod(size) * C and n_bad_r to n_bad;
  2. padding: a NaN planted in every padded position of y and target changes no region output;
  3. three deliberate mistakes in a copy of the evaluator each fail 1 or 2 on a named case;
  4. utils.region_grid / region_counts / region_of against the evaluator's shapes, utils.metric_regions_from_sse against utils.PSNR
     of each box within psnr_bound_db;
  5. rcb_recon_regions_workspace_bytes against its formula and its refusals (callable without a device)."""
import math

import numpy as np
import pytest

import extent_emul as X
import recon_emul as E
import region_emul as R
import sample16_emul as K
from test_recon_emul_cpu import psnr_bound_db

from recombiner_amd import _lib, ops, utils

F32 = np.float32
FORMATS = [K.U8, K.F32FMT, K.u16(9), K.S16]


def _inputs(name, kind="random", seed=1):
    pn, ps, Cc, _, _ = R.CASES[name]
    return (pn, ps, Cc) + R.inputs(pn, ps, Cc, seed, kind=kind)


def _with_bad(y, t):
    yb, tb = y.copy(), t.copy()
    yb.reshape(-1)[::17] = np.nan
    tb.reshape(-1)[5::23] = np.inf
    return yb, tb


def _whole_sum(y, t, pn, ps, fmt, size):
    """the datapoint figures of the entries that exist: finish_crop for the 8-bit / raw modes with a size, finish_whole otherwise"""
    if size is not None and fmt[0] < 2:
        return X.finish_crop(y, t, pn, ps, size, mode=fmt[0])
    return K.finish_whole(y, t, pn, ps, fmt, size=size)


def check_partition(evaluate, name, size, region, fmt):
    pn, ps, Cc, y, t = _inputs(name)
    extent = size if size is not None else X.grid_of(pn, ps)
    got = evaluate(y, t, pn, ps, region, fmt, size)
    want = _whole_sum(y, t, pn, ps, fmt, size)
    nr = R.region_grid(extent, region)
    assert int(got["counts"].sum()) == int(np.prod(extent)) * Cc
    assert got["sse_r"].shape == got["n_bad_r"].shape == (R.N_DATA, *nr)
    for d in range(R.N_DATA):
        every = np.concatenate([got["terms"][(d,) + idx] for idx in np.ndindex(*nr)])
        assert every.size == int(np.prod(extent)) * Cc
        assert math.fsum(every) == want["sse"][d]
        assert math.fsum(got["sse_r"][d].reshape(-1)) == pytest.approx(want["sse"][d], rel=1e-12)
    yb, tb = _with_bad(y, t)
    got, want = evaluate(yb, tb, pn, ps, region, fmt, size), _whole_sum(yb, tb, pn, ps, fmt, size)
    assert np.array_equal(got["n_bad_r"].reshape(R.N_DATA, -1).sum(1), want["n_bad"])
    assert np.array_equal(np.isnan(got["sse_r"]), got["n_bad_r"] > 0)


def check_padding(evaluate, name, size, region, fmt):
    pn, ps, Cc, y, t = _inputs(name, seed=3)
    clean = evaluate(y, t, pn, ps, region, fmt, size)
    pad = E.cut(~X.inside(R.N_DATA, pn, ps, Cc, size if size is not None else X.grid_of(pn, ps)), pn, ps)
    yn, tn = np.where(pad, F32(np.nan), y), np.where(pad, F32(np.nan), t)
    assert size is None or pad.any()
    got = evaluate(yn, tn, pn, ps, region, fmt, size)
    assert np.array_equal(got["sse_r"], clean["sse_r"], equal_nan=True) and np.array_equal(got["n_bad_r"], clean["n_bad_r"])
    assert not np.isnan(got["sse_r"]).any()


def _evaluator(y, t, pn, ps, region, fmt, size):
    return R.finish_regions(y, t, pn, ps, region, fmt=fmt, size=size)


@pytest.mark.parametrize("fmt", FORMATS, ids=str)
@pytest.mark.parametrize("name,size,region", R.ALL, ids=str)
def test_the_regions_partition_the_extent(name, size, region, fmt):
    check_partition(_evaluator, name, size, region, fmt)


@pytest.mark.parametrize("name,size,region", R.ALL, ids=str)
def test_padding_changes_no_region(name, size, region):
    check_padding(_evaluator, name, size, region, K.U8)


def test_the_many_chunks_case_is_one_region_of_257_chunks():
    pn, ps, Cc, size, region = R.MANY
    assert R.region_grid(X.grid_of(pn, ps), region) == (1, 1)
    assert -(-int(np.prod(ps)) * Cc // 8192) == 257


# ---- 3. mutants ------------------------------------------------------------------------------------------------------------------
def _mutant(which):
    """a copy of region_emul.finish_regions with one mistake:
      "grid"      the regions tile the grid instead of the extent
      "unclipped" a box on the far edge is not clipped to the extent
      "channels"  the stitched signal is read with the channels outermost"""
    def evaluate(y, t, pn, ps, region, fmt, size):
        y, t = np.asarray(y, dtype=F32), np.asarray(t, dtype=F32)
        _, v = K.finish(y, fmt)
        G = X.grid_of(pn, ps)
        extent = tuple(size) if size is not None else G
        crop = (slice(None),) + tuple(slice(0, s) for s in extent)

        def whole(a):
            w = E.stitch(a, pn, ps)
            if which == "channels":
                w = np.moveaxis(w.reshape(w.shape[0], w.shape[-1], *G), 1, -1)
            return w if which in ("grid", "unclipped") else w[crop]

        wy, wt, wm = whole(y), whole(t), whole(E.terms(v, t))
        tiled = G if which == "grid" else extent
        nr = R.region_grid(tiled, region)
        n_data = wy.shape[0]
        out = dict(sse_r=np.zeros((n_data, *nr)), n_bad_r=np.zeros((n_data, *nr), dtype=np.int32),
                   counts=np.zeros(nr, dtype=np.int64), terms={})
        for idx in np.ndindex(*nr):
            if which == "unclipped":
                sl = tuple(slice(r * q, (r + 1) * q) for r, q in zip(idx, region))
            else:
                sl = tuple(slice(r * q, min((r + 1) * q, s)) for r, q, s in zip(idx, region, tiled))
            out["counts"][idx] = wy[(0,) + sl].size
            for d in range(n_data):
                bad = int((~np.isfinite(wy[(d,) + sl])).sum()) + int((~np.isfinite(wt[(d,) + sl])).sum())
                tm = wm[(d,) + sl].reshape(-1)
                out["terms"][(d,) + idx] = tm
                out["sse_r"][(d,) + idx] = math.fsum(tm) if bad == 0 else np.nan
                out["n_bad_r"][(d,) + idx] = bad
        return out
    return evaluate


MUTANT_CASE = ("2d", (7, 13), (3, 4))          # an extent inside the grid, boxes that divide neither, three channels


@pytest.mark.parametrize("which", ["grid", "unclipped", "channels"])
def test_each_mutant_of_the_evaluator_is_caught(which):
    failed = []
    for check in (check_partition, check_padding):
        check(_evaluator, *MUTANT_CASE, K.U8)                          # (the evaluator itself passes)
        try:
            check(_mutant(which), *MUTANT_CASE, K.U8)
        except (AssertionError, KeyError, ValueError):
            failed.append(check.__name__)
    print(which, "fails", failed)
    assert failed


# ---- 4. the host helpers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size,region", R.ALL, ids=str)
def test_region_grid_and_counts_are_the_evaluators(name, size, region):
    pn, ps, Cc, y, _ = _inputs(name)
    extent = size if size is not None else X.grid_of(pn, ps)
    want = R.finish_regions(y, None, pn, ps, region, size=size)
    assert utils.region_grid(extent, region) == want["n_bad_r"].shape[1:]
    counts = utils.region_counts(extent, region, Cc)
    assert counts.dtype == np.int64 and np.array_equal(counts, want["counts"])


def test_region_of():
    lay3, lay2 = ops.PeLayout((1, 2, 2), (3, 2, 4)), ops.PeLayout((2, 3), (4, 5))
    assert utils.region_of(lay3, "patch") == (3, 2, 4) and utils.region_of(lay3, "frame") == (1, 4, 8)
    assert utils.region_of(lay3, "row") == (1, 4, 8) and utils.region_of(lay2, "row") == (1, 15)
    assert utils.region_of(lay2, (3, 4)) == (3, 4) and utils.region_of(lay2, [8, 100]) == (8, 100)
    config = dict(data_dim=2, pixel_sizes=[4, 5], patch_nums=[2, 3], patch=True)
    assert utils.region_of(config, "patch") == (4, 5) and utils.region_of(config, "row") == (1, 15)
    config["patch"] = False
    assert utils.region_of(config, "row") == (1, 5)
    for bad in (lambda: utils.region_of(lay2, "frame"), lambda: utils.region_of(lay2, "tile"), lambda: utils.region_of(lay2, (3,)),
                lambda: utils.region_of(lay2, (0, 4)), lambda: utils.region_grid((8, 15), (3,)), lambda: utils.region_grid((8,), (0,))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("dataset", ["kodak", "audio"])
@pytest.mark.parametrize("name,size,region", [("2d", None, (4, 5)), ("2d", (7, 13), (3, 4)), ("2d", (5, 11), (8, 15)),
                                              ("3d", None, (1, 4, 8)), ("3d", (2, 3, 7), (2, 3, 3)), ("1d", (33,), (10,))], ids=str)
def test_metric_regions_from_sse_is_utils_psnr_of_each_box(dataset, name, size, region):
    pn, ps, Cc, _, _ = R.CASES[name]
    rng = np.random.RandomState(4)
    shape = (R.N_DATA * int(np.prod(pn)), int(np.prod(ps)), Cc)
    t = rng.rand(*shape).astype(F32)
    y = (t + 0.05 * rng.randn(*shape)).astype(F32)
    rounds = utils.METRIC_ROUNDS[dataset]
    ev = R.finish_regions(y, t, pn, ps, region, fmt=K.U8 if rounds else K.F32FMT, size=size)
    got = utils.metric_regions_from_sse(ev["sse_r"], ev["counts"], dataset)
    assert got.dtype == np.float64 and got.shape == ev["sse_r"].shape
    wy, wt = R.whole_cropped(y, pn, ps, size), R.whole_cropped(t, pn, ps, size)
    for idx, sl in R.boxes(wy.shape[1:-1], region):
        for d in range(R.N_DATA):
            want = utils.PSNR(wt[(d,) + sl], wy[(d,) + sl], round=rounds)
            assert want < 60.0 and abs(got[(d,) + idx] - want) <= psnr_bound_db(int(ev["counts"][idx]))


def test_metric_regions_from_sse_special_values():
    sse = np.array([[0.0, np.nan, 3.0], [12.0, 1.0, 6.0]])
    counts = np.array([4, 2, 6])
    psnr = utils.metric_regions_from_sse(sse, counts, "video")
    assert psnr[0, 0] == np.inf and np.isnan(psnr[0, 1]) and psnr[0, 2] == -10.0 * np.log10(0.5)
    assert np.array_equal(utils.metric_regions_from_sse(sse, counts, "cifar"), psnr, equal_nan=True)     # per region, every preset
    rmsd = utils.metric_regions_from_sse(sse, counts, "protein")
    assert rmsd[1, 0] == 25.0 * np.sqrt(3.0 * 3.0) and rmsd[0, 0] == 0.0 and np.isnan(rmsd[0, 1])
    with pytest.raises(ValueError):
        utils.metric_regions_from_sse(sse, counts[:2], "video")
    with pytest.raises(ValueError):
        utils.metric_regions_from_sse(sse, counts, "imagenet")


# ---- 5. the workspace ---------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_formula_and_refusals():
    ws = _lib.load().rcb_recon_regions_workspace_bytes
    for n_data, n_regions, elems in [(1, 1, 1), (3, 6, 60), (3, 2, 8192), (3, 2, 8193), (1, 1, 2_100_000), (24, 1536, 768)]:
        assert ws(n_data, n_regions, elems) == n_data * n_regions * -(-elems // 8192) * 12
    for refused in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1, 1, 1 << 31), (1, 1 << 31, 1), (1 << 31, 1, 1),
                    (1 << 16, 1 << 15, 1), (1 << 11, 1 << 10, 8192 * 1024), (2, 1 << 30, 1), (1, 1 << 20, 8192 * 2048)]:
        assert ws(*refused) == -1, refused
    assert ws((1 << 31) - 1, 1, 1) == ((1 << 31) - 1) * 12 and ws(1, 1, (1 << 31) - 1) == (1 << 18) * 12
