"""numpy restatement of rcb_recon_regions (include/rcb.h, N4 417), written from its definition -- not from the kernel:

    the values v and the terms float64((t - v) in fp32)^2 are those of rcb_recon_finish_fmt (sample16_emul.finish, recon_emul.terms);
    y, target and the terms are stitched to whole signals (recon_emul.stitch) and cropped to the extent `size` (the grid without one);
    regions tile the EXTENT: nr[i] = ceil(size[i] / region[i]) boxes per axis, box r_i = [r_i * region[i], min((r_i + 1) * region[i],
    size[i])), the region index row-major; the elements of a box are its positions row-major with the channels innermost;
    sse_r[d][r]   = math.fsum of the box's exact fp64 terms (correctly rounded: half an ulp and no order of its own), NaN when one of
                    the box's y or target elements is not finite
    n_bad_r[d][r] = the non-finite y plus the non-finite target elements of the box (np.isfinite)

The boxes are cut by numpy slicing of the cropped whole signal; no index arithmetic is shared with the kernel.  A format is the
pair (kind, depth) of sample16_emul; the library's (mode, depth) is the same pair.  Premises: tests/test_region_emul_cpu.py."""
import math

import numpy as np

import recon_emul as E
import sample16_emul as K

F32 = np.float32

# name -> (patch_nums, patch_size, C, sizes (None: the grid), regions): the smallest shapes that reach each path of the kernel
CASES = {
    "1d": ((5,), (7,), 1, [None, (33,)], [(1,), (4,), (7,), (10,), (35,), (100,)]),
    # (3, 4) straddles patches on both axes; (4, 5) is the patch
    "2d": ((2, 3), (4, 5), 3, [None, (7, 13), (5, 11)], [(1, 1), (4, 5), (3, 4), (1, 15), (8, 1), (8, 15)]),
    "2d_vec": ((2, 2), (3, 4), 4, [None, (5, 7)], [(2, 2), (3, 4), (6, 8)]),               # runs of 16: the 16-byte path
    "3d": ((1, 2, 2), (3, 2, 4), 3, [None, (2, 3, 7)], [(1, 4, 8), (3, 2, 4), (2, 3, 3)]),  # "frame", "patch", a straddling box
    # (72, 48): one region of 10 368 elements, 2 chunks; (64, 48): regions of 2 chunks and of 1 chunk in one launch
    "two_chunks": ((3, 2), (24, 24), 3, [None], [(72, 48), (64, 48)]),
}
# 257 chunks: the `t, t + 256` leg of the reduce; one region covering an unpatched signal
MANY = ((1, 1), (1000, 700), 3, None, (1000, 700))
N_DATA = 3
ALL = [(name, size, region) for name, (_, _, _, sizes, regions) in CASES.items() for size in sizes for region in regions]


def mode_fmt(mode, depth=0):
    """the library's (mode, depth) -> the evaluators' format pair"""
    return (int(mode), int(depth))


def grid_of(patch_nums, patch_size):
    return tuple(a * b for a, b in zip(patch_nums, patch_size))


def region_grid(extent, region):
    return tuple(-(-int(s) // int(r)) for s, r in zip(extent, region))


def boxes(extent, region):
    """the boxes of the extent, in region order -> (index per axis, slices per axis)"""
    for idx in np.ndindex(*region_grid(extent, region)):
        yield idx, tuple(slice(r * q, min((r + 1) * q, s)) for r, q, s in zip(idx, region, extent))


def whole_cropped(a, patch_nums, patch_size, size):
    """[N, P, C] -> whole signals [n_data, *size, C]"""
    w = E.stitch(np.asarray(a), patch_nums, patch_size)
    return w if size is None else w[(slice(None),) + tuple(slice(0, s) for s in size)]


def finish_regions(y, target, patch_nums, patch_size, region, fmt=K.U8, size=None):
    """-> dict(sse_r [n_data, *nr] fp64 (None without target), n_bad_r [n_data, *nr] int32, counts [*nr] int64,
               terms: {(d, *idx): the box's exact fp64 terms in element order} (None without target; for the bounds))"""
    y = np.asarray(y, dtype=F32)
    _, v = K.finish(y, fmt)
    wy = whole_cropped(y, patch_nums, patch_size, size)
    n_data, extent = wy.shape[0], wy.shape[1:-1]
    nr = region_grid(extent, region)
    out = dict(sse_r=None, n_bad_r=np.zeros((n_data, *nr), dtype=np.int32), counts=np.zeros(nr, dtype=np.int64), terms=None)
    wt = wm = None
    if target is not None:
        t = np.asarray(target, dtype=F32)
        wt = whole_cropped(t, patch_nums, patch_size, size)
        wm = whole_cropped(E.terms(v, t), patch_nums, patch_size, size)
        out["sse_r"] = np.zeros((n_data, *nr), dtype=np.float64)
        out["terms"] = {}
    for idx, sl in boxes(extent, region):
        out["counts"][idx] = wy[(0,) + sl].size
        for d in range(n_data):
            bad = int((~np.isfinite(wy[(d,) + sl])).sum())
            if target is not None:
                bad += int((~np.isfinite(wt[(d,) + sl])).sum())
                tm = wm[(d,) + sl].reshape(-1)                              # positions row-major, channels innermost
                out["terms"][(d,) + idx] = tm
                out["sse_r"][(d,) + idx] = math.fsum(tm) if bad == 0 else np.nan
            out["n_bad_r"][(d,) + idx] = bad
    return out


def inputs(patch_nums, patch_size, C, seed, n_data=N_DATA, kind="dyadic"):
    """(y, target) [N, P, C]: dyadic (exact sums, mode 1), or uniform random slightly beyond [0, 1]"""
    shape = (n_data * int(np.prod(patch_nums)), int(np.prod(patch_size)), C)
    if kind == "dyadic":
        return E.dyadic(shape, seed), E.dyadic(shape, seed + 1)
    rng = np.random.RandomState(seed)
    return rng.uniform(-0.1, 1.1, size=shape).astype(F32), rng.uniform(0, 1, size=shape).astype(F32)
