"""numpy restatement of rcb_signal_patch_pad and rcb_recon_finish_crop (include/rcb.h, N4 411), composed from the evaluators of the
uncropped entries, which it leaves as they are:

    pad  = signal_emul.targets(np.pad(view, mode="edge") out to the grid, patch_nums, patch_size)
    crop = recon_emul.finish(...) with u8 / whole sliced to the extent, sse = math.fsum over the exact fp64 terms INSIDE the
           extent (NaN when one of those elements is not finite), n_bad = the non-finite x and t inside the extent

np.pad and slicing carry the geometry; no index arithmetic is shared with the kernels (premises: tests/test_extent_emul_cpu.py)."""
import math

import numpy as np

import recon_emul as E
import signal_emul as S

F32 = np.float32

# name -> (patch_nums, patch_size, C, sizes): the smallest shapes at which each index term and each path can go wrong
CASES = {
    "1d": ((3,), (4,), 1, [(12,), (9,), (8,), (1,)]),                       # (8,): the last patch wholly padded
    # (7, 11): cropped rows of 33 elements, not 4-aligned, a quad straddling the edge; (5, 4): a whole column of patches padded
    "2d": ((2, 3), (4, 4), 3, [(8, 12), (7, 11), (5, 4), (1, 1)]),
    "2d_aligned": ((2, 3), (4, 4), 4, [(6, 10)]),                           # cropped rows of 40 elements: stores by quad
    "2d_elem": ((2, 2), (3, 5), 3, [(4, 7)]),                               # runs of 15: the element path only
    "3d": ((1, 2, 2), (2, 4, 4), 3, [(2, 7, 5), (1, 8, 8)]),
    "unpatched": ((1, 1), (4, 4), 3, [(3, 4)]),
}
N_DATA = 3
ALL = [(name, size) for name, (_, _, _, sizes) in CASES.items() for size in sizes]


def grid_of(patch_nums, patch_size):
    return tuple(a * b for a, b in zip(patch_nums, patch_size))


def pad_edge(view, patch_nums, patch_size):
    """view [n, *size, C] -> [n, *G, C]: the edge samples replicated after the signal on every spatial axis"""
    view = np.asarray(view)
    G = grid_of(patch_nums, patch_size)
    size = view.shape[1:-1]
    assert len(size) == len(G) and all(1 <= s <= g for s, g in zip(size, G))
    return np.pad(view, [(0, 0)] + [(0, g - s) for s, g in zip(size, G)] + [(0, 0)], mode="edge")


def targets(view, patch_nums, patch_size):
    """what rcb_signal_patch_pad writes: fp32 [N, P, C]"""
    return S.targets(pad_edge(view, patch_nums, patch_size), patch_nums, patch_size)


def inside(n_data, patch_nums, patch_size, C, size):
    """bool [n_data, *G, C]: the positions of the grid that lie inside the extent"""
    G = grid_of(patch_nums, patch_size)
    m = np.zeros((n_data, *G, C), dtype=bool)
    m[(slice(None),) + tuple(slice(0, s) for s in size)] = True
    return m


def finish_crop(y, target, patch_nums, patch_size, size, mode=0):
    """-> dict(u8, whole, sse, n_bad, terms): u8 / whole [n_data, *size, C]; `terms` [n_data, prod(size) * C] are the exact fp64 terms
    of the elements inside the extent (for error bounds)"""
    y = np.asarray(y, dtype=F32)
    full = E.finish(y, target, patch_nums, patch_size, mode=mode)
    crop = (slice(None),) + tuple(slice(0, s) for s in size)
    n_data, C = full["whole"].shape[0], y.shape[-1]
    out = dict(u8=None if full["u8"] is None else np.ascontiguousarray(full["u8"][crop]),
               whole=np.ascontiguousarray(full["whole"][crop]), sse=None, terms=None)
    bad = (~np.isfinite(E.stitch(y, patch_nums, patch_size)[crop])).reshape(n_data, -1).sum(1)
    if target is not None:
        t = np.asarray(target, dtype=F32)
        bad = bad + (~np.isfinite(E.stitch(t, patch_nums, patch_size)[crop])).reshape(n_data, -1).sum(1)
        tm = E.stitch(full["terms"].reshape(y.shape), patch_nums, patch_size)[crop].reshape(n_data, -1)
        out["terms"] = tm
        out["sse"] = np.array([math.fsum(row) if b == 0 else np.nan for row, b in zip(tm, bad)], dtype=np.float64)
    out["n_bad"] = bad.astype(np.int32)
    return out
