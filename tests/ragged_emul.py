"""numpy restatement of the per-signal entries of include/rcb.h (N4 413: rcb_signal_patch_ragged, rcb_recon_finish_ragged), composed
signal by signal from the evaluators of the entries they generalise, which stay as they are:

    targets  = the rows of sample16_emul.targets(view_k[None], pad=True), signal after signal
    finish   = sample16_emul.finish_whole(rows of signal k, size=sizes[k]) per signal: q / whole cropped to the signal's own extent
               (and transposed where it is delivered with axes 0 and 1 exchanged), sse / n_bad over its real samples

np.pad, slicing and np.transpose carry the geometry; nothing here knows offsets, strides or tables (premises:
tests/test_ragged_emul_cpu.py)."""
import numpy as np

import sample16_emul as Q

F32 = np.float32


def per_of(patch_nums):
    return int(np.prod(patch_nums))


def targets(views, patch_nums, patch_size, fmt):
    """views: a list of arrays [*size_k, C] (the signals along the MODEL's axes) -> fp32 [n * per, P, C]"""
    return np.concatenate([Q.targets(np.asarray(v)[None], patch_nums, patch_size, fmt, pad=True) for v in views], axis=0)


def finish(y, target, patch_nums, patch_size, fmt, sizes, swaps=None):
    """-> dict(q: list (None entries for f32), whole: list, sse [n] (None without target), n_bad [n]); entry k of a list is
    [*sizes[k], C], or with swaps[k] its transpose [sizes[k][1], sizes[k][0], C], contiguous"""
    y = np.asarray(y, dtype=F32)
    per, n = per_of(patch_nums), len(sizes)
    assert y.shape[0] == n * per
    swaps = [False] * n if swaps is None else list(swaps)
    out = dict(q=[], whole=[], sse=None if target is None else np.zeros(n), n_bad=np.zeros(n, dtype=np.int32))
    for k in range(n):
        rows = slice(k * per, (k + 1) * per)
        one = Q.finish_whole(y[rows], None if target is None else np.asarray(target, dtype=F32)[rows], patch_nums, patch_size, fmt,
                             size=tuple(sizes[k]))
        for key in ("q", "whole"):
            a = None if one[key] is None else one[key][0]
            if a is not None and swaps[k]:
                assert a.ndim == 3
                a = np.ascontiguousarray(a.transpose(1, 0, 2))
            out[key].append(a)
        if target is not None:
            out["sse"][k] = one["sse"][0]
        out["n_bad"][k] = one["n_bad"][0]
    return out
