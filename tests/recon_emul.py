"""numpy restatement of rcb_recon_finish (include/rcb.h, N4), written from its definition -- not from the kernel:

    mode 0:  q = rint(clip(x, 0, 1) * 255) in fp32 (round half to even),  v = q / 255 (fp32 division);  a NaN x gives q = 0
    mode 1:  v = x
    u8 / whole : q / v of every datapoint stitched to its whole signal
    sse[d]     : sum over the datapoint's elements of float64(d)^2, d = t - v subtracted in fp32; NaN if any x or t of the
                 datapoint is not finite
    n_bad[d]   : the non-finite x plus the non-finite t of the datapoint

The patch -> whole map is reshape / transpose, the way utils.map_lpe_to_inr_inputs cuts a stitched grid into patches (and
its inverse); no index arithmetic is shared with the kernel.  The sum is math.fsum: the correctly rounded sum of the exact
fp64 terms, so it carries half an ulp and no order of its own."""
import math

import numpy as np

F32 = np.float32


def stitch(a, patch_nums=None, patch_size=None):
    """a [N, P, C] -> whole signals [n_data, *(patch_nums[i] * patch_size[i]), C]; without a geometry the rows are whole"""
    a = np.asarray(a)
    if not patch_nums:
        return a
    pn, ps = list(patch_nums), list(patch_size)
    nd = len(pn)
    N, P, C = a.shape
    assert P == int(np.prod(ps)) and N % int(np.prod(pn)) == 0
    a = a.reshape(-1, *pn, *ps, C)                                   # [n_data, patch index per axis, pixel per axis, C]
    inter = [1 + i + j * nd for i in range(nd) for j in range(2)]    # (patch axis i, pixel axis i) side by side
    a = a.transpose([0] + inter + [1 + 2 * nd])
    return a.reshape(-1, *[pn[i] * ps[i] for i in range(nd)], C)


def cut(whole, patch_nums, patch_size):
    """the inverse: whole signals -> patches [N, P, C], with the reshape / permute of utils.map_lpe_to_inr_inputs"""
    pn, ps = list(patch_nums), list(patch_size)
    nd = len(pn)
    C = whole.shape[-1]
    split = [v for i in range(nd) for v in (pn[i], ps[i])]
    o = whole.reshape(-1, *split, C)
    back = [1 + 2 * i for i in range(nd)] + [2 + 2 * i for i in range(nd)]
    return o.transpose([0] + back + [1 + 2 * nd]).reshape(-1, int(np.prod(ps)), C)


def round8(x):
    """-> (q, v) of mode 0, both fp32 arrays"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(x), F32(0), np.clip(x, F32(0), F32(1))).astype(F32)
        p = c * F32(255)                                             # one fp32 multiply
        assert p.dtype == F32
        q = np.rint(p)                                               # half to even
        v = q / F32(255)                                             # one fp32 division
    assert v.dtype == F32
    return q, v


def terms(v, t):
    """float64((t - v) in fp32)^2, elementwise"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(t, dtype=F32) - np.asarray(v, dtype=F32)
        assert d.dtype == F32
        d = d.astype(np.float64)
        return d * d


def finish(y, target=None, patch_nums=None, patch_size=None, mode=0):
    """-> dict(u8, whole, sse, n_bad, terms): u8 None in mode 1; sse / terms None without target.  `terms` [n_data, E] are the
    exact fp64 terms of every datapoint (of the finite elements; for error bounds)."""
    y = np.asarray(y, dtype=F32)
    N, P, C = y.shape
    per = int(np.prod(patch_nums)) if patch_nums else 1
    n_data = N // per
    if mode == 0:
        q, v = round8(y)
        u8 = stitch(q.astype(np.uint8), patch_nums, patch_size)
    else:
        v, u8 = y, None
    out = dict(u8=u8, whole=stitch(v, patch_nums, patch_size), sse=None, terms=None)
    bad = (~np.isfinite(y)).reshape(n_data, -1).sum(1)
    if target is not None:
        t = np.asarray(target, dtype=F32)
        bad = bad + (~np.isfinite(t)).reshape(n_data, -1).sum(1)
        tm = terms(v, t).reshape(n_data, -1)
        out["terms"] = tm
        out["sse"] = np.array([math.fsum(row) if b == 0 else np.nan for row, b in zip(tm, bad)], dtype=np.float64)
    out["n_bad"] = bad.astype(np.int32)
    return out


def tie_inputs():
    """fp32 x in (0, 1) whose fp32 product with 255 is exactly k + 0.5: -> (x [n], k [n]).  The exact quotient (k + 0.5) / 255
    is never an fp32 number, but the ROUNDED product of a neighbour can land on the half: those are the inputs on which
    half-to-even and half-away-from-zero differ."""
    xs, ks = [], []
    for k in range(255):
        x0 = F32((k + 0.5) / 255.0)
        cand = [x0]
        lo = hi = x0
        for _ in range(4):
            lo, hi = np.nextafter(lo, F32(0)), np.nextafter(hi, F32(1))
            cand += [lo, hi]
        for x in cand:
            if F32(x) * F32(255) == F32(k + 0.5) and 0 < x < 1:
                xs.append(x)
                ks.append(k)
    return np.array(xs, dtype=F32), np.array(ks, dtype=np.int64)


def dyadic(shape, seed):
    """fp32 multiples of 2^-6 in [-1, 1]: differences are exact multiples of 2^-6 in [-2, 2], their squares exact multiples
    of 2^-12 up to 2^14 units"""
    rng = np.random.RandomState(seed)
    return (rng.randint(-64, 65, size=shape).astype(np.float64) / 64.0).astype(F32)
