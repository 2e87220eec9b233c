"""numpy restatement of the sample formats of include/rcb.h (N4 412: rcb_signal_patch_fmt, rcb_recon_finish_fmt), written from the header
text alone, every step one np.float32 operation:

    u16 at depth b, M = 2^b - 1:   in   y = float32(q) / float32(M)
                                   out  c = 0 if x is NaN else min(max(x, 0), 1);  q = rint(c * float32(M));  v = float32(int(q)) / M
    s16:                           in   y = (float32(q) + 32768) / 65536
                                   out  u = min(rint(c * 65536), 65535);  q = int(u) - 32768 (int16);  v = u / 65536
    u8 / f32:                      the evaluators of the older entries (signal_emul.unit8, recon_emul.round8), unchanged

composed around signal_emul / recon_emul / extent_emul the way extent_emul is: those carry the geometry (slices, np.pad, reshape /
transpose), this file only the per-sample arithmetic.  A format is the pair (kind, depth) of the header: U8 = (0, 0), F32 = (1, 0),
u16(b) = (2, b), S16 = (3, 0).  Premises: tests/test_sample16_emul_cpu.py."""
import math

import numpy as np

import extent_emul as X
import recon_emul as E
import signal_emul as S

F32 = np.float32
U8, F32FMT, S16 = (0, 0), (1, 0), (3, 0)


def u16(depth):
    assert 9 <= depth <= 16
    return (2, depth)


def m_of(fmt):
    return (1 << fmt[1]) - 1


def np_dtype(fmt):
    return (np.uint8, np.float32, np.uint16, np.int16)[fmt[0]]


def to_target(q, fmt):
    """stored samples -> fp32 targets, elementwise"""
    q = np.asarray(q)
    kind = fmt[0]
    if kind == 0:
        assert q.dtype == np.uint8
        return S.unit8(q)
    if kind == 1:
        assert q.dtype == F32
        return q
    if kind == 2:
        assert q.dtype == np.uint16
        y = q.astype(F32) / F32(m_of(fmt))                               # one fp32 division; no clamp above M
    else:
        assert q.dtype == np.int16
        y = (q.astype(F32) + F32(32768)) / F32(65536)                    # exact sum, exact division
    assert y.dtype == F32
    return y


def clip01(x):
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), F32(0), np.minimum(np.maximum(x, F32(0)), F32(1))).astype(F32)


def finish(x, fmt):
    """reconstruction values -> (q in the format's integer dtype (None for f32), v fp32), elementwise"""
    kind = fmt[0]
    if kind == 0:
        q, v = E.round8(x)
        return q.astype(np.uint8), v
    if kind == 1:
        return None, np.asarray(x, dtype=F32)
    c = clip01(x)
    if kind == 2:
        M = F32(m_of(fmt))
        p = c * M                                                        # one fp32 multiply
        assert p.dtype == F32
        qi = np.rint(p).astype(np.int64)                                 # half to even
        v = qi.astype(F32) / M                                           # from the INTEGER: q = 0 gives +0.0
        assert v.dtype == F32
        return qi.astype(np.uint16), v
    p = c * F32(65536)
    assert p.dtype == F32
    u = np.minimum(np.rint(p), F32(65535))
    v = u / F32(65536)
    assert v.dtype == F32
    return (u.astype(np.int64) - 32768).astype(np.int16), v


def targets(view, patch_nums, patch_size, fmt, pad=False):
    """what rcb_signal_patch_fmt writes: fp32 [N, P, C]; pad: `view` holds only its own extent and is edge-padded to the grid"""
    view = np.asarray(view)
    if pad:
        view = X.pad_edge(view, patch_nums, patch_size)
    return to_target(S.patch(view, patch_nums, patch_size), fmt)


def finish_whole(y, target, patch_nums, patch_size, fmt, size=None):
    """what rcb_recon_finish_fmt writes -> dict(q, whole, sse, n_bad, terms), the layout and the rules of recon_emul.finish
    (size None) or extent_emul.finish_crop (size): q / whole stitched and cropped, sse = math.fsum of the exact fp64 terms of the
    real elements (NaN when one of their x or t is not finite), n_bad = the non-finite x and t among them"""
    y = np.asarray(y, dtype=F32)
    q, v = finish(y, fmt)
    G = X.grid_of(patch_nums, patch_size) if patch_nums else None
    crop = (slice(None),) + (tuple(slice(0, s) for s in size) if size is not None else ())
    whole = E.stitch(v, patch_nums, patch_size)
    n_data = whole.shape[0]
    out = dict(q=None if q is None else np.ascontiguousarray(E.stitch(q, patch_nums, patch_size)[crop]),
               whole=np.ascontiguousarray(whole[crop]), sse=None, terms=None)
    assert size is None or (G is not None and len(size) == len(G))
    bad = (~np.isfinite(E.stitch(y, patch_nums, patch_size)[crop])).reshape(n_data, -1).sum(1)
    if target is not None:
        t = np.asarray(target, dtype=F32)
        bad = bad + (~np.isfinite(E.stitch(t, patch_nums, patch_size)[crop])).reshape(n_data, -1).sum(1)
        tm = E.stitch(E.terms(v, t), patch_nums, patch_size)[crop].reshape(n_data, -1)
        out["terms"] = tm
        out["sse"] = np.array([math.fsum(row) if b == 0 else np.nan for row, b in zip(tm, bad)], dtype=np.float64)
    out["n_bad"] = bad.astype(np.int32)
    return out


def tie_inputs(fmt):
    """fp32 x in (0, 1) whose rounded-to-nearest decision is an exact tie -> (x [n], k [n]): the integer part k of the half.
    u16: the fp32 product x * M is exactly k + 1/2 (the exact quotient (k + 1/2) / M is no fp32 number, but the ROUNDED product of
    a neighbour lands on the half; k + 1/2 must itself be an fp32 number: below 2^23, always true here).  s16: x = (k + 1/2) /
    65536 exactly, a dyadic fp32 number, its product exact.  A spread of k over the whole range, both parities."""
    if fmt[0] == 3:
        ks = np.unique(np.concatenate([np.arange(0, 64), np.arange(32760, 32776), np.arange(65470, 65535),
                                       np.arange(0, 65535, 257)]))
        x = ((ks.astype(np.float64) + 0.5) / 65536.0).astype(F32)
        assert np.array_equal(x.astype(np.float64) * 65536.0, ks + 0.5)
        return x, ks.astype(np.int64)
    M = m_of(fmt)
    ks = np.unique(np.concatenate([np.arange(0, min(M, 96)), np.arange(M - 96, M), np.arange(0, M, max(M // 251, 1))]))
    xs, kk = [], []
    for k in ks:
        x0 = F32((k + 0.5) / M)
        cand, lo, hi = [x0], x0, x0
        for _ in range(4):
            lo, hi = np.nextafter(lo, F32(0)), np.nextafter(hi, F32(1))
            cand += [lo, hi]
        for x in cand:
            if F32(x) * F32(M) == F32(k + 0.5) and 0 < x < 1:
                xs.append(x)
                kk.append(k)
    return np.array(xs, dtype=F32), np.array(kk, dtype=np.int64)


def special_values(fmt):
    """the ties, one ulp to either side of each, and the ends of the range (no NaN: the callers place those)"""
    x, _ = tie_inputs(fmt)
    one = F32(1)
    return np.concatenate([x, np.nextafter(x, F32(0)), np.nextafter(x, one),
                           np.array([-0.0, 0.0, 1.0, np.inf, -np.inf, np.nextafter(one, F32(0)), np.nextafter(one, F32(2)),
                                     np.nextafter(F32(0), F32(-1)), 1e-40, -1e-40, 0.5], dtype=F32)])
