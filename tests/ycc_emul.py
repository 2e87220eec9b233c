"""numpy restatement of rcb_ycc_to_rgb, rcb_rgb_to_ycc and rcb_ycc_sse (include/rcb.h, N4 418), written from the header's definition
-- not from the kernel: plain fp64 array arithmetic in the stated order (numpy rounds every product and every sum on its own, so
nothing is contracted), np.rint (half to even), Python-int sums.  tests/test_ycc_emul_cpu.py holds its premises; tests/
test_hip_ycc.py holds the kernels to it bit for bit."""
import numpy as np


def peak(kind, depth):
    """L of a sample format: 255 for kind 0 (uint8), 2^depth - 1 for kind 2 (u16 at depth 9 .. 16)"""
    return 255 if kind == 0 else (1 << depth) - 1


def chroma_size(H, W, ss):
    """(Hc, Wc) of the chroma planes of an H x W frame at subsampling ss (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0)"""
    return ((H + 1) // 2 if ss == 2 else H), ((W + 1) // 2 if ss else W)


def quantise(v, L):
    """Q(v) = (int)rint(fmin(fmax(v, 0), L)), half to even"""
    return np.rint(np.minimum(np.maximum(v, 0.0), float(L))).astype(np.int64)


def forward_unrounded(rgb, m):
    """p_k = (m[k][0] r + m[k][1] g) + m[k][2] b for k = 0, 1, 2: rgb integers [..., H, W, 3] -> three fp64 arrays [..., H, W]"""
    m = np.asarray(m, dtype=np.float64).reshape(3, 3)
    r, g, b = (np.asarray(rgb[..., k]).astype(np.float64) for k in range(3))
    return [(m[k, 0] * r + m[k, 1] * g) + m[k, 2] * b for k in range(3)]


def chroma_mean(p, ss):
    """the unrounded chroma plane of p [..., H, W] at subsampling ss: the mean over the block, the far row and column clipped"""
    H, W = p.shape[-2:]
    Hc, Wc = chroma_size(H, W, ss)
    if ss == 0:
        return p
    j0, j1 = np.minimum(2 * np.arange(Wc), W - 1), np.minimum(2 * np.arange(Wc) + 1, W - 1)
    if ss == 1:
        return (p[..., :, j0] + p[..., :, j1]) * 0.5
    i0, i1 = np.minimum(2 * np.arange(Hc), H - 1), np.minimum(2 * np.arange(Hc) + 1, H - 1)
    top, bottom = p[..., i0, :], p[..., i1, :]
    return ((top[..., :, j0] + top[..., :, j1]) + (bottom[..., :, j0] + bottom[..., :, j1])) * 0.25


def rgb_to_ycc(rgb, m, off, L, ss):
    """rgb integers [..., H, W, 3] -> (Y [..., H, W], Cb, Cr [..., Hc, Wc]) int64: the mean of the UNROUNDED values, then + off[k],
    the clamp to [0, L] and the one rounding"""
    off = np.asarray(off, dtype=np.float64).reshape(3)
    p = forward_unrounded(rgb, m)
    return (quantise(p[0] + off[0], L), quantise(chroma_mean(p[1], ss) + off[1], L), quantise(chroma_mean(p[2], ss) + off[2], L))


def ycc_to_rgb(y, cb, cr, n, o, L, ss):
    """planes Y [..., H, W], Cb, Cr [..., Hc, Wc] of integers -> rgb int64 [..., H, W, 3]: position (y, x) reads the chroma sample
    (ss == 2 ? y >> 1 : y, ss ? x >> 1 : x); v_k = (n[k][0] (Y - o[0]) + n[k][1] (Cb - o[1])) + n[k][2] (Cr - o[2])"""
    n = np.asarray(n, dtype=np.float64).reshape(3, 3)
    o = np.asarray(o, dtype=np.float64).reshape(3)
    H, W = y.shape[-2:]
    rows = np.arange(H) >> 1 if ss == 2 else np.arange(H)
    cols = np.arange(W) >> 1 if ss else np.arange(W)
    Y = np.asarray(y).astype(np.float64) - o[0]
    Cb = np.asarray(cb).astype(np.float64)[..., rows, :][..., :, cols] - o[1]
    Cr = np.asarray(cr).astype(np.float64)[..., rows, :][..., :, cols] - o[2]
    return np.stack([quantise((n[k, 0] * Y + n[k, 1] * Cb) + n[k, 2] * Cr, L) for k in range(3)], axis=-1)


def plane_sse(qa, qb):
    """sum (qa - qb)^2 over the last two axes as Python integers: an object array of the leading shape"""
    d = np.asarray(qa, dtype=np.int64) - np.asarray(qb, dtype=np.int64)
    rows = (d * d).sum(axis=-1)                              # (a row of at most 2^26 terms < 2^32: exact in int64)
    lead = rows.shape[:-1]
    flat = rows.reshape(-1, rows.shape[-1])
    out = np.empty(flat.shape[0], dtype=object)
    for i, r in enumerate(flat):
        out[i] = sum(int(v) for v in r)
    return out.reshape(lead)


def ycc_sse(a, b, m, off, L, ss):
    """rgb integers a, b [..., H, W, 3] -> Python-int sums [..., 3] (an object array): per plane the sum of (qa - qb)^2 over the
    integers rgb_to_ycc delivers for a and for b"""
    pa, pb = rgb_to_ycc(a, m, off, L, ss), rgb_to_ycc(b, m, off, L, ss)
    return np.stack([plane_sse(x, y) for x, y in zip(pa, pb)], axis=-1)
