"""numpy restatement of rcb_resize (include/rcb.h, N4 416), written from its definition -- not from the kernel.  Everything is
fp64, one IEEE operation per step:

    taps    scale = n_in / n_out;  support = max(scale, 1);  inv = 1 / scale when scale >= 1, else 1
            center = scale * (i + 0.5);  first = max(trunc((center - support) + 0.5), 0);  last = min(trunc((center + support) + 0.5),
            n_in);  g_j = max(0, 1 - |(((first + j) - center) + 0.5) * inv|);  w_j = g_j / ((g_0 + g_1) + ...)
            n_in == n_out: first = i, one tap of 1.0
    filter  the last spatial axis first, taps ascending, the first product starting the sum; the row-filtered values stay fp64
    output  integers: rint(min(max(a, 0), L)), half to even, ONE rounding;  fp32: float32(a)

Both passes are explicit loops over the taps; no index arithmetic is shared with the kernel (no tiles, no chunks).

Switches for deliberate mistakes (tests/test_resize_emul_cpu.py shows that each is caught): antialias=False (support 1 when
reducing), round_between=True (the integer rounding also between the passes), half_pixel=False (centres without the 0.5),
normalise=False (w_j = g_j), first_axis_first=True (the passes exchanged)."""
import numpy as np

MAX_TAPS = 33


def taps(n_in, n_out, antialias=True, half_pixel=True, normalise=True):
    """-> (first int32 [n_out], count int32 [n_out], w float64 [n_out, MAX_TAPS] padded with +0.0)"""
    n_in, n_out = int(n_in), int(n_out)
    scale = np.float64(n_in) / np.float64(n_out)
    reducing = bool(scale >= 1.0) and antialias
    support = scale if reducing else np.float64(1.0)
    inv = np.float64(1.0) / scale if reducing else np.float64(1.0)
    first, count = np.zeros(n_out, dtype=np.int32), np.zeros(n_out, dtype=np.int32)
    w = np.zeros((n_out, MAX_TAPS), dtype=np.float64)
    half = np.float64(0.5)
    if n_in == n_out:                                        # the identity: one tap of 1.0 (the tap of weight 0 behind it is dropped)
        first[:], count[:], w[:, 0] = np.arange(n_out), 1, 1.0
        return first, count, w
    for i in range(n_out):
        center = scale * (np.float64(i) + (half if half_pixel else np.float64(0.0)))
        f = max(int((center - support) + half), 0)           # int() truncates
        last = min(int((center + support) + half), n_in)
        n = last - f
        assert 1 <= n <= MAX_TAPS, (n_in, n_out, i, n)
        g = [max(np.float64(0.0), np.float64(1.0) - abs(((np.float64(f + j) - center) + half) * inv)) for j in range(n)]
        total = g[0]
        for j in range(1, n):
            total = total + g[j]
        for j in range(n):
            w[i, j] = g[j] / total if normalise else g[j]
        first[i], count[i] = f, n
    return first, count, w


def _pass(v, axis, tp):
    """one pass along `axis` of the fp64 array v: out[i] = ((w0 v[f] + w1 v[f + 1]) + ...), an explicit loop over the taps"""
    first, count, w = tp
    v = np.moveaxis(v, axis, -1)
    out = np.empty(v.shape[:-1] + (len(first),), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(first)):
            f = int(first[i])
            acc = w[i, 0] * v[..., f]
            for j in range(1, int(count[i])):
                acc = acc + w[i, j] * v[..., f + j]
            out[..., i] = acc
    return np.moveaxis(out, -1, axis)


def level_max(kind, depth=0):
    return 255 if kind == 0 else (1 << depth) - 1


def _round(a, L):
    return np.rint(np.minimum(np.maximum(a, 0.0), np.float64(L)))


def unrounded(src, size, round_between=False, first_axis_first=False, L=255, **tap_switches):
    """src [..., H, W, C] (any number of leading axes) -> the fp64 values a [..., H_out, W_out, C] before the output rule"""
    v = np.asarray(src).astype(np.float64)                   # (uint8, uint16 and float32 are exact in fp64)
    H, W = v.shape[-3], v.shape[-2]
    ty, tx = taps(H, size[0], **tap_switches), taps(W, size[1], **tap_switches)
    order = [(-3, ty), (-2, tx)] if first_axis_first else [(-2, tx), (-3, ty)]
    t = _pass(v, *order[0])
    if round_between:
        t = _round(t, L)
    return _pass(t, *order[1])


def resize(src, size, kind=0, depth=0, **switches):
    """-> the resized array of the source's dtype: kind 0 uint8, 1 float32, 2 uint16 at `depth`"""
    L = level_max(kind, depth) if kind != 1 else 0
    a = unrounded(src, size, L=L, **switches)
    if kind == 1:
        with np.errstate(over="ignore", invalid="ignore"):
            return a.astype(np.float32)
    return _round(a, L).astype(np.uint8 if kind == 0 else np.uint16)


def ties(src, size, L=255):
    """how many exact ties k + 1/2 the output rule meets -> (k even, k odd)"""
    a = unrounded(src, size, L=L)
    k = np.floor(a)
    tie = (a - k == 0.5) & (a > 0) & (a < L)
    return int((tie & (k % 2 == 0)).sum()), int((tie & (k % 2 == 1)).sum())


def center_crop_start(n, size):
    """torchvision's rule, with Python's round"""
    return int(round((n - size) / 2.0))
