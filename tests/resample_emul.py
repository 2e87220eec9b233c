"""numpy restatement of rcb_resample (include/rcb.h, N4 419), written from its definition -- not from the kernel.  Everything is
fp64, one IEEE operation per step:

    rates   g = gcd(rate_in, rate_out);  o = rate_in / g;  n = rate_out / g;  o == n: one tap of 1.0 at k = 0
    taps    base = min(o, n) * 0.99;  width = ceil(6.0 * o / base);  s = base / o
            phase p, offset k in [-width, width + o):  t = (-p / n + k / o) * base, kept where |t| < 6
            c = cos(((t * pi) / 6) / 2);  tp = t * pi;  w = ((tp == 0 ? 1 : sin(tp) / tp) * (c * c)) * s
    filter  L_out = ceil(n * L_in / o);  output i = q n + p:  a = ((w_0 v(m_0) + w_1 v(m_0 + 1)) + ...), m_0 = q o + first[p], taps
            ascending, the first product starting the sum; v(m) = +0.0 outside [0, L_in) and multiplied like any other sample
    mix     v(m) = ((g_0 x_0(m) + g_1 x_1(m)) + ...) before the filter, one output channel; without it every channel on its own
    affine  a' = a * gain + bias (two operations), skipped when gain == 1 and bias == 0
    output  s16: rint(min(max(a', -32768), 32767)), half to even;  fp32: float32(a')

sin and cos are Python's math.sin / math.cos (the platform's libm) on operands formed as above.  The filter is an explicit loop
over phases and taps on a zero-padded copy; no index arithmetic is shared with the kernel (no tiles, no staged span).  `taps=`
hands the filter a table from elsewhere (the library's own, in the device tests: the filter is then exact whatever libm did).

Switches for deliberate mistakes (tests/test_resample_emul_cpu.py shows which are caught): rolloff=False (base = min(o, n)),
flip_phase=True (t = (+p / n + k / o) * base), scale=False (w without s), window=False (c * c = 1), short=1 (|t| <= 6 with width
one short; short=2: two short)."""
import functools
import math

import numpy as np

MAX_TAPS = 97
RATES = [(48000, 16000), (44100, 16000), (22050, 16000), (8000, 16000), (16000, 44100), (128000, 16000)]


def ratio(rate_in, rate_out):
    g = math.gcd(int(rate_in), int(rate_out))
    return int(rate_in) // g, int(rate_out) // g


def legal(rate_in, rate_out):
    o, n = ratio(rate_in, rate_out)
    return o == n or (o <= 8 * n and n <= 1024 and o <= 8192)


def length(L_in, rate_in, rate_out):
    o, n = ratio(rate_in, rate_out)
    return -((-n * int(L_in)) // o)                          # ceil in integer arithmetic


@functools.lru_cache(maxsize=None)
def taps(rate_in, rate_out, rolloff=True, flip_phase=False, scale=True, window=True, short=0):
    """-> (o, n, first int32 [n] (offsets k, negative ones included), count int32 [n], w float64 [n, MAX_TAPS] padded with +0.0);
    computed once per set of arguments, and not to be written to"""
    o, n = ratio(rate_in, rate_out)
    first, count = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    w = np.zeros((n, MAX_TAPS), dtype=np.float64)
    if o == n:
        count[0], w[0, 0] = 1, 1.0
        return o, n, first, count, w
    f = np.float64
    base = f(min(o, n)) * (f(0.99) if rolloff else f(1.0))
    width = int(math.ceil(f(6.0) * f(o) / base)) - short
    s = base / f(o)
    pi = f(math.pi)
    for p in range(n):
        ph = -f(p) / f(n)
        kept = []
        for k in range(-width, width + o):
            t = ((-ph if flip_phase else ph) + f(k) / f(o)) * base
            if (abs(t) <= 6.0) if short else (abs(t) < 6.0):
                c = f(math.cos(((t * pi) / f(6.0)) / f(2.0))) if window else f(1.0)
                tp = t * pi
                sinc = f(1.0) if tp == 0.0 else f(math.sin(tp)) / tp
                kept.append((k, (sinc * (c * c)) * s if scale else sinc * (c * c)))
        ks = [k for k, _ in kept]
        if not ks:                                           # (only a mistake leaves a phase without taps: one tap of 0.0)
            assert flip_phase
            count[p] = 1
            continue
        assert ks == list(range(ks[0], ks[0] + len(ks))) and len(ks) <= MAX_TAPS, (o, n, p)
        first[p], count[p] = ks[0], len(ks)
        w[p, :len(ks)] = [v for _, v in kept]
    return o, n, first, count, w


def mixed(src, mix=None):
    """src [n_sig, L, C] (int16 or float32) -> the fp64 values the filter reads, [n_sig, L, C_out]"""
    x = np.asarray(src).astype(np.float64)                   # (int16 and float32 are exact in fp64)
    if mix is None:
        return x
    g = np.asarray(mix, dtype=np.float64).reshape(-1)
    assert g.size == x.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        v = g[0] * x[..., 0]
        for c in range(1, g.size):
            v = v + g[c] * x[..., c]
    return v[..., None]


def filtered(v, tp, length_out=None):
    """v fp64 [n_sig, L, C] -> the unrounded outputs [n_sig, length_out, C] with the taps tp = (o, n, first, count, w)"""
    o, n, first, count, w = tp
    L = v.shape[1]
    L_out = -((-n * L) // o)
    length_out = L_out if length_out is None else int(length_out)
    assert 1 <= length_out <= L_out
    q_max = (length_out - 1) // n
    left = max(0, -int(first.min()))
    right = max(0, q_max * o + int((first + count).max()) - L)
    pad = np.zeros((v.shape[0], left + L + right, v.shape[2]), dtype=np.float64)             # +0.0
    pad[:, left:left + L] = v
    out = np.empty((v.shape[0], length_out, v.shape[2]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(min(n, length_out)):
            q = np.arange((length_out - 1 - p) // n + 1)
            m0 = q * o + int(first[p]) + left
            acc = w[p, 0] * pad[:, m0]
            for j in range(1, int(count[p])):
                acc = acc + w[p, j] * pad[:, m0 + j]
            out[:, q * n + p] = acc
    return out


def unrounded(src, rate_in, rate_out, mix=None, gain=1.0, bias=0.0, length_out=None, taps_from=None, **switches):
    tp = taps(rate_in, rate_out, **switches) if taps_from is None else taps_from
    a = filtered(mixed(src, mix), tp, length_out)
    if not (gain == 1.0 and bias == 0.0):
        with np.errstate(invalid="ignore", over="ignore"):
            a = a * np.float64(gain) + np.float64(bias)
    return a


def rounded(a, kind):
    """the output rule: kind 3 int16, kind 1 float32"""
    if kind == 1:
        with np.errstate(over="ignore", invalid="ignore"):
            return a.astype(np.float32)
    assert kind == 3
    return np.rint(np.minimum(np.maximum(a, -32768.0), 32767.0)).astype(np.int16)


def resample(src, rate_in, rate_out, **kw):
    """-> the resampled array of the source's dtype (int16: kind 3, float32: kind 1)"""
    src = np.asarray(src)
    return rounded(unrounded(src, rate_in, rate_out, **kw), 3 if src.dtype == np.int16 else 1)
