"""The definition of rcb_resample (include/rcb.h, N4 419) on the CPU: the evaluator tests/resample_emul.py against torchaudio's
algorithm restated here in torch fp64 (torchaudio.functional.resample at its defaults: the clamped Hann-windowed sinc kernel,
zero padding of (width, width + o), conv1d with stride o) and against scipy.signal.upfirdn with the prototype filter rebuilt from
the polyphase rows -- a second, independent statement; the deliberate mistakes; the C planner rcb_resample_taps against the
evaluator's taps; rcb_resample_length, rcb_resample_table_bytes, the refusals, and what utils.resample_to_preset refuses."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_emul as E

from recombiner_amd import _lib, config, utils

RATES = E.RATES                                              # the six ratios the header names
L_IN = 4000
UNROUNDED_TOL = 1e-9                                         # (1.5e-11 observed at the worst)
TIE_WINDOW = 1e-9
TIE_SHARE = 1e-4
LONGEST = {(48000, 16000): 37, (44100, 16000): 34, (22050, 16000): 17, (8000, 16000): 13, (16000, 44100): 13, (128000, 16000): 97}
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -3


def _src():
    """s16-magnitude, uniform in +-32768: int16 [2, L_IN, 1]"""
    return np.random.default_rng(0).integers(-32768, 32768, size=(2, L_IN, 1)).astype(np.int16)


def torchaudio_kernel(o, n):
    """torchaudio.functional._get_sinc_resample_kernel for the reduced rates (o, n) at the defaults, in fp64 -> ([n, 1, 2 width + o],
    width)"""
    lowpass_filter_width, rolloff = 6, 0.99
    base_freq = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base_freq)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None, None] / n + idx
    t *= base_freq
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    scale = base_freq / o
    kernels = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t)
    kernels *= window * scale
    return kernels, width


_REFERENCE = {}


def reference(rates):
    """torchaudio's _apply_sinc_resample_kernel on _src() in fp64, unrounded [2, L_out]: computed once per pair of rates"""
    if rates not in _REFERENCE:
        o, n = E.ratio(*rates)
        kernel, width = torchaudio_kernel(o, n)
        x = torch.from_numpy(_src()[..., 0]).double()
        padded = F.pad(x, (width, width + o))
        y = F.conv1d(padded[:, None], kernel, stride=o)
        y = y.transpose(1, 2).reshape(x.shape[0], -1)
        _REFERENCE[rates] = y[..., :math.ceil(n * L_IN / o)].numpy()
    return _REFERENCE[rates]


def _compare(rates, **switches):
    """the evaluator (with `switches`) against the reference -> (largest difference of the unrounded values, number of integers that
    differ away from a tie, share of the samples within TIE_WINDOW of a tie k + 1/2)"""
    a = E.unrounded(_src(), *rates, **switches)[..., 0]
    t = reference(rates)
    assert a.shape == t.shape == (2, E.length(L_IN, *rates))
    diff = float(np.abs(a - t).max())
    near_tie = np.abs((t - np.floor(t)) - 0.5) <= TIE_WINDOW
    differ = E.rounded(a, 3) != E.rounded(t, 3)
    return diff, int((differ & ~near_tie).sum()), float(near_tie.mean())


@pytest.mark.parametrize("rates", RATES, ids=["%d-%d" % r for r in RATES])
def test_the_evaluator_is_torchaudios_algorithm(rates):
    diff, wrong, excluded = _compare(rates)
    print("%d -> %d: unrounded within %.3g of torchaudio's algorithm; %d integers differ away from a tie; %.3g of the samples lie "
          "within %.0e of a tie" % (*rates, diff, wrong, excluded, TIE_WINDOW))
    assert diff <= UNROUNDED_TOL
    assert wrong == 0 and excluded <= TIE_SHARE
    # the rounded result is int16 and clamps: the noise is full scale, and the sinc overshoots
    q = E.resample(_src(), *rates)
    assert q.dtype == np.int16 and q.shape == (2, E.length(L_IN, *rates), 1)


@pytest.mark.parametrize("rates", RATES, ids=["%d-%d" % r for r in RATES])
def test_the_evaluator_is_an_upfirdn(rates):
    """y[q n + p] = sum_k w[p][k] x[q o + k] is upfirdn(h, x, up=n, down=o) delayed by S outputs, with h[S o - u] = w[p][k] for
    u = k n - p o (distinct for every (p, k), as gcd(o, n) = 1 and p < n) and S = ceil(u_max / o)"""
    from scipy.signal import upfirdn
    o, n, first, count, w = E.taps(*rates)
    u = [(int(first[p]) + j) * n - p * o for p in range(n) for j in range(int(count[p]))]
    assert len(set(u)) == len(u)
    S = -(-max(u) // o)
    h = np.zeros(S * o - min(u) + 1)
    for p in range(n):
        for j in range(int(count[p])):
            h[S * o - ((int(first[p]) + j) * n - p * o)] = w[p, j]
    x = _src()[..., 0].astype(np.float64)
    L_out = E.length(L_IN, *rates)
    y = upfirdn(h, x, up=n, down=o, axis=-1)[:, S:S + L_out]
    a = E.unrounded(_src(), *rates)[..., 0]
    diff = float(np.abs(y - a).max())
    print("%d -> %d: within %.3g of scipy's upfirdn (delay %d)" % (*rates, diff, S))
    assert y.shape == a.shape and diff <= UNROUNDED_TOL
    assert float(np.abs(y - reference(rates)).max()) <= UNROUNDED_TOL


# the mistake, and the ratios on which it is one (flipping the sign of the phase changes nothing where there is one phase)
MANY_PHASES = [r for r in RATES if E.ratio(*r)[1] > 1]
MISTAKES = [("no rolloff", dict(rolloff=False), RATES), ("phase sign", dict(flip_phase=True), MANY_PHASES),
            ("scale dropped", dict(scale=False), RATES), ("rectangular window", dict(window=False), RATES),
            ("|t| <= 6, width two short", dict(short=2), RATES)]


@pytest.mark.parametrize("name,switches,where", MISTAKES, ids=[m[0] for m in MISTAKES])
def test_mistakes_fail_the_comparison(name, switches, where):
    assert len(where) >= 4
    for rates in where:
        diff, wrong, _ = _compare(rates, **switches)
        print("%s at %d -> %d: unrounded off by %.3g, %d integers differ" % (name, *rates, diff, wrong))
        assert diff > 1e3 * UNROUNDED_TOL, (name, rates)


def test_width_one_short_is_no_mistake():
    """`|t| <= 6` with `width` one short is the definition itself on every legal ratio, so it cannot fail a comparison: |t| = 6 would
    need k / o - p / n = 6 / base exactly, and the offsets beyond +-(width - 1) are never kept -- on the low side the kept k exceed
    -6 o / base > -width, hence k >= -(width - 1); on the high side they lie below o (n - 1) / n + 6 o / base, and width - 1 + o
    exceeds that because the fraction of 6 o / base (0.06 for enlargements, 6 o / (0.99 n) mod 1 otherwise) is below o / n.  The taps
    are equal bit for bit; the mistake that does bite is two short (above)."""
    for rates in RATES:
        want, got = E.taps(*rates), E.taps(*rates, short=1)
        assert want[:2] == got[:2] and all(np.array_equal(a, b) for a, b in zip(want[2:], got[2:]))


def _c_taps(rate_in, rate_out, max_taps=E.MAX_TAPS, rows=None, null=()):
    lib = _lib.load()
    o, n = ctypes.c_int32(-7), ctypes.c_int32(-7)
    rows = rows or max(E.ratio(max(rate_in, 1), max(rate_out, 1))[1], 1)
    first, count = np.full(rows, -7, dtype=np.int32), np.full(rows, -7, dtype=np.int32)
    w = np.full((rows, max(max_taps, 1)), -7.0)
    args = dict(o=ctypes.byref(o), n=ctypes.byref(n), first=ctypes.c_void_p(first.ctypes.data),
                count=ctypes.c_void_p(count.ctypes.data), w=ctypes.c_void_p(w.ctypes.data))
    for k in null:
        args[k] = None
    rc = lib.rcb_resample_taps(rate_in, rate_out, args["o"], args["n"], args["first"], args["count"], args["w"], max_taps)
    return rc, o.value, n.value, first, count, w


def test_c_planner_against_the_evaluator():
    """o, n, first and count are equal exactly: both sides form t by the same IEEE operations.  The weights: with u = 2^-53, a libm
    result within 1 ulp of the true value (glibc's documented bound for sin and cos, the premise) is off by at most 2 u
    relatively.  w = fl(fl(fl(S / tp) fl(C C)) s) with S = sin(tp) and C = cos(..) from libm on operands that are the same bits on
    both sides: S carries 2 u, C C carries 2 * 2 u, and the four roundings (quotient, square, product, scale) u each -- 10 u per
    side to first order, (1 + 2 u)^3 (1 + u)^4 - 1 < 10.000001 u in full.  Two sides therefore differ by less than 20.00001 u |w|,
    and |w| <= s as |sinc| <= 1 and the window <= 1: the bound is 10.00001 * 2^-52 * s.  (Both sides calling one libm, the observed
    difference is 0; the bound is what holds for any libm within the premise.)"""
    lines = []
    for rates in RATES + [(16000, 16000), (96000, 44100), (11025, 48000)]:
        o, n, first, count, w = E.taps(*rates)
        rc, co, cn, cfirst, ccount, cw = _c_taps(*rates)
        assert rc == int(count.max()) and (co, cn) == (o, n)
        assert np.array_equal(cfirst, first) and np.array_equal(ccount, count)
        s = min(o, n) * 0.99 / o if o != n else 1.0
        bound = 10.00001 * 2.0 ** -52 * s
        worst = float(np.abs(cw - w).max())
        lines.append("%6d -> %6d  %4d : %-4d  longest %2d  worst |w_c - w_numpy| = %.3g = %.3g of the bound %.3g"
                     % (*rates, o, n, rc, worst, worst / bound, bound))
        assert worst <= bound
        for p in range(n):                                   # behind the taps: +0.0
            assert not cw[p, count[p]:].any() and not np.signbit(cw[p, count[p]:]).any()
    print("\n".join(lines))


def test_identity_row_longest_rows_and_lengths():
    assert E.taps(16000, 16000)[:2] == (1, 1)
    rc, o, n, first, count, w = _c_taps(44100, 44100)
    assert (rc, o, n) == (1, 1, 1) and first[0] == 0 and count[0] == 1 and w[0, 0] == 1.0 and not w[0, 1:].any()
    for rates, longest in LONGEST.items():
        assert int(E.taps(*rates)[3].max()) == longest
        assert _c_taps(*rates, null=("first", "count", "w"), max_taps=0)[:3] == (longest, *E.ratio(*rates))      # the query form
    assert utils.RESAMPLE_MAX_TAPS == E.MAX_TAPS == max(LONGEST.values())
    o, n, first, count, w = utils.resample_taps(44100, 16000)
    assert (o, n) == (441, 160) and w.shape == (160, 97) and first.dtype == count.dtype == np.int32
    for L, rates, want in [(700, (48000, 16000), 234), (1600, (48000, 16000), 534), (1500, (44100, 16000), 545), (300, (8000, 16000), 600),
                           (200, (16000, 44100), 552), (4200, (128000, 16000), 525), (5, (128000, 16000), 1), (132300, (44100, 16000), 48000),
                           (300, (16000, 16000), 300), (2 ** 31 - 1, (16000, 44100), -(-441 * (2 ** 31 - 1) // 160))]:
        assert utils.resample_length(L, *rates) == E.length(L, *rates) == want
    lib = _lib.load()
    for rates, longest in LONGEST.items():
        n = E.ratio(*rates)[1]
        assert lib.rcb_resample_table_bytes(*rates) == 8 * n * (1 + longest)
    assert lib.rcb_resample_table_bytes(16000, 16000) == 16


def test_planner_refusals():
    lib = _lib.load()
    for rates in RATES:
        assert E.legal(*rates)
    for rates, code in [((0, 16000), ERR_SHAPE), ((16000, -1), ERR_SHAPE), ((128001, 16000), ERR_UNSUPPORTED),      # 128001 : 16000
                        ((9, 1), ERR_UNSUPPORTED), ((16000, 16001), ERR_UNSUPPORTED),                               # n = 16001
                        ((8191 * 2, 1025 * 2), ERR_UNSUPPORTED), ((8193, 1024), ERR_UNSUPPORTED)]:
        rc, o, n, first, count, w = _c_taps(*rates, rows=4)
        assert rc == code and (o, n) == (-7, -7) and (first == -7).all() and (w == -7.0).all(), rates
        assert lib.rcb_last_error_string()
        assert lib.rcb_resample_table_bytes(*rates) == -1 and lib.rcb_resample_length(100, *rates) == -1
        assert not E.legal(*rates) or code == ERR_SHAPE
        with pytest.raises(_lib.RcbError):
            utils.resample_taps(*rates)
        with pytest.raises(_lib.RcbError):
            utils.resample_length(100, *rates)
    assert _c_taps(8192, 1024)[0] == 97 and _c_taps(8, 1)[0] == 97                                                   # the limits pass
    for null in [("o",), ("n",), ("first",), ("count", "w"), ("w",)]:
        rc, o, n, first, count, w = _c_taps(48000, 16000, null=null)
        assert rc == ERR_ARG and (first == -7).all() and (count == -7).all() and (w == -7.0).all(), null
    rc, o, n, first, count, w = _c_taps(48000, 16000, max_taps=36)
    assert rc == ERR_SHAPE and (o, n) == (-7, -7) and (first == -7).all() and (w == -7.0).all()
    assert _c_taps(48000, 16000, max_taps=37)[0] == 37
    assert lib.rcb_resample_length(0, 48000, 16000) == -1 and lib.rcb_resample_length(2 ** 31, 48000, 16000) == -1
    with pytest.raises(_lib.RcbError, match="samples"):
        utils.resample_length(0, 48000, 16000)


def test_resample_to_preset_refusals():
    """everything it refuses, it refuses before the device is touched (CPU tensors)"""
    audio = config.configs["audio"]
    pn, ps = utils.preset_grid(audio)
    assert pn[0] * ps[0] == 48000 and audio["output_dim"] == 1
    pcm = torch.zeros(1, 132300, 2, dtype=torch.int16)
    with pytest.raises(ValueError, match="data_dim 1"):
        utils.resample_to_preset(config.configs["kodak"], torch.zeros(1, 10, 10, 3), 44100)
    with pytest.raises(ValueError, match="axes"):
        utils.resample_to_preset(audio, pcm[0], 44100)
    with pytest.raises(ValueError, match="2 channels, the preset has 1"):
        utils.resample_to_preset(audio, pcm, 44100, mix=None)
    with pytest.raises(ValueError, match="3 mix weights for 2 channels"):
        utils.resample_to_preset(audio, pcm, 44100, mix=[0.5, 0.25, 0.25])
    with pytest.raises(ValueError, match="mix 'median'"):
        utils.resample_to_preset(audio, pcm, 44100, mix="median")
    with pytest.raises(ValueError, match=r"(?s)ops\.resample.*compress_signals_any"):
        utils.resample_to_preset(audio, pcm[:, :132297], 44100)          # ceil(47 999.2): one output short of the grid
    with pytest.raises(ValueError, match=r"(?s)ops\.resample.*compress_signals_any"):
        utils.resample_to_preset(audio, pcm.transpose(1, 2)[:, :, :1000], 44100, channels_first=True)
    with pytest.raises(_lib.RcbError):
        utils.resample_to_preset(audio, pcm, 16000 * 9)                  # 9 : 1
    stereo = dict(audio, output_dim=2)
    with pytest.raises(ValueError, match="a mix leaves 1 channel"):
        utils.resample_to_preset(stereo, pcm, 44100)
