"""rcb_resample (N4 419) against the numpy evaluator of its definition (tests/resample_emul.py): every comparison is bit for bit --
int16 as integers, fp32 through an int32 view with generated NaNs mapped to one pattern (their sign differs between x86 and the
GPU: tests/test_hip_resize.py).  The evaluator is fed THE LIBRARY'S OWN taps (utils.resample_taps), as the posterior tests feed
tapped device values: the filter is then exact whatever libm did; tests/test_resample_emul_cpu.py holds the taps themselves.

The kernel works on tiles of 256 consecutive outputs of one signal and stages the samples a tile needs in LDS (csrc/resample.hip:
kTile).  The shapes are the smallest at which that can still go wrong: the identity, a partial tile, three tiles, phases that wrap
inside and across tiles (441 : 160), enlargement by 2 and by 441 / 160 (more phases than a tile has outputs), 8 : 1 with its 97
taps, the largest span and the padded LDS index, a source shorter than a tap row, and the cut to the first `length` outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_emul as E

pytestmark = pytest.mark.gpu

from recombiner_amd import _lib, ops, utils  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

DEV = "cuda"
TILE = 256
# (rate_in, rate_out), L_in, outputs
CASES = [((16000, 16000), 300, 300), ((48000, 16000), 700, 234), ((48000, 16000), 1600, 534), ((44100, 16000), 1500, 545),
         ((8000, 16000), 300, 600), ((16000, 44100), 200, 552), ((128000, 16000), 4200, 525), ((128000, 16000), 5, 1)]
IDS = ["%d-%d-%d" % (*r, L) for r, L, _ in CASES]
OPERANDS = ["s16_noise", "s16_square", "f32_specials", "f32_affine"]
KIND = {np.dtype(np.int16): 3, np.dtype(np.float32): 1}
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -3
SENT = 0x5A
S16 = SampleFormat.s16()


def make(operand, shape, seed=0):
    """a source [n, L, C] of the operand's numpy dtype"""
    rng = np.random.default_rng(seed)
    n, L, Cc = shape
    if operand == "s16_noise":
        return rng.integers(-32768, 32768, shape).astype(np.int16)
    if operand == "s16_square":                              # full scale, period 14, every signal and channel at its own phase
        m = np.arange(L)[None, :, None] + 3 * np.arange(n)[:, None, None] + 5 * np.arange(Cc)[None, None, :]
        return np.where(m % 14 < 7, 32767, -32768).astype(np.int16)
    a = rng.standard_normal(shape).astype(np.float32)
    if operand == "f32_specials":                            # the special values of tests/test_hip_resize.py's make
        flat = a.reshape(-1)
        for k, v in enumerate([0.0, -0.0, 1e-40, -3e-42, np.inf, np.nan, 3e38, -3e38]):
            flat[(7 + 13 * k) % flat.size] = np.float32(v)
    return a


def affine_of(operand):
    return dict(gain=0.5, bias=0.5) if operand == "f32_affine" else {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.contiguous().cpu().numpy()


def bits(a):
    """what is compared: int16 as it is; fp32 as int32, every NaN as one pattern (see the module text)"""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    b = a.view(np.int32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


_TAPS = {}


def lib_taps(rates):
    if rates not in _TAPS:
        _TAPS[rates] = utils.resample_taps(*rates)
    return _TAPS[rates]


def expect(src, rates, length=None, mix=None, gain=1.0, bias=0.0):
    """the evaluator on the library's taps -> the array of the source's dtype"""
    return E.resample(src, *rates, taps_from=lib_taps(rates), length_out=length, mix=mix, gain=gain, bias=bias)


def same(got, want):
    if want.dtype == np.float32 and not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def _guarded(n_bytes, pad=64):
    big = torch.full((n_bytes + 2 * pad,), SENT, device=DEV, dtype=torch.uint8)

    def check():
        assert bool((big[:pad] == SENT).all().item()) and bool((big[pad + n_bytes:] == SENT).all().item())
    return big[pad:pad + n_bytes], check


def raw(t, rates, length=None, mix=None, gain=1.0, bias=0.0, **over):
    """rcb_resample on the device tensor t [n, L, C] (any strides) with guard bytes on both sides of dst and of the table -> (rc, the
    output as numpy or None, untouched: whether dst still holds its sentinel).  `over` replaces single arguments (the refusals)."""
    lib = _lib.load()
    store = t.untyped_storage()
    L_out = E.length(int(t.shape[1]), *rates)
    g = dict(kind=KIND[np.dtype(str(t.dtype).split(".")[1])], n=int(t.shape[0]), L=int(t.shape[1]), C=int(t.shape[2]),
             strides=[int(v) for v in t.stride()], offset=int(t.storage_offset()), rate_in=rates[0], rate_out=rates[1],
             length=L_out if length is None else length, src_elems=store.nbytes() // t.element_size(), null=(), table_delta=0,
             table_shift=0)
    g.update(over)
    shape = (int(t.shape[0]), L_out if length is None else length, 1 if mix is not None else int(t.shape[2]))
    n_out = int(np.prod(shape)) * t.element_size()
    dst, check_d = _guarded(max(n_out, 8))
    need = int(lib.rcb_resample_table_bytes(*rates))
    table, check_t = _guarded(max(need, 8) + 8)
    assert dst.data_ptr() % 8 == 0 and table.data_ptr() % 8 == 0
    mix_arr = None if mix is None else np.ascontiguousarray(mix, dtype=np.float64)
    rc = lib.rcb_resample(None if "src" in g["null"] else C.c_void_p(store.data_ptr()), g["src_elems"], g["kind"], g["n"], g["L"], g["C"],
                          None if "strides" in g["null"] else (C.c_int64 * 3)(*g["strides"]), g["offset"], g["rate_in"], g["rate_out"],
                          None if mix_arr is None else C.c_void_p(mix_arr.ctypes.data), gain, bias, g["length"],
                          None if "dst" in g["null"] else C.c_void_p(dst.data_ptr()),
                          None if "table" in g["null"] else C.c_void_p(table.data_ptr() + g["table_shift"]),
                          max(need, 0) + g["table_delta"], ops.stream_ptr())
    torch.cuda.synchronize()
    check_d(), check_t()
    untouched = bool((dst == SENT).all().item())
    if rc != 0 or n_out == 0:
        return rc, None, untouched
    return rc, host(dst[:n_out].view(t.dtype).view(shape)), untouched


@pytest.mark.parametrize("operand", OPERANDS)
@pytest.mark.parametrize("rates,L,outputs", CASES, ids=IDS)
def test_shapes_operands_and_channels(rates, L, outputs, operand):
    """through the C entry, guard bytes on both sides of dst and of the table; C = 1, 2, 3 kept"""
    assert E.length(L, *rates) == outputs
    past = np.zeros(2, dtype=np.int64)
    for Cc in (1, 2, 3):
        src = make(operand, (2, L, Cc), seed=Cc)
        kw = affine_of(operand)
        rc, got, _ = raw(dev(src), rates, **kw)
        want = expect(src, rates, **kw)
        assert rc == 0 and want.shape == (2, outputs, Cc)
        assert same(got, want), (rates, L, operand, Cc)
        if rates[0] == rates[1] and not kw:                  # the identity returns the source, whatever it holds: the raw bits
            assert np.array_equal(got.view(np.int16 if src.dtype == np.int16 else np.int32),
                                  src.view(np.int16 if src.dtype == np.int16 else np.int32))
        if operand == "s16_square":
            a = E.unrounded(src, *rates, taps_from=lib_taps(rates))
            past += [(a > 32767.0).sum(), (a < -32768.0).sum()]
            assert got.max() <= 32767 and got.min() >= -32768
    if operand == "s16_square" and (rates, L) in [((48000, 16000), 1600), ((44100, 16000), 1500), ((8000, 16000), 300)]:
        assert past.min() > 50, past                         # (the clamp is exercised at both limits)
    if operand == "f32_specials" and L >= 200:
        assert np.isnan(want).any() and np.isfinite(want).any()


@pytest.mark.parametrize("rates,L,outputs", CASES[1:], ids=IDS[1:])
def test_channels_mixed_to_one(rates, L, outputs):
    """the mix is formed in fp64 before the filter: mean weights and uneven ones, two and three channels, both kinds"""
    for Cc, mix in [(2, [0.5, 0.5]), (3, [1.0 / 3] * 3), (2, [0.75, -0.125]), (3, [0.6, 0.3, 0.1])]:
        for operand in ("s16_noise", "f32_affine"):
            src = make(operand, (2, L, Cc), seed=10 + Cc)
            kw = affine_of(operand)
            rc, got, _ = raw(dev(src), rates, mix=mix, **kw)
            want = expect(src, rates, mix=mix, **kw)
            assert rc == 0 and want.shape == (2, outputs, 1) and same(got, want), (rates, Cc, mix, operand)
    one = make("s16_noise", (1, L, 1), seed=3)               # a mix of one channel is a gain
    assert same(host(ops.resample(dev(one), *rates, sample_format=S16, mix=[0.5])), expect(one, rates, mix=[0.5]))


def test_the_first_outputs_come_from_the_whole_source():
    """length=100 of 234: the first 100 outputs of the full result, not the result of a shorter source"""
    rates, L = (48000, 16000), 700
    src = make("s16_noise", (2, L, 2), seed=4)
    full = expect(src, rates)
    rc, got, _ = raw(dev(src), rates, length=100)
    assert rc == 0 and same(got, np.ascontiguousarray(full[:, :100])) and same(got, expect(src, rates, length=100))
    short = expect(src[:, :300], rates)
    assert short.shape[1] == 100 and not np.array_equal(short, got)
    out = ops.resample(dev(src), *rates, sample_format=S16, length=100)
    assert tuple(out.shape) == (2, 100, 2) and same(host(out), got)
    for length in (1, TILE, TILE + 1):                       # a whole tile, and one output into the next
        src1 = make("f32_specials", (1, 1600, 1), seed=length)
        assert same(host(ops.resample(dev(src1), *rates, length=length)), expect(src1, rates, length=length))


def test_views_go_to_the_kernel_as_they_are():
    """channel-first storage, a window of a longer buffer at a non-zero offset, an expanded channel and three signals through a
    signal stride: each equals the evaluator on the view's values, and nothing is made contiguous"""
    rates = (44100, 16000)
    seen = []

    def check(view, **kw):
        assert not view.is_contiguous()
        fmt = S16 if view.dtype == torch.int16 else None
        got = ops.resample(view, *rates, sample_format=fmt, **kw)
        assert got.is_contiguous() and same(host(got), expect(host(view), rates, **kw))
        seen.append(view)

    cf = dev(make("s16_noise", (2, 2, 1500), seed=1))        # [n, C, L]
    check(cf.transpose(1, 2))
    check(cf.transpose(1, 2), mix=[0.5, 0.5])
    long = dev(make("s16_noise", (3, 2500, 2), seed=2))
    win = long[:, 700:2200]
    assert win.storage_offset() > 0
    check(win)
    check(long[1:, 700:2200], mix=[0.25, 0.75])              # (the offset carries a whole signal as well)
    mono = dev(make("f32_specials", (2, 1500, 1), seed=3)).expand(2, 1500, 3)
    assert mono.stride(-1) == 0
    check(mono)
    many = dev(make("s16_square", (6, 1500, 1), seed=4))
    three = many[::2]
    assert three.shape[0] == 3 and three.stride(0) == 2 * 1500
    check(three)
    assert len(seen) == 6


def test_a_signal_alone_in_its_batch_and_twice():
    for rates, L in [((44100, 16000), 1500), ((128000, 16000), 4200)]:
        src = make("s16_noise", (3, L, 2), seed=8)
        t = dev(src)
        got = ops.resample(t, *rates, sample_format=S16)
        assert got.dtype == torch.int16 and got.is_contiguous() and same(host(got), expect(src, rates))
        assert torch.equal(ops.resample(t, *rates, sample_format=S16), got)
        out = torch.empty_like(got)
        assert ops.resample(t, *rates, sample_format=S16, out=out) is out and torch.equal(out, got)
        alone = ops.resample(t[1][None], *rates, sample_format=S16)
        assert torch.equal(alone[0], got[1])
        f = dev(make("f32_specials", (3, L, 1), seed=9))
        gf = ops.resample(f, *rates, mix=[1.0], gain=0.5, bias=0.5)
        assert np.array_equal(bits(host(ops.resample(f[2][None], *rates, mix=[1.0], gain=0.5, bias=0.5)[0])), bits(host(gf[2])))
        assert np.array_equal(bits(host(ops.resample(f, *rates, mix=[1.0], gain=0.5, bias=0.5))), bits(host(gf)))


def test_no_signals():
    t = torch.empty(0, 700, 2, dtype=torch.int16, device=DEV)
    out = ops.resample(t, 48000, 16000, sample_format=S16)
    assert tuple(out.shape) == (0, 234, 2)
    rc, _, untouched = raw(dev(make("s16_noise", (1, 700, 2))), (48000, 16000), n=0, null=("src", "dst", "table"))
    assert rc == 0 and untouched


def test_wrapper_checks():
    pcm = dev(make("s16_noise", (1, 700, 2)))
    with pytest.raises(ValueError, match="sample_format"):
        ops.resample(pcm, 48000, 16000)
    with pytest.raises(_lib.RcbError, match="GPU"):
        ops.resample(pcm.cpu(), 48000, 16000, sample_format=S16)
    with pytest.raises(_lib.RcbError, match="must be"):
        ops.resample(pcm[0], 48000, 16000, sample_format=S16)
    with pytest.raises(_lib.RcbError, match="output of shape"):
        ops.resample(pcm, 48000, 16000, sample_format=S16, out=torch.empty(1, 234, 2, device=DEV))
    with pytest.raises(ValueError, match="3 mix weights for 2 channels"):
        ops.resample(pcm, 48000, 16000, sample_format=S16, mix=[1, 2, 3])
    with pytest.raises(_lib.RcbError, match="kind 0"):
        ops.resample(pcm.to(torch.uint8), 48000, 16000)
    with pytest.raises(_lib.RcbError, match="kind 2"):
        ops.resample(pcm, 48000, 16000, sample_format=SampleFormat.u16(16))
    with pytest.raises(_lib.RcbError, match="8 : 1"):
        ops.resample(pcm, 9, 1, sample_format=S16)
    with pytest.raises(_lib.RcbError, match="outputs asked"):
        ops.resample(pcm, 48000, 16000, sample_format=S16, length=235)
    with pytest.raises(_lib.RcbError, match="reads"):
        ops.resample(pcm, 48000, 16000, sample_format=SampleFormat.f32())


def test_refusals_launch_nothing():
    """every refusal of the header: its code, and dst keeps its sentinel"""
    rates = (48000, 16000)
    src = make("s16_noise", (2, 700, 2), seed=9)
    t = dev(src)
    rc, got, _ = raw(t, rates)
    assert rc == 0 and same(got, expect(src, rates))
    st = [int(v) for v in t.stride()]
    need_elems = t.numel()
    cases = [
        (dict(kind=0), ERR_ARG), (dict(kind=2), ERR_ARG), (dict(kind=4), ERR_ARG), (dict(kind=-1), ERR_ARG),
        (dict(strides=[st[0], -st[1], st[2]]), ERR_ARG), (dict(strides=[-1] + st[1:]), ERR_ARG), (dict(offset=-1), ERR_ARG),
        (dict(null=("src",)), ERR_ARG), (dict(null=("dst",)), ERR_ARG), (dict(null=("strides",)), ERR_ARG), (dict(null=("table",)), ERR_ARG),
        (dict(C=0), ERR_SHAPE), (dict(C=9, strides=[st[0], st[1], 0]), ERR_SHAPE), (dict(n=-1), ERR_SHAPE), (dict(L=0), ERR_SHAPE),
        (dict(rate_in=0), ERR_SHAPE), (dict(rate_out=-16000), ERR_SHAPE),
        (dict(length=0), ERR_SHAPE), (dict(length=-1), ERR_SHAPE), (dict(length=235), ERR_SHAPE),
        (dict(src_elems=need_elems - 1), ERR_SHAPE), (dict(offset=1), ERR_SHAPE), (dict(n=3), ERR_SHAPE), (dict(L=701, length=234), ERR_SHAPE),
        (dict(C=3), ERR_SHAPE), (dict(strides=[st[0], 1 << 62, st[2]]), ERR_SHAPE),
        (dict(table_delta=-1), ERR_SHAPE), (dict(table_shift=4), ERR_SHAPE),
        (dict(rate_in=9, rate_out=1, length=1), ERR_UNSUPPORTED), (dict(rate_in=16000, rate_out=16001, length=1), ERR_UNSUPPORTED),
        (dict(rate_in=8193, rate_out=1024, length=1), ERR_UNSUPPORTED),
        (dict(rate_in=1, rate_out=2, L=(1 << 31) - 1, strides=[0, 0, 0], length=1), ERR_UNSUPPORTED),      # 2^32 - 2 outputs
        (dict(n=1 << 31, strides=[0] + st[1:]), ERR_UNSUPPORTED),                                         # 2^31 workgroups
    ]
    for over, code in cases:
        rc, _, untouched = raw(t, rates, **over)
        assert rc == code and untouched, (over, rc)
        assert _lib.load().rcb_last_error_string()
    # ... and the limits themselves pass
    rc, got, _ = raw(t, rates, src_elems=need_elems)
    assert rc == 0
    wide = make("s16_noise", (1, 64, 8), seed=1)             # eight channels
    rc, got, _ = raw(dev(wide), (8000, 16000))
    assert rc == 0 and same(got, expect(wide, (8000, 16000)))
