"""rcb_resize (N4 416) against the numpy evaluator of its definition (tests/resize_emul.py): every comparison is bit for bit --
integers as integers, fp32 through an int32 view.

The kernel works on tiles of 8 x 32 output positions and takes the input rows of a tile in LDS chunks of 32 (csrc/resize.hip: kTY,
kTX, kRows).  The shapes are the smallest at which it can still go wrong: the identity, the 240 -> 128 ratio, non-integer scales,
partial tiles on both axes and more than one of each, enlargement, 2 : 1 with exact ties, and 16 : 1 on the row axis (32 taps,
7 * 16 + 32 = 144 input rows per tile: five chunks).

NaNs: IEEE 754 leaves the sign and payload of a GENERATED NaN open (0 * inf is the negative default NaN on x86 and the positive
one on the GPU), so both sides' NaNs are mapped to one pattern before the int32 view; that a NaN stands where the evaluator has one
is asserted, and the identity, which generates none, is compared on the raw bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import resize_emul as E

pytestmark = pytest.mark.gpu

from recombiner_amd import _lib, ops  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

DEV = "cuda"
SHAPES = [((16, 16), (16, 16)), ((30, 30), (16, 16)), ((37, 53), (16, 16)), ((45, 70), (19, 33)), ((7, 5), (16, 16)),
          ((32, 16), (16, 8)), ((272, 40), (17, 20))]
FMTS = {"u8": (0, 0), "u16_10": (2, 10), "u16_16": (2, 16), "f32": (1, 0)}
NP_DTYPE = {0: np.uint8, 1: np.float32, 2: np.uint16}
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -3
SENT = 0x5A


def make(fmt, shape, seed=0):
    """a source of `shape` in the format's numpy dtype"""
    kind, depth = fmt
    rng = np.random.default_rng(seed)
    if kind == 1:
        a = rng.standard_normal(shape).astype(np.float32)
        flat = a.reshape(-1)
        special = [0.0, -0.0, 1e-40, -3e-42, np.inf, np.nan, 3e38, -3e38]
        for k, v in enumerate(special):
            flat[(7 + 13 * k) % flat.size] = np.float32(v)
        return a
    L = E.level_max(kind, depth)
    a = rng.integers(0, L + 1, shape)
    if kind == 2 and depth < 16:                             # stored values above L: in as they are, out clamped
        a.reshape(-1)[::5] = 65535
        a.reshape(-1)[3::11] = L + 1
    return a.astype(NP_DTYPE[kind])


def dev(a):
    """numpy -> a device tensor of the same bits (uint16 through its int16 view)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def host(t):
    """a device tensor (any strides) -> numpy of the same bits"""
    t = t.contiguous()
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def bits(a):
    """what is compared: integers as they are; fp32 as int32, every NaN as one pattern (see the module text)"""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    b = a.view(np.int32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def expect(src, size, fmt):
    return E.resize(src, size, kind=fmt[0], depth=fmt[1])


def _guarded(n_bytes, pad=64):
    big = torch.full((n_bytes + 2 * pad,), SENT, device=DEV, dtype=torch.uint8)

    def check():
        assert bool((big[:pad] == SENT).all().item()) and bool((big[pad + n_bytes:] == SENT).all().item())
    return big[pad:pad + n_bytes], check


def raw(t, size, fmt, **over):
    """rcb_resize on the device tensor t ([n, H, W, C] or [n, T, H, W, C], any strides) with guard bytes on both sides of dst and
    of the table -> (rc, the output as numpy or None, untouched: whether dst still holds its sentinel).  `over` replaces single
    arguments (the refusals)."""
    lib = _lib.load()
    clip = t.dim() == 5
    st = [int(v) for v in t.stride()]
    store = t.untyped_storage()
    g = dict(kind=fmt[0], depth=fmt[1], n=int(t.shape[0]), T=int(t.shape[1]) if clip else 1, H=int(t.shape[-3]), W=int(t.shape[-2]),
             C=int(t.shape[-1]), strides=[st[0], st[1] if clip else 0] + st[-3:], offset=int(t.storage_offset()), Ho=int(size[0]),
             Wo=int(size[1]), src_elems=store.nbytes() // t.element_size(), null=(), table_delta=0, table_shift=0)
    g.update(over)
    shape = (int(t.shape[0]), *([int(t.shape[1])] if clip else []), int(size[0]), int(size[1]), int(t.shape[-1]))
    n_out = int(np.prod(shape)) * t.element_size()
    dst, check_d = _guarded(max(n_out, 8))
    need = int(lib.rcb_resize_table_bytes(int(t.shape[-3]), int(t.shape[-2]), int(size[0]), int(size[1])))
    table, check_t = _guarded(max(need, 8) + 8)
    assert dst.data_ptr() % 8 == 0 and table.data_ptr() % 8 == 0
    rc = lib.rcb_resize(None if "src" in g["null"] else C.c_void_p(store.data_ptr()), g["src_elems"], g["kind"], g["depth"], g["n"],
                        g["T"], g["H"], g["W"], g["C"], None if "strides" in g["null"] else (C.c_int64 * 5)(*g["strides"]), g["offset"],
                        g["Ho"], g["Wo"], None if "dst" in g["null"] else C.c_void_p(dst.data_ptr()),
                        None if "table" in g["null"] else C.c_void_p(table.data_ptr() + g["table_shift"]), max(need, 0) + g["table_delta"],
                        ops.stream_ptr())
    torch.cuda.synchronize()
    check_d(), check_t()
    untouched = bool((dst == SENT).all().item())
    if rc != 0 or n_out == 0:
        return rc, None, untouched
    return rc, host(dst[:n_out].view(t.dtype).view(shape)), untouched


@pytest.mark.parametrize("name", list(FMTS))
@pytest.mark.parametrize("hw,size", SHAPES, ids=["%dx%d-%dx%d" % (*a, *b) for a, b in SHAPES])
def test_shapes_formats_and_channels(hw, size, name):
    """through the C entry, guard bytes on both sides of dst and of the table"""
    fmt = FMTS[name]
    for Cc in (1, 3, 4):
        src = make(fmt, (2, *hw, Cc), seed=Cc)
        rc, got, _ = raw(dev(src), size, fmt)
        want = expect(src, size, fmt)
        assert rc == 0 and got.dtype == want.dtype and got.shape == want.shape == (2, *size, Cc)
        if fmt[0] == 1:
            assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(bits(got), bits(want)), (hw, size, name, Cc)
        if hw == size:                                       # the identity returns the source, whatever it holds: the raw bits
            if fmt[0] == 1:                                  # of fp32, the integers (a stored value above L clamped to L: the
                assert np.array_equal(got.view(np.int32), src.view(np.int32))         # output rule holds for the identity too)
            else:
                assert np.array_equal(got, np.minimum(src, E.level_max(*fmt)))
    if name == "u16_10":                                     # (the stored values above L were there, and came out clamped)
        assert src.max() == 65535 and got.max() <= 1023


def test_exact_ties_round_half_to_even():
    """2 : 1: inner weights (1, 3, 3, 1) / 8 on both axes, so the values are multiples of 1 / 64 and exact ties k + 1/2 occur, for
    even and for odd k; the evaluator counts them"""
    src = make(FMTS["u8"], (4, 32, 16, 3), seed=21)
    even, odd = E.ties(src, (16, 8))
    assert even > 0 and odd > 0
    got = host(ops.resize(dev(src), (16, 8)))
    assert np.array_equal(got, expect(src, (16, 8), FMTS["u8"]))
    src16 = make(FMTS["u16_16"], (4, 32, 16, 1), seed=22)
    even, odd = E.ties(src16, (16, 8), L=65535)
    assert even > 0 and odd > 0
    got = host(ops.resize(dev(src16), (16, 8), sample_format=SampleFormat.u16(16)))
    assert np.array_equal(got, expect(src16, (16, 8), FMTS["u16_16"]))


def test_clips_and_frames_alone():
    """[n, T, H, W, C] with n = 2, T = 3; a frame resized alone is that frame of its batch; two launches give the same bits"""
    src = make(FMTS["u8"], (2, 3, 45, 70, 3), seed=5)
    t = dev(src)
    got = ops.resize(t, (19, 33))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3, 19, 33, 3) and got.is_contiguous()
    want = expect(src, (19, 33), FMTS["u8"])
    assert np.array_equal(host(got), want)
    assert torch.equal(ops.resize(t, (19, 33)), got)
    out = torch.empty_like(got)
    assert ops.resize(t, (19, 33), out=out) is out and torch.equal(out, got)
    alone = ops.resize(t[1, 2][None], (19, 33))
    assert tuple(alone.shape) == (1, 19, 33, 3) and torch.equal(alone[0], got[1, 2])
    f = make(FMTS["f32"], (2, 3, 37, 53, 1), seed=6)
    gf = ops.resize(dev(f), (16, 16))
    assert np.array_equal(bits(host(gf)), bits(expect(f, (16, 16), FMTS["f32"])))
    assert np.array_equal(bits(host(ops.resize(dev(f)[0, 1][None], (16, 16))[0])), bits(host(gf[0, 1])))


def test_views_go_to_the_kernel_as_they_are():
    """channel-first storage, transposed axes, a window of a larger tensor at a non-zero offset, a stride-0 channel and a frame
    stride larger than a frame: each equals the evaluator on the view's values, and nothing is made contiguous"""
    size = (19, 33)
    seen = []

    def check(view, fmt=FMTS["u8"], sample_format=None):
        assert not view.is_contiguous()
        got = ops.resize(view, size, sample_format=sample_format)
        assert np.array_equal(bits(host(got)), bits(expect(host(view), size, fmt)))
        seen.append(view)

    cf = dev(make(FMTS["u8"], (2, 3, 45, 70), seed=1))       # [n, C, H, W]
    check(cf.permute(0, 2, 3, 1))
    tr = dev(make(FMTS["u8"], (2, 70, 45, 3), seed=2))       # [n, W, H, C]
    check(tr.transpose(1, 2))
    big = dev(make(FMTS["u16_10"], (2, 60, 90, 3), seed=3))
    win = big[:, 9:54, 11:81]
    assert win.storage_offset() > 0
    check(win, FMTS["u16_10"], SampleFormat.u16(10))
    win1 = big[1:, 9:54, 11:81]                              # (the offset carries a whole signal as well)
    check(win1, FMTS["u16_10"], SampleFormat.u16(10))
    grey = dev(make(FMTS["f32"], (2, 45, 70, 1), seed=4)).expand(2, 45, 70, 3)
    assert grey.stride(-1) == 0
    check(grey, FMTS["f32"])
    clips = dev(make(FMTS["u8"], (2, 6, 45, 70, 3), seed=5))
    check(clips[:, 1::2])                                    # frames 1, 3, 5: a frame stride of two frames
    assert clips[:, 1::2].stride(1) == 2 * 45 * 70 * 3
    check(clips[:, :3].transpose(2, 3))                      # clips of 70 x 45 through transposed strides
    assert len(seen) == 7


def test_no_signals():
    t = torch.empty(0, 45, 70, 3, dtype=torch.uint8, device=DEV)
    out = ops.resize(t, (19, 33))
    assert tuple(out.shape) == (0, 19, 33, 3)
    rc, _, untouched = raw(dev(make(FMTS["u8"], (1, 45, 70, 3))), (19, 33), FMTS["u8"], n=0, null=("src", "dst", "table"))
    assert rc == 0 and untouched


def test_wrapper_checks():
    u8 = dev(make(FMTS["u8"], (1, 20, 20, 3)))
    with pytest.raises(ValueError, match="sample_format"):
        ops.resize(u8.to(torch.int16), (8, 8))
    with pytest.raises(_lib.RcbError, match="GPU"):
        ops.resize(u8.cpu(), (8, 8))
    with pytest.raises(_lib.RcbError, match="must be"):
        ops.resize(u8[0], (8, 8))
    with pytest.raises(_lib.RcbError, match="output of shape"):
        ops.resize(u8, (8, 8), out=torch.empty(1, 8, 8, 3, device=DEV))
    with pytest.raises(_lib.RcbError, match="kind 3"):
        ops.resize(u8.to(torch.int16), (8, 8), sample_format=SampleFormat.s16())
    with pytest.raises(_lib.RcbError, match="16 : 1"):
        ops.resize(dev(make(FMTS["u8"], (1, 20, 33, 3))), (8, 2))
    with pytest.raises(_lib.RcbError, match="reads"):
        ops.resize(u8, (8, 8), sample_format=SampleFormat.u16(10))


def test_refusals_launch_nothing():
    """every refusal of the header: its code, and dst keeps its sentinel"""
    src = make(FMTS["u8"], (2, 3, 20, 24, 3), seed=9)
    t = dev(src)
    u8, size = FMTS["u8"], (9, 10)
    rc, got, _ = raw(t, size, u8)
    assert rc == 0 and np.array_equal(got, expect(src, size, u8))
    st = [int(v) for v in t.stride()]
    need_elems = t.numel()
    cases = [
        (dict(kind=3), ERR_ARG), (dict(kind=4), ERR_ARG), (dict(kind=-1), ERR_ARG),
        (dict(depth=8), ERR_ARG), (dict(kind=2, depth=8), ERR_ARG), (dict(kind=2, depth=17), ERR_ARG), (dict(kind=2, depth=0), ERR_ARG),
        (dict(kind=1, depth=10), ERR_ARG),
        (dict(C=0), ERR_SHAPE), (dict(C=33), ERR_SHAPE),
        (dict(H=0), ERR_SHAPE), (dict(W=0), ERR_SHAPE), (dict(Ho=0), ERR_SHAPE), (dict(Wo=-1), ERR_SHAPE), (dict(T=0), ERR_SHAPE),
        (dict(n=-1), ERR_SHAPE),
        (dict(Ho=1), ERR_UNSUPPORTED), (dict(Wo=1), ERR_UNSUPPORTED),                # 20 : 1 and 24 : 1
        (dict(strides=[st[0], st[1], -st[2], st[3], st[4]]), ERR_ARG), (dict(strides=[-1] + st[1:]), ERR_ARG),
        (dict(offset=-1), ERR_ARG),
        (dict(src_elems=need_elems - 1), ERR_SHAPE), (dict(offset=1), ERR_SHAPE), (dict(n=3), ERR_SHAPE), (dict(W=25), ERR_SHAPE),
        (dict(strides=[st[0], st[1], 1 << 62, st[3], st[4]]), ERR_SHAPE),
        (dict(null=("src",)), ERR_ARG), (dict(null=("dst",)), ERR_ARG), (dict(null=("strides",)), ERR_ARG),
        (dict(null=("table",)), ERR_ARG),
        (dict(table_delta=-1), ERR_SHAPE), (dict(table_shift=4), ERR_SHAPE),
        (dict(n=1 << 31, strides=[0, 0] + st[2:]), ERR_UNSUPPORTED),                 # two tiles per frame, 2^31 * 3 frames
    ]
    for over, code in cases:
        rc, _, untouched = raw(t, size, u8, **over)
        assert rc == code and untouched, (over, rc)
        assert _lib.load().rcb_last_error_string()
    # ... and the limits themselves pass
    rc, got, _ = raw(t, (2, 10), u8)                         # 10 : 1
    assert rc == 0 and np.array_equal(got, expect(src, (2, 10), u8))
    rc, got, _ = raw(t, size, u8, src_elems=need_elems)
    assert rc == 0
