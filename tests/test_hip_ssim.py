"""rcb_ssim (N4 414) against the numpy evaluator of its definition (tests/ssim_emul.py): every comparison is bit for bit -- the
{ssim, cs} map through an int64 view, the fixed-point sums as integers.

The kernel works on tiles of T x T = 16 x 16 window positions (csrc/ssim.hip: kT), so H - 10 and W - 10 run over
{1, T - 1, T, T + 1, 2 T + 1}: one partial tile, a tile less one, a full tile, a tile and a sliver, three tiles."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ssim_emul as E

pytestmark = pytest.mark.gpu

from recombiner_amd import _lib, ops, utils  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

DEV = "cuda"
T = 16
EXTENTS = [1 + 10, T - 1 + 10, T + 10, T + 1 + 10, 2 * T + 1 + 10]
FMTS = {"u8": (0, 0), "u16_9": (2, 9), "u16_12": (2, 12), "u16_16": (2, 16)}
INPUTS = ["noise", "smooth", "complement", "zeros", "full"]
SENT_I, SENT_F, SENT_B = -0x0123456789ABCDEF, -7.25, 0x5A
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -3


def _np_dtype(fmt):
    return np.uint8 if fmt[0] == 0 else np.uint16


def make(kind, fmt, shape, seed=0):
    """integer operands (a, b) [n, H, W, C] in the format's numpy dtype"""
    L = E.level_max(*fmt)
    rng = np.random.default_rng(seed)
    n, H, W, Cc = shape
    if kind == "noise":
        a, b = rng.integers(0, L + 1, shape), rng.integers(0, L + 1, shape)
        if fmt[0] == 2 and fmt[1] < 16:                      # stored values above M = 2^depth - 1: used as they are
            a.reshape(-1)[::5] = 65535
            b.reshape(-1)[::7] = L + 1
    elif kind == "smooth":
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        base = np.rint(L * (0.5 + 0.4 * np.sin(yy / 7.0) * np.cos(xx / 5.0))).astype(np.int64)
        a = np.broadcast_to(base[None, :, :, None], shape) + rng.integers(0, 2, shape)
        b = np.clip(a + rng.integers(-3, 4, shape), 0, L)
    elif kind == "complement":
        a = rng.integers(0, 2, shape) * L
        b = L - a
    elif kind == "zeros":
        a, b = np.zeros(shape, dtype=np.int64), rng.integers(0, 2, shape)
    elif kind == "full":
        a, b = np.full(shape, L), np.full(shape, L) - rng.integers(0, 2, shape)
    else:
        raise ValueError(kind)
    return a.astype(_np_dtype(fmt)), b.astype(_np_dtype(fmt))


def dev(a):
    """numpy uint8 / uint16 -> a device tensor of the same bits (uint16 through its int16 view)"""
    if a.dtype == np.uint16:
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV).view(torch.uint16)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(n, dtype, sentinel, pad=16):
    """n elements inside a larger buffer of sentinels -> (the whole buffer, the inner view, check() that the rim is untouched)"""
    big = torch.full((n + 2 * pad,), sentinel, device=DEV, dtype=dtype)

    def check():
        assert bool((big[:pad] == sentinel).all().item()) and bool((big[pad + n:] == sentinel).all().item())
    return big, big[pad:pad + n], check


def _vp(x):
    if x is None:
        return None
    return C.c_void_p(x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())


def raw(a, b, fmt, scales=1, want_map=True, **over):
    """rcb_ssim on device tensors a, b [n, H, W, C] with guarded outputs and workspace -> (rc, sums or None, map or None,
    untouched: whether sums and map still hold their sentinels).  `over` replaces single arguments (the refusals)."""
    lib = _lib.load()
    n, H, W, Cc = (int(v) for v in a.shape)
    kind, depth = fmt
    g = dict(kind=kind, depth=depth, n=n, H=H, W=W, C=Cc, scales=scales, st_a=[int(v) for v in a.stride()],
             st_b=[int(v) for v in b.stride()], null=(), ws_delta=0, ws_shift=0)
    g.update(over)
    L = E.level_max(kind if kind in (0, 2) else 0, depth if 9 <= depth <= 16 else 9)
    c1, c2 = E.constants(L)
    win = np.ascontiguousarray(utils.ssim_window())
    n_sums = max(n, 1) * max(min(g["scales"], 5), 1) * Cc * 2
    n_map = max(n, 1) * (H - 10) * (W - 10) * Cc * 2 if want_map else 0
    _, sums, check_s = _guarded(n_sums, torch.int64, SENT_I)
    _, smap, check_m = _guarded(max(n_map, 1), torch.float64, SENT_F)
    need = int(lib.rcb_ssim_workspace_bytes(n, H, W, Cc, scales))
    ws_big, ws, check_w = _guarded(max(need, 16), torch.uint8, SENT_B, pad=64)
    assert ws.data_ptr() % 16 == 0
    st_a, st_b = (C.c_int64 * 4)(*g["st_a"]), (C.c_int64 * 4)(*g["st_b"])
    rc = lib.rcb_ssim(None if "a" in g["null"] else _vp(a), None if "b" in g["null"] else _vp(b), g["kind"], g["depth"], g["n"],
                      g["H"], g["W"], g["C"], None if "st_a" in g["null"] else st_a, None if "st_b" in g["null"] else st_b,
                      None if "win" in g["null"] else _vp(win), c1, c2, g["scales"], None if "sums" in g["null"] else _vp(sums),
                      _vp(smap) if want_map else None,
                      None if "ws" in g["null"] else C.c_void_p(ws.data_ptr() + g["ws_shift"]), max(need, 0) + g["ws_delta"],
                      ops.stream_ptr())
    torch.cuda.synchronize()
    check_s(), check_m(), check_w()
    untouched = bool((sums == SENT_I).all().item()) and bool((smap == SENT_F).all().item())
    if rc != 0 or n == 0:
        return rc, None, None, untouched
    out_s = sums.view(n, scales, Cc, 2).cpu().numpy()
    out_m = smap.view(n, H - 10, W - 10, Cc, 2).cpu().numpy() if want_map else None
    return rc, out_s, out_m, untouched


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(want).view(np.int64))


def expect(a, b, fmt, scales=1):
    L = E.level_max(*fmt)
    return E.batch_sums(a.astype(np.int64), b.astype(np.int64), L, scales), E.batch_map(a.astype(np.int64), b.astype(np.int64), L)


# ---- shapes, channels, batch sizes, formats and inputs ----------------------------------------------------------------------------
@pytest.mark.parametrize("W", EXTENTS)
@pytest.mark.parametrize("H", EXTENTS)
def test_tile_edges(H, W):
    """every (H - 10, W - 10) of the tile grid; per shape C = 1, 3, 4, with n, the format and the input family rotating so that
    all of them meet every extent of each axis"""
    i = EXTENTS.index(H) * len(EXTENTS) + EXTENTS.index(W)
    for j, Cc in enumerate((1, 3, 4)):
        n = (1, 3)[(i + j) % 2]
        name = list(FMTS)[(i + j) % len(FMTS)]
        kind = INPUTS[(i // 2 + j) % len(INPUTS)]
        a, b = make(kind, FMTS[name], (n, H, W, Cc), seed=i * 3 + j)
        rc, sums, smap, _ = raw(dev(a), dev(b), FMTS[name])
        want_s, want_m = expect(a, b, FMTS[name])
        assert rc == 0 and same_bits(smap, want_m), (Cc, n, name, kind)
        assert np.array_equal(sums, want_s), (Cc, n, name, kind)


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("name", list(FMTS))
def test_formats_and_inputs(name, kind):
    """every format with every input family at one shape of three tiles by two, C = 3, n = 3 -- the complement family has
    negative cs, the 9- and 12-bit noise stored values above 2^depth - 1"""
    a, b = make(kind, FMTS[name], (3, 2 * T + 1 + 10, T + 1 + 10, 3), seed=len(name) + len(kind))
    rc, sums, smap, _ = raw(dev(a), dev(b), FMTS[name])
    want_s, want_m = expect(a, b, FMTS[name])
    assert rc == 0 and same_bits(smap, want_m) and np.array_equal(sums, want_s)
    if kind == "complement":
        assert (smap[..., 1] < 0).any() and (sums[..., 1] < 0).all()


@pytest.mark.parametrize("name", list(FMTS))
def test_identical_operands_are_exactly_one(name):
    a, _ = make("noise", FMTS[name], (2, 43, 27, 3), seed=2)
    t = dev(a)
    rc, sums, smap, _ = raw(t, t.clone(), FMTS[name])
    assert rc == 0 and np.all(smap == 1.0)
    assert np.all(sums == 33 * 17 * E.FX)


# ---- strides -----------------------------------------------------------------------------------------------------------------------
def test_strided_operands_give_the_bits_of_their_contiguous_copies():
    fmt = FMTS["u8"]
    n, H, W, Cc = 2, 27, 43, 3
    a, b = make("smooth", fmt, (n, H, W, Cc), seed=9)
    _, base_s, base_m, _ = raw(dev(a), dev(b), fmt)
    ta, tb = dev(a), dev(b)
    big = torch.zeros(n, H + 5, W + 7, Cc, device=DEV, dtype=torch.uint8)
    big[:, 2:2 + H, 3:3 + W] = ta
    views = {
        "channel_first": (ta.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), tb),
        "transposed": (ta, tb.transpose(1, 2).contiguous().transpose(1, 2)),
        "window": (big[:, 2:2 + H, 3:3 + W], tb.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)),
    }
    for name, (va, vb) in views.items():
        assert not (va.is_contiguous() and vb.is_contiguous()), name
        rc, sums, smap, _ = raw(va, vb, fmt)
        assert rc == 0 and same_bits(smap, base_m) and np.array_equal(sums, base_s), name
    # a broadcast channel (stride 0) against three real ones
    g = ta[..., :1].contiguous()
    rc, sums, smap, _ = raw(g.expand(n, H, W, Cc), tb, fmt)
    assert g.expand(n, H, W, Cc).stride(3) == 0
    _, want_s, want_m, _ = raw(g.expand(n, H, W, Cc).contiguous(), tb, fmt)
    assert rc == 0 and same_bits(smap, want_m) and np.array_equal(sums, want_s)
    assert np.array_equal(sums, E.batch_sums(np.repeat(a[..., :1], Cc, -1).astype(np.int64), b.astype(np.int64), 255))
    # through the wrapper: the same strides, the same bits
    s2, m2 = ops.ssim_sums(views["window"][0], views["window"][1], want_map=True)
    assert np.array_equal(s2.cpu().numpy(), base_s) and same_bits(m2.cpu().numpy(), base_m)


def test_offsets_past_2_31_elements():
    """two small images placed by an image stride above 2^31 elements: the second one's offsets need 64 bits"""
    fmt = FMTS["u8"]
    n, H, W, Cc = 2, 12, 27, 1
    a, b = make("noise", fmt, (n, H, W, Cc), seed=4)
    stride = 2 ** 31 + 64
    store = torch.empty(stride + H * W * Cc, device=DEV, dtype=torch.uint8)
    va = store.as_strided((n, H, W, Cc), (stride, W * Cc, Cc, 1))
    va.copy_(dev(a))
    rc, sums, smap, _ = raw(va, dev(b), fmt)
    want_s, want_m = expect(a, b, fmt)
    assert rc == 0 and same_bits(smap, want_m) and np.array_equal(sums, want_s)
    assert not np.array_equal(sums[0], sums[1])


# ---- five scales ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _five_scale_case(name, H, W, Cc):
    a, b = make("smooth", FMTS[name], (1, H, W, Cc), seed=H + W)
    L = E.level_max(*FMTS[name])
    sums = E.sums(a[0].astype(np.int64), b[0].astype(np.int64), L, 5)
    return a, b, sums, E.ssim_figure(sums, H, W), E.msssim_figure(sums, H, W)


@pytest.mark.parametrize("name,H,W,Cc", [("u8", 176, 176, 1), ("u8", 177, 191, 3), ("u16_12", 176, 180, 2)])
def test_five_scales(name, H, W, Cc):
    a, b, want, want_ssim, want_ms = _five_scale_case(name, H, W, Cc)
    rc, sums, _, _ = raw(dev(a), dev(b), FMTS[name], scales=5, want_map=False)
    assert rc == 0
    for s in range(5):
        assert sums[0, s].tolist() == want[s], s
    assert utils.msssim_from_sums(sums, H, W).tolist() == [want_ms] and utils.ssim_from_sums(sums, H, W).tolist() == [want_ssim]
    assert 0.0 < want_ms < 1.0
    # the figures through the package's own path
    fmt = SampleFormat(*FMTS[name])
    assert utils.ssim_device(dev(a), dev(b), sample_format=fmt, multiscale=True).tolist() == [want_ms]
    assert utils.ssim_device([dev(a)[0]], [dev(b)[0]], sample_format=fmt).tolist() == [want_ssim]
    # fewer scales: the leading ones, unchanged
    rc, two, _, _ = raw(dev(a), dev(b), FMTS[name], scales=2, want_map=False)
    assert rc == 0 and np.array_equal(two, sums[:, :2])


# ---- an image alone, in a batch, in a permuted batch, twice ------------------------------------------------------------------------
def test_sums_do_not_depend_on_the_batch_or_the_run():
    fmt = FMTS["u8"]
    a, b = make("smooth", fmt, (4, 47, 59, 3), seed=12)
    ta, tb = dev(a), dev(b)
    _, whole, whole_m, _ = raw(ta, tb, fmt, scales=3)
    _, again, again_m, _ = raw(ta, tb, fmt, scales=3)
    assert np.array_equal(whole, again) and same_bits(whole_m, again_m)
    perm = [2, 0, 3, 1]
    _, shuffled, shuffled_m, _ = raw(ta[perm].contiguous(), tb[perm].contiguous(), fmt, scales=3)
    assert np.array_equal(shuffled, whole[perm]) and same_bits(shuffled_m, whole_m[perm])
    for k in range(4):
        _, alone, alone_m, _ = raw(ta[k:k + 1], tb[k:k + 1], fmt, scales=3)
        assert np.array_equal(alone[0], whole[k]) and same_bits(alone_m[0], whole_m[k]), k
    assert np.array_equal(whole, E.batch_sums(a.astype(np.int64), b.astype(np.int64), 255, 3))


# ---- the wrapper's checks --------------------------------------------------------------------------------------------------------
def test_wrapper_checks():
    a, b = make("noise", FMTS["u16_12"], (1, 22, 22, 1))
    ta, tb = dev(a), dev(b)
    with pytest.raises(ValueError, match="sample_format"):
        ops.ssim_sums(ta, tb)
    with pytest.raises(ValueError, match="sample_format"):
        ops.ssim_sums(ta.view(torch.int16), tb.view(torch.int16))
    with pytest.raises(_lib.RcbError):
        ops.ssim_sums(ta, tb, sample_format=SampleFormat.u8())
    with pytest.raises(_lib.RcbError):
        ops.ssim_sums(ta.float(), tb.float())
    with pytest.raises(_lib.RcbError):
        ops.ssim_sums(ta, tb[:, :21], sample_format=SampleFormat.u16(12))
    with pytest.raises(_lib.RcbError, match="scales"):
        ops.ssim_sums(ta, tb, sample_format=SampleFormat.u16(12), scales=3)
    with pytest.raises(ValueError, match="too small"):
        utils.ssim_device(ta, tb, sample_format=SampleFormat.u16(12), multiscale=True)
    # an int16 tensor holds the same bits as the uint16 one
    s1, _ = ops.ssim_sums(ta, tb, sample_format=SampleFormat.u16(12), scales=2)
    s2, m2 = ops.ssim_sums(ta.view(torch.int16), tb, sample_format=SampleFormat.u16(12), scales=2, want_map=True)
    assert torch.equal(s1, s2) and s1.dtype == torch.int64 and tuple(m2.shape) == (1, 12, 12, 1, 2) and m2.dtype == torch.float64
    assert np.array_equal(s1.cpu().numpy(), E.batch_sums(a.astype(np.int64), b.astype(np.int64), 4095, 2))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib = _lib.load()
    fmt = FMTS["u8"]
    a, b = make("noise", fmt, (2, 43, 45, 3), seed=1)
    ta, tb = dev(a), dev(b)
    rc, sums, _, untouched = raw(ta, tb, fmt, scales=2)
    assert rc == 0 and not untouched                          # the call the refusals below are one step away from
    a16, b16 = make("noise", FMTS["u16_12"], (2, 43, 45, 3), seed=1)
    bad = [(dict(kind=1), ERR_ARG), (dict(kind=3), ERR_ARG), (dict(kind=4), ERR_ARG), (dict(depth=8), ERR_ARG),
           (dict(kind=2, depth=8), ERR_ARG), (dict(kind=2, depth=17), ERR_ARG), (dict(kind=2, depth=0), ERR_ARG),
           (dict(C=0), ERR_SHAPE), (dict(C=33), ERR_SHAPE), (dict(H=10), ERR_SHAPE), (dict(W=10), ERR_SHAPE),
           (dict(scales=0), ERR_ARG), (dict(scales=6), ERR_ARG), (dict(scales=3), ERR_SHAPE), (dict(H=8203, W=8202), ERR_UNSUPPORTED),
           (dict(st_a=[43 * 45 * 3, -135, 3, 1]), ERR_ARG), (dict(st_b=[43 * 45 * 3, 135, 3, -1]), ERR_ARG), (dict(n=-1), ERR_SHAPE),
           (dict(null=("a",)), ERR_ARG), (dict(null=("b",)), ERR_ARG), (dict(null=("sums",)), ERR_ARG), (dict(null=("win",)), ERR_ARG),
           (dict(null=("st_a",)), ERR_ARG), (dict(null=("ws",)), ERR_SHAPE), (dict(ws_delta=-1), ERR_SHAPE),
           (dict(ws_shift=8), ERR_SHAPE)]
    for kw, code in bad:
        rc, _, _, untouched = raw(ta, tb, fmt, **{"scales": 2, **kw})
        assert rc == code and untouched, (kw, rc)
        assert lib.rcb_last_error_string()
    rc, _, _, untouched = raw(dev(a16), dev(b16), FMTS["u16_12"], scales=2, depth=0)
    assert rc == ERR_ARG and untouched
    # no images: succeeds and launches nothing
    rc, _, _, untouched = raw(ta[:0], tb[:0], fmt, scales=2, null=("a", "b", "sums", "ws"))
    assert rc == 0 and untouched
    # 2^26 positions are accepted, one more row of them is not; a refused shape has no workspace size
    assert lib.rcb_ssim_workspace_bytes(1, 8202, 8202, 1, 1) == 0 and lib.rcb_ssim_workspace_bytes(1, 8203, 8202, 1, 1) == -1
    assert lib.rcb_ssim_workspace_bytes(2, 43, 45, 3, 2) > 0 and lib.rcb_ssim_workspace_bytes(2, 43, 45, 3, 2) % 16 == 0
    assert lib.rcb_ssim_workspace_bytes(2, 43, 45, 3, 3) == -1 and lib.rcb_ssim_workspace_bytes(2, 43, 45, 33, 1) == -1
    assert lib.rcb_ssim_workspace_bytes(1, 175, 300, 1, 5) == -1 and lib.rcb_ssim_workspace_bytes(1, 176, 176, 1, 5) > 0
