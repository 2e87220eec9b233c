"""rcb_ycc_to_rgb, rcb_rgb_to_ycc and rcb_ycc_sse (N4 418) against the numpy evaluator of their definition (tests/ycc_emul.py):
every comparison is bit for bit, integers as integers.

A thread of the kernels owns 2 x 4 positions and a workgroup 16 x 128 (csrc/colour.hip: kTH, kTW, kWY, kWX).  The shapes are the
smallest at which they can still go wrong: one position, one row, one whole chroma block, odd sizes on both axes (the clipped far
row and column), 8 x 32 +- 1 (a partial thread tile, which leaves the dword path), 17 x 65 and 17 x 129 (a second workgroup on
each axis, by one position).  The 8-bit cube holds every RGB triple: tests/test_ycc_emul_cpu.py counts the values a contracted
evaluation changes there, so it is the guard of the no-contraction rule."""
import ctypes as C

import numpy as np
import pytest
import torch

import ycc_emul as E

pytestmark = pytest.mark.gpu

from recombiner_amd import _lib, ops, utils  # noqa: E402
from recombiner_amd._lib import RcbError  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

DEV = "cuda"
SIZES = [(1, 1), (1, 7), (2, 2), (5, 7), (8, 31), (8, 32), (8, 33), (17, 65), (17, 129)]
FMTS = {"u8": (0, 0), "u16_10": (2, 10), "u16_16": (2, 16)}
MATRICES = [("bt601", True), ("bt709", False), ("bt2020", True), ("bt601", False), ("bt709", True), ("bt2020", False)]
NP_DTYPE = {0: np.uint8, 2: np.uint16}
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -3
SENT = 0x5A


def sample_format(fmt):
    return SampleFormat.u8() if fmt[0] == 0 else SampleFormat.u16(fmt[1])


def matrix(k, fmt):
    standard, full = MATRICES[k % len(MATRICES)]
    return utils.ycc_matrix(standard, full, sample_format(fmt))


def make(fmt, shape, seed=0):
    """integers of `shape` in the format's numpy dtype: random, with the extremes and, below 16 bits, stored values above L"""
    L = E.peak(*fmt)
    a = np.random.default_rng(seed).integers(0, L + 1, shape)
    flat = a.reshape(-1)
    flat[::7] = L
    flat[3::11] = 0
    if fmt[0] == 2 and fmt[1] < 16:
        flat[5::13] = 65535
    return a.astype(NP_DTYPE[fmt[0]])


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def host(t):
    t = t.contiguous()
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _guarded(n_bytes, pad=64, shift=0):
    """n_bytes of device memory with sentinel bytes on both sides (shift: the first byte's address modulo 4)"""
    big = torch.full((n_bytes + 2 * pad + 4,), SENT, device=DEV, dtype=torch.uint8)
    lo = pad + shift

    def check():
        assert bool((big[:lo] == SENT).all().item()) and bool((big[lo + n_bytes:] == SENT).all().item())
    return big[lo:lo + n_bytes], check


def _out(shape, np_dtype, shift=0):
    item = np.dtype(np_dtype).itemsize
    buf, check = _guarded(max(int(np.prod(shape)) * item, 1), shift=shift * item)

    def read():
        check()
        return buf.cpu().numpy()[:int(np.prod(shape)) * item].view(np_dtype).reshape(shape)
    return buf, read


def _alloc_shape(n, T, h, w):
    """the shape of an output, or one element where the entry must refuse (or would need more than a test allocates)"""
    fits = 0 <= n <= 64 and 1 <= T <= 64 and h >= 1 and w >= 1 and h * w <= 1 << 20
    return (n, T, h, w) if fits else (1,)


def _f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    return a, C.c_void_p(a.ctypes.data)


def _rgb_args(t):
    """(storage pointer, elements, strides[5], offset, (n, T, H, W)) of an RGB tensor [n, H, W, 3] or [n, T, H, W, 3], any strides"""
    clip = t.dim() == 5
    st = [int(v) for v in t.stride()]
    store = t.untyped_storage()
    return dict(ptr=store.data_ptr(), elems=store.nbytes() // t.element_size(), strides=[st[0], st[1] if clip else 0] + st[-3:],
                offset=int(t.storage_offset()), n=int(t.shape[0]), T=int(t.shape[1]) if clip else 1, H=int(t.shape[-3]),
                W=int(t.shape[-2]))


def raw_forward(t, mx, ss, fmt, want=(True, True, True), shift=0, **over):
    """rcb_rgb_to_ycc with guard bytes round every output -> (rc, [y, cb, cr] as numpy, None where not wanted)"""
    lib = _lib.load()
    g = dict(_rgb_args(t), kind=fmt[0], depth=fmt[1], ss=ss, null=())
    g.update(over)
    Hc, Wc = E.chroma_size(g["H"], g["W"], ss)
    shapes = [_alloc_shape(g["n"], g["T"], g["H"], g["W"]), _alloc_shape(g["n"], g["T"], Hc, Wc), _alloc_shape(g["n"], g["T"], Hc, Wc)]
    outs = [_out(s, NP_DTYPE[fmt[0]], shift) if w else None for s, w in zip(shapes, want)]
    (_m, m_ptr), (_o, o_ptr) = _f64(mx.m), _f64(mx.off)
    rc = lib.rcb_rgb_to_ycc(None if "src" in g["null"] else C.c_void_p(g["ptr"]), g["elems"],
                            None if "strides" in g["null"] else (C.c_int64 * 5)(*g["strides"]), g["offset"], g["kind"], g["depth"],
                            g["ss"], g["n"], g["T"], g["H"], g["W"], None if "m" in g["null"] else m_ptr,
                            None if "off" in g["null"] else o_ptr,
                            *(C.c_void_p(o[0].data_ptr()) if o else None for o in outs), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, [o[1]() if o else None for o in outs]


def _plane_args(p, clip):
    st = [int(v) for v in p.stride()]
    store = p.untyped_storage()
    return (p.data_ptr(), (store.data_ptr() + store.nbytes() - p.data_ptr()) // p.element_size(),
            [st[0], st[1] if clip else 0, st[-2], st[-1]])


def raw_inverse(y, cb, cr, mx, ss, fmt, shift=0, **over):
    """rcb_ycc_to_rgb on three plane tensors [n, (T,) rows, columns] of any strides -> (rc, rgb as numpy)"""
    lib = _lib.load()
    clip = y.dim() == 4
    planes = [_plane_args(p, clip) for p in (y, cb, cr)]
    g = dict(kind=fmt[0], depth=fmt[1], ss=ss, n=int(y.shape[0]), T=int(y.shape[1]) if clip else 1, H=int(y.shape[-2]), W=int(y.shape[-1]),
             elems=[p[1] for p in planes], strides=[p[2] for p in planes], null=())
    g.update(over)
    shape = (int(y.shape[0]), int(y.shape[1]) if clip else 1, int(y.shape[-2]), int(y.shape[-1]), 3)
    dst, read = _out(shape, NP_DTYPE[fmt[0]], shift)
    (_n, n_ptr), (_o, o_ptr) = _f64(mx.n), _f64(mx.o)
    ptrs = [None if name in g["null"] else C.c_void_p(p[0]) for name, p in zip(("py", "pcb", "pcr"), planes)]
    sts = [None if "strides%d" % k in g["null"] else (C.c_int64 * 4)(*g["strides"][k]) for k in range(3)]
    rc = lib.rcb_ycc_to_rgb(*ptrs, None if "elems" in g["null"] else (C.c_int64 * 3)(*g["elems"]), *sts, g["kind"], g["depth"], g["ss"],
                            g["n"], g["T"], g["H"], g["W"], None if "inv" in g["null"] else n_ptr, None if "o" in g["null"] else o_ptr,
                            None if "dst" in g["null"] else C.c_void_p(dst.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = read()
    return rc, out if clip else out[:, 0]


def raw_sse(a, b, mx, ss, fmt, **over):
    """rcb_ycc_sse with guard bytes round the sums -> (rc, int64 [n, T, 3])"""
    lib = _lib.load()
    ga, gb = _rgb_args(a), _rgb_args(b)
    g = dict(kind=fmt[0], depth=fmt[1], ss=ss, n=ga["n"], T=ga["T"], H=ga["H"], W=ga["W"], null=(), a_strides=ga["strides"],
             b_strides=gb["strides"], a_offset=ga["offset"], b_offset=gb["offset"], a_elems=ga["elems"], b_elems=gb["elems"])
    g.update(over)
    sums, read = _out((ga["n"], ga["T"], 3), np.int64)
    assert sums.data_ptr() % 8 == 0
    (_m, m_ptr), (_o, o_ptr) = _f64(mx.m), _f64(mx.off)
    rc = lib.rcb_ycc_sse(None if "a" in g["null"] else C.c_void_p(ga["ptr"]), g["a_elems"],
                         None if "a_strides" in g["null"] else (C.c_int64 * 5)(*g["a_strides"]), g["a_offset"],
                         None if "b" in g["null"] else C.c_void_p(gb["ptr"]), g["b_elems"],
                         None if "b_strides" in g["null"] else (C.c_int64 * 5)(*g["b_strides"]), g["b_offset"], g["kind"], g["depth"],
                         g["ss"], g["n"], g["T"], g["H"], g["W"], None if "m" in g["null"] else m_ptr, None if "off" in g["null"] else o_ptr,
                         None if "sse" in g["null"] else C.c_void_p(sums.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, read()


def last_error():
    return _lib.load().rcb_last_error_string().decode(errors="replace")


def expect_forward(src, mx, ss, fmt):
    return E.rgb_to_ycc(src.astype(np.int64), mx.m, mx.off, E.peak(*fmt), ss)


def sse_as_ints(sse):
    return [[[int(v) for v in f] for f in s] for s in sse]


# ---- the three entries over sizes, subsamplings, formats, ranges and standards ---------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_every_entry_matches_the_evaluator(size):
    H, W = size
    k = 0
    for name, fmt in FMTS.items():
        for ss in (0, 1, 2):
            for n, T in ((1, 1), (3, 3)) if size in ((5, 7), (8, 33), (17, 129)) else ((3, 1),):
                mx = matrix(k, fmt)
                k += 1
                L = E.peak(*fmt)
                a, b = make(fmt, (n, T, H, W, 3), seed=k), make(fmt, (n, T, H, W, 3), seed=100 + k)
                want = expect_forward(a, mx, ss, fmt)
                rc, got = raw_forward(dev(a), mx, ss, fmt)
                assert rc == 0, last_error()
                for g_, w_, plane in zip(got, want, "Y Cb Cr".split()):
                    assert g_.shape == w_.shape and np.array_equal(g_.astype(np.int64), w_), (name, ss, n, T, plane)
                if fmt[0] == 0:                              # (the luma plane off the 4-byte boundary: no dword stores, the same bits)
                    rc, moved = raw_forward(dev(a), mx, ss, fmt, shift=1)
                    assert rc == 0 and all(np.array_equal(g_, m_) for g_, m_ in zip(got, moved)), (name, ss)
                # the inverse, on planes that are NOT a forward's output: every combination of samples may meet
                Hc, Wc = E.chroma_size(H, W, ss)
                y, cb, cr = make(fmt, (n, T, H, W), seed=k), make(fmt, (n, T, Hc, Wc), seed=k + 1), make(fmt, (n, T, Hc, Wc), seed=k + 2)
                rc, rgb = raw_inverse(dev(y), dev(cb), dev(cr), mx, ss, fmt)
                assert rc == 0, last_error()
                assert np.array_equal(rgb.astype(np.int64), E.ycc_to_rgb(y.astype(np.int64), cb.astype(np.int64), cr.astype(np.int64),
                                                                       mx.n, mx.o, L, ss)), (name, ss, n, T)
                # the sums: the evaluator's Python integers, which are the sums over rgb_to_ycc's own outputs
                rc, sse = raw_sse(dev(a), dev(b), mx, ss, fmt)
                assert rc == 0, last_error()
                assert sse_as_ints(sse) == sse_as_ints(E.ycc_sse(a.astype(np.int64), b.astype(np.int64), mx.m, mx.off, L, ss)), (name, ss)
                _, other = raw_forward(dev(b), mx, ss, fmt)
                own = [[[int(((got[p][i, t].astype(np.int64) - other[p][i, t].astype(np.int64)) ** 2).sum()) for p in range(3)]
                        for t in range(T)] for i in range(n)]
                assert sse_as_ints(sse) == own


# ---- the 8-bit cube: every RGB triple (and every Y'CbCr triple) once ---------------------------------------------------------------
@pytest.fixture(scope="module")
def cube():
    v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8)


def _by_rows(fn, rows=512):
    return [fn(slice(lo, lo + rows)) for lo in range(0, 4096, rows)]


@pytest.mark.parametrize("standard,full", [("bt601", True), ("bt709", False)])
def test_forward_on_the_whole_cube(cube, standard, full):
    mx = utils.ycc_matrix(standard, full, None)
    y, cb, cr = ops.rgb_to_ycc(dev(cube[None]), mx, 0)
    got = [host(p)[0] for p in (y, cb, cr)]
    want = _by_rows(lambda s: E.rgb_to_ycc(cube[s], mx.m, mx.off, 255, 0))
    for k in range(3):
        assert np.array_equal(got[k], np.concatenate([w[k] for w in want]).astype(np.uint8)), "plane %d" % k


def test_inverse_on_the_whole_cube(cube):
    mx = utils.ycc_matrix("bt601", True, None)
    planes = [dev(np.ascontiguousarray(cube[None, :, :, k])) for k in range(3)]
    got = host(ops.ycc_to_rgb(*planes, mx, 0))[0]
    want = np.concatenate(_by_rows(lambda s: E.ycc_to_rgb(cube[s, :, 0], cube[s, :, 1], cube[s, :, 2], mx.n, mx.o, 255, 0)))
    assert np.array_equal(got, want.astype(np.uint8))


# ---- memory layouts: the dword path and the element-wise path give the same bits ----------------------------------------------------
@pytest.mark.parametrize("ss", [0, 1, 2])
def test_rgb_layouts_share_the_bits(ss):
    fmt = FMTS["u8"]
    mx = matrix(ss, fmt)
    n, T, H, W = 2, 2, 10, 34
    a = make(fmt, (n, T, H, W, 3), seed=7)
    want = expect_forward(a, mx, ss, fmt)
    b = make(fmt, (n, T, H, W, 3), seed=8)
    want_sse = sse_as_ints(E.ycc_sse(a.astype(np.int64), b.astype(np.int64), mx.m, mx.off, 255, ss))
    big = torch.full((n, T, H + 5, 48, 3), 77, device=DEV, dtype=torch.uint8)
    big[:, :, 2:2 + H, 4:4 + W] = dev(a)
    odd = torch.full((n, T, H + 5, 47, 3), 77, device=DEV, dtype=torch.uint8)
    odd[:, :, 2:2 + H, 3:3 + W] = dev(a)
    padded = torch.full((n, T, H, 36, 3), 77, device=DEV, dtype=torch.uint8)
    padded[:, :, :, :W] = dev(a)
    flat = torch.zeros(a.size + 3, device=DEV, dtype=torch.uint8)
    views = {
        "contiguous": dev(a),
        "padded rows (dwords; the last tile of a row is partial)": padded[:, :, :, :W],
        "channel-first": dev(np.ascontiguousarray(np.moveaxis(a, -1, 2))).movedim(2, -1),
        "a window of a larger clip (dwords)": big[:, :, 2:2 + H, 4:4 + W],
        "a window of a larger clip (rows off the 4-byte boundary)": odd[:, :, 2:2 + H, 3:3 + W],
        "transposed": dev(np.ascontiguousarray(np.swapaxes(a, 2, 3))).transpose(2, 3),
        "a misaligned base": flat[1:1 + a.size].copy_(dev(a).reshape(-1)).view(n, T, H, W, 3),
    }
    assert views["a window of a larger clip (dwords)"].data_ptr() % 4 == 0 and views["a misaligned base"].data_ptr() % 4 == 1
    for name, v in views.items():
        assert np.array_equal(host(v), a), name
        for shift in (0, 1):                                 # (shift 1: the luma plane off the 4-byte boundary too)
            rc, got = raw_forward(v, mx, ss, fmt, shift=shift)
            assert rc == 0, last_error()
            assert all(np.array_equal(g_.astype(np.int64), w_) for g_, w_ in zip(got, want)), (name, shift)
        rc, sse = raw_sse(v, dev(b), mx, ss, fmt)
        assert rc == 0 and sse_as_ints(sse) == want_sse, name
        rc, sse = raw_sse(dev(b), v, mx, ss, fmt)
        assert rc == 0 and sse_as_ints(sse) == want_sse, name
    # a broadcast channel: gray through an expanded view
    gray = make(fmt, (n, T, H, W, 1), seed=9)
    rc, got = raw_forward(dev(gray).expand(n, T, H, W, 3), mx, ss, fmt)
    assert rc == 0
    assert all(np.array_equal(g_.astype(np.int64), w_) for g_, w_ in zip(got, expect_forward(np.repeat(gray, 3, axis=-1), mx, ss, fmt)))


@pytest.mark.parametrize("layout", ["i420", "yv12", "nv12", "yuv422p", "yuv444p"])
@pytest.mark.parametrize("name", ["u8", "u16_10"])
def test_raw_frame_layouts_in_one_buffer(layout, name):
    fmt = FMTS[name]
    sf = sample_format(fmt)
    mx = matrix(1, fmt)
    n, T, H, W = 2, 3, 9, 12
    ss = utils.YUV_LAYOUTS[layout]
    Hc, Wc = E.chroma_size(H, W, ss)
    raw = make(fmt, (n * T * (H * W + 2 * Hc * Wc),), seed=11)
    (y, cb, cr), got_ss = utils.yuv_planes(dev(raw), n, T, H, W, layout, sf)
    assert got_ss == ss and cb.data_ptr() != cr.data_ptr()
    want = E.ycc_to_rgb(host(y).astype(np.int64), host(cb).astype(np.int64), host(cr).astype(np.int64), mx.n, mx.o, E.peak(*fmt), ss)
    for shift in (0, 1):                                     # (dst on and off the 4-byte boundary: dword and element stores)
        rc, rgb = raw_inverse(y, cb, cr, mx, ss, fmt, shift=shift)
        assert rc == 0, last_error()
        assert np.array_equal(rgb.astype(np.int64), want), shift
    assert np.array_equal(host(ops.ycc_to_rgb(y, cb, cr, mx, ss, sample_format=sf)).astype(np.int64), want)
    assert np.array_equal(host(utils.ycc_to_rgb_device((y, cb, cr), mx, ss, sample_format=sf)).astype(np.int64), want)
    # a window of the frames: rows 1 .. 8 and columns 4 .. 11 (whole chroma blocks) of every plane
    wy, wcb, wcr = y[..., 2:8, 4:12], cb[..., (2 >> (ss == 2)):(8 >> (ss == 2)), (4 >> (ss > 0)):(12 >> (ss > 0))], \
        cr[..., (2 >> (ss == 2)):(8 >> (ss == 2)), (4 >> (ss > 0)):(12 >> (ss > 0))]
    rc, rgb = raw_inverse(wy, wcb, wcr, mx, ss, fmt)
    assert rc == 0 and np.array_equal(rgb.astype(np.int64), want[:, :, 2:8, 4:12])


def test_bilinear_chroma_is_resize_then_the_444_entry():
    fmt = FMTS["u8"]
    mx = matrix(0, fmt)
    raw = make(fmt, (2 * (10 * 16 + 2 * 5 * 8),), seed=12)
    (y, cb, cr), ss = utils.yuv_planes(dev(raw), 1, 2, 10, 16, "i420")
    got = utils.ycc_to_rgb_device((y, cb, cr), mx, ss, chroma="bilinear")
    up = [host(ops.resize(c.unsqueeze(-1), (10, 16))).astype(np.int64)[..., 0] for c in (cb, cr)]
    assert np.array_equal(host(got).astype(np.int64), E.ycc_to_rgb(host(y).astype(np.int64), up[0], up[1], mx.n, mx.o, 255, 0))
    with pytest.raises(ValueError, match="chroma"):
        utils.ycc_to_rgb_device((y, cb, cr), mx, ss, chroma="nearest")


# ---- the sums ----------------------------------------------------------------------------------------------------------------------
def test_sums_are_zero_for_an_operand_against_itself_and_have_no_order():
    fmt = FMTS["u8"]
    mx = matrix(0, fmt)
    n, T, H, W = 4, 2, 17, 129
    a, b = dev(make(fmt, (n, T, H, W, 3), seed=1)), dev(make(fmt, (n, T, H, W, 3), seed=2))
    assert int(ops.ycc_sse(a, a, mx, 2).abs().sum()) == 0
    whole = ops.ycc_sse(a, b, mx, 2)
    assert whole.dtype == torch.int64 and tuple(whole.shape) == (n, T, 3) and int(whole.min()) > 0
    assert torch.equal(whole, ops.ycc_sse(a, b, mx, 2))                                      # run to run
    perm = [2, 0, 3, 1]
    assert torch.equal(ops.ycc_sse(a[perm], b[perm], mx, 2), whole[perm])                      # batch order
    for i in range(n):
        assert torch.equal(ops.ycc_sse(a[i:i + 1], b[i:i + 1], mx, 2), whole[i:i + 1])         # alone
    assert torch.equal(ops.ycc_sse(a[:, 0], b[:, 0], mx, 2), whole[:, 0])                      # images: the T axis dropped
    psnr = utils.ycc_frames_device(a, b, mx, 2)
    assert psnr.shape == (n, T, 4)
    assert np.array_equal(psnr, utils.psnr_ycc_from_sse(whole.cpu().numpy(), H, W, 2))
    assert np.array_equal(utils.ycc_device(a[:, 1], b[:, 1], mx, 2), psnr[:, 1])


def test_the_extreme_sums_do_not_overflow():
    """16 bits, every term L^2 = 2^32 - 2^17 + 1: a 32-bit partial sum anywhere would wrap at the second term"""
    fmt = FMTS["u16_16"]
    L = 65535
    mx = utils.ycc_matrix("bt601", True, SampleFormat.u16(16))
    H, W = 17, 129
    pairs = {"white / black": ((L, L, L), (0, 0, 0)), "blue / yellow": ((0, 0, L), (L, L, 0)), "red / cyan": ((L, 0, 0), (0, L, L))}
    for ss in (0, 2):
        Hc, Wc = E.chroma_size(H, W, ss)
        for k, (name, (ca, cb_)) in enumerate(pairs.items()):
            a = np.broadcast_to(np.asarray(ca, dtype=np.uint16), (1, 1, H, W, 3))
            b = np.broadcast_to(np.asarray(cb_, dtype=np.uint16), (1, 1, H, W, 3))
            rc, sse = raw_sse(dev(a), dev(b), mx, ss, fmt)
            assert rc == 0, last_error()
            assert sse_as_ints(sse) == sse_as_ints(E.ycc_sse(a.astype(np.int64), b.astype(np.int64), mx.m, mx.off, L, ss)), name
            assert int(sse[0, 0, k]) >= (L - 1) ** 2 * (H * W if k == 0 else Hc * Wc) > 1 << 40, name   # (a tie may round to 1; no 32-bit sum holds it)


def test_one_capture_and_replay_of_the_sums():
    fmt = FMTS["u8"]
    mx = matrix(0, fmt)
    shape = (3, 2, 17, 65, 3)
    a, b = dev(make(fmt, shape, seed=3)), dev(make(fmt, shape, seed=4))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ycc_sse(a, b, mx, 2)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.ycc_sse(a, b, mx, 2)
    a.copy_(dev(make(fmt, shape, seed=5)))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.ycc_sse(a, b, mx, 2))
    assert sse_as_ints(out.cpu().numpy()) == sse_as_ints(E.ycc_sse(host(a).astype(np.int64), host(b).astype(np.int64), mx.m, mx.off, 255, 2))


# ---- null outputs, n = 0, refusals -------------------------------------------------------------------------------------------------
def test_every_combination_of_outputs():
    fmt = FMTS["u16_10"]
    mx = matrix(3, fmt)
    a = make(fmt, (2, 1, 5, 7, 3), seed=6)
    want = expect_forward(a, mx, 2, fmt)
    for mask in range(1, 8):
        wanted = tuple(bool(mask >> k & 1) for k in range(3))
        rc, got = raw_forward(dev(a), mx, 2, fmt, want=wanted)
        assert rc == 0, last_error()
        for k in range(3):
            assert (got[k] is None) == (not wanted[k])
            assert got[k] is None or np.array_equal(got[k].astype(np.int64), want[k])
    rc, _ = raw_forward(dev(a), mx, 2, fmt, want=(False, False, False))
    assert rc == ERR_ARG and "all null" in last_error()
    sf = sample_format(fmt)
    (cr, y) = ops.rgb_to_ycc(dev(a), mx, 2, sample_format=sf, want=("cr", "y"))
    assert np.array_equal(host(cr).astype(np.int64), want[2]) and np.array_equal(host(y).astype(np.int64), want[0])
    (y4,) = ops.rgb_to_ycc(dev(a)[:, 0], mx, 2, sample_format=sf, want=("y",))
    assert tuple(y4.shape) == (2, 5, 7) and np.array_equal(host(y4).astype(np.int64), want[0][:, 0])
    with pytest.raises(ValueError, match="want"):
        ops.rgb_to_ycc(dev(a), mx, 2, sample_format=sf, want=())


def test_no_signals_succeed_and_launch_nothing():
    fmt = FMTS["u8"]
    mx = matrix(0, fmt)
    a = dev(make(fmt, (1, 1, 4, 4, 3)))
    rc, got = raw_forward(a, mx, 2, fmt, n=0)
    assert rc == 0 and all((g_ == SENT).all() for g_ in got)
    rc, sse = raw_sse(a, a, mx, 2, fmt, n=0)
    assert rc == 0 and (sse.view(np.uint8) == SENT).all()
    p = dev(make(fmt, (1, 4, 4)))
    rc, rgb = raw_inverse(p, p, p, mx, 0, fmt, n=0)
    assert rc == 0 and (rgb == SENT).all()
    assert tuple(ops.ycc_sse(a[:0], a[:0], mx, 2).shape) == (0, 1, 3)
    assert tuple(ops.ycc_to_rgb(p[:0], p[:0], p[:0], mx, 0).shape) == (0, 4, 4, 3)


REFUSALS_RGB = [
    (dict(kind=1), ERR_ARG, "kind 1"), (dict(kind=3), ERR_ARG, "kind 3"), (dict(depth=8), ERR_ARG, "depth 8"),
    (dict(kind=2, depth=0), ERR_ARG, "depth 0"), (dict(kind=2, depth=17), ERR_ARG, "depth 17"),
    (dict(ss=3), ERR_ARG, "subsampling 3"), (dict(ss=-1), ERR_ARG, "subsampling -1"),
    (dict(H=0), ERR_SHAPE, "0 x 6"), (dict(W=0), ERR_SHAPE, "4 x 0"), (dict(T=0), ERR_SHAPE, "0 frames"), (dict(n=-1), ERR_SHAPE, "-1 signals"),
    (dict(H=8193, W=8192), ERR_UNSUPPORTED, "2^26"),
    (dict(null=("m",)), ERR_ARG, "null matrix"), (dict(null=("off",)), ERR_ARG, "null matrix"),
]


@pytest.mark.parametrize("entry", ["rgb_to_ycc", "ycc_sse", "ycc_to_rgb"])
def test_refusals_name_their_reason_and_launch_nothing(entry):
    fmt = FMTS["u8"]
    mx = matrix(0, fmt)
    a = dev(make(fmt, (2, 3, 4, 6, 3), seed=1))
    planes = [dev(make(fmt, (2, 3, 4, 6), seed=2)), dev(make(fmt, (2, 3, 2, 3), seed=3)), dev(make(fmt, (2, 3, 2, 3), seed=4))]

    def call(**over):
        if entry == "rgb_to_ycc":
            rc, got = raw_forward(a, mx, over.pop("ss", 2), fmt, **over)
            return rc, all((g_ == SENT).all() for g_ in got)
        if entry == "ycc_sse":
            over = {("a_" + k if k in ("strides", "offset", "elems") else k): v for k, v in over.items()}
            over["null"] = tuple({"strides": "a_strides", "src": "a"}.get(v, v) for v in over.get("null", ()))
            rc, sse = raw_sse(a, a, mx, over.pop("ss", 2), fmt, **over)
            return rc, bool((sse.view(np.uint8) == SENT).all())
        over["null"] = tuple({"m": "inv", "off": "o"}.get(v, v) for v in over.get("null", ()))
        rc, rgb = raw_inverse(*planes, mx, over.pop("ss", 2), fmt, **over)
        return rc, bool((rgb == SENT).all())

    for over, code, text in REFUSALS_RGB:
        rc, untouched = call(**dict(over))
        assert rc == code and untouched, (over, rc, last_error())
        assert text in last_error() and last_error().startswith(entry), (over, last_error())
    wg_n = (1 << 31)                                         # 2^31 signals of one workgroup each, every signal the same memory
    if entry == "ycc_to_rgb":
        more = [(dict(strides=[[6 * 4 * 3, 24, 6, -1]] + [[18, 6, 3, 1]] * 2), ERR_ARG, "negative stride of the Y plane"),
                (dict(strides=[[72, 24, 6, 1], [18, 6, 3, 1], [18, 6, -3, 1]]), ERR_ARG, "negative stride of the Cr plane"),
                (dict(elems=[143, 36, 36]), ERR_SHAPE, "the Y plane reaches past its 143 elements"),
                (dict(elems=[144, 35, 36]), ERR_SHAPE, "the Cb plane reaches past its 35 elements"),
                (dict(elems=[144, 36, 0]), ERR_SHAPE, "the Cr plane reaches past"),
                (dict(strides=[[72, 24, 6, 1], [18, 6, 3, 1 << 62], [18, 6, 3, 1]]), ERR_SHAPE, "the Cb plane reaches past"),
                (dict(null=("py",)), ERR_ARG, "null py"), (dict(null=("pcr",)), ERR_ARG, "null py"), (dict(null=("dst",)), ERR_ARG, "null py"),
                (dict(null=("strides1",)), ERR_ARG, "null strides of the Cb plane"), (dict(null=("elems",)), ERR_ARG, "null element counts"),
                (dict(n=wg_n, T=1, strides=[[0, 0, 6, 1], [0, 0, 3, 1], [0, 0, 3, 1]]), ERR_UNSUPPORTED, "2^31 - 1 workgroups")]
    else:
        name = "src" if entry == "rgb_to_ycc" else "a"
        more = [(dict(strides=[72 * 3, 72, 18, 3, -1]), ERR_ARG, "negative stride of %s" % name),
                (dict(offset=-1), ERR_ARG, "negative offset"),
                (dict(elems=431), ERR_SHAPE, "%s reaches past its 431 elements" % name),
                (dict(offset=1), ERR_SHAPE, "%s reaches past its 432 elements" % name),
                (dict(strides=[1 << 62, 72, 18, 3, 1]), ERR_SHAPE, "reaches past"),
                (dict(null=("src",)), ERR_ARG, "null %s" % name), (dict(null=("strides",)), ERR_ARG, "null strides of %s" % name),
                (dict(n=wg_n, T=1, strides=[0, 0, 18, 3, 1], **({"b_strides": [0, 0, 18, 3, 1]} if entry == "ycc_sse" else {})),
                 ERR_UNSUPPORTED, "2^31 - 1 workgroups")]
        if entry == "ycc_sse":
            more.append((dict(null=("sse",)), ERR_ARG, "null sse"))
    for over, code, text in more:
        rc, untouched = call(**dict(over))
        assert rc == code and untouched, (over, rc, last_error())
        assert text in last_error(), (over, last_error())
    # the sizes at the limit are taken: 2^26 positions is legal (checked without a launch: the reach is refused next)
    rc, _ = call(H=8192, W=8192)
    assert rc == ERR_SHAPE and "reaches past" in last_error()


def test_wrappers_raise_with_the_entry_s_message():
    fmt = FMTS["u8"]
    mx = matrix(0, fmt)
    a = dev(make(fmt, (2, 4, 6, 3)))
    with pytest.raises(RcbError, match="subsampling 3"):
        ops.rgb_to_ycc(a, mx, 3)
    with pytest.raises(RcbError, match="three channels needed"):
        ops.ycc_sse(a[..., :2], a[..., :2], mx, 2)
    with pytest.raises(RcbError, match="kind 1"):
        ops.rgb_to_ycc(a.float(), mx, 2)
    with pytest.raises(ValueError, match="sample_format"):
        ops.rgb_to_ycc(a.to(torch.int16), mx, 2)
    with pytest.raises(ValueError, match="formed for"):
        ops.ycc_sse(a, a, utils.ycc_matrix("bt601", True, SampleFormat.u16(10)), 2)
    with pytest.raises(RcbError, match="chroma planes"):
        ops.ycc_to_rgb(a[..., 0], a[..., 1], a[..., 2], mx, 2)
    with pytest.raises(RcbError, match="one shape"):
        ops.ycc_sse(a, a[:1], mx, 2)
    out = torch.empty(2, 4, 6, 3, device=DEV, dtype=torch.uint8)
    assert ops.ycc_to_rgb(a[..., 0], a[..., 1], a[..., 2], mx, 0, out=out) is out
    with pytest.raises(RcbError, match="output of shape"):
        ops.ycc_to_rgb(a[..., 0], a[..., 1], a[..., 2], mx, 0, out=out[:1])
