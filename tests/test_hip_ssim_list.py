"""rcb_ssim_list (N4 415) -- lists of images of mixed sizes and layouts, and the frames of clips, in one call -- against the numpy
evaluator (tests/ssim_emul.py) and against rcb_ssim itself on each image alone: every comparison is of integers, bit for bit.
The kernels' tiles are 16 x 16 window positions (tests/test_hip_ssim.py), so the extents run over 11, 26, 27, 42, 43: one
position, a tile, a tile and a sliver, two tiles, two tiles and a sliver."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ssim_emul as E
from test_hip_ssim import DEV, ERR_ARG, ERR_SHAPE, FMTS, SENT_B, SENT_I, _guarded, _vp, dev, make

pytestmark = pytest.mark.gpu

from recombiner_amd import _lib, ops, utils  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

EDGES = [(11, 11), (26, 27), (27, 26), (43, 11), (11, 43), (42, 42), (43, 43)]


@functools.lru_cache(maxsize=None)
def images(name, shapes, Cc, scales=1, kind="smooth"):
    """one seeded pair per shape -> ([a_k], [b_k]) numpy [H, W, C], and the evaluator's sums [n, scales, C, 2]; computed once"""
    a, b = [], []
    for k, (H, W) in enumerate(shapes):
        x, y = make(kind if k % 2 else "noise", FMTS[name], (1, H, W, Cc), seed=100 + k)
        a.append(x[0]), b.append(y[0])
    L = E.level_max(*FMTS[name])
    want = np.asarray([E.sums(x.astype(np.int64), y.astype(np.int64), L, scales) for x, y in zip(a, b)], dtype=np.int64)
    want.setflags(write=False)
    return a, b, want


def fmt_of(name):
    return SampleFormat(*FMTS[name]) if FMTS[name][0] else None


def run(a, b, name, scales=1):
    return ops.ssim_sums_list(a, b, sample_format=fmt_of(name), scales=scales).cpu().numpy()


# ---- tile and prefix edges, list order -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,Cc", [("u8", 3), ("u16_12", 1)])
def test_tile_and_prefix_edges(name, Cc):
    a, b, want = images(name, tuple(EDGES), Cc)
    ta, tb = [dev(x) for x in a], [dev(x) for x in b]
    got = run(ta, tb, name)
    assert got.shape == (len(EDGES), 1, Cc, 2) and got.dtype == np.int64
    assert np.array_equal(got, want)
    rev = run(ta[::-1], tb[::-1], name)
    assert np.array_equal(rev, want[::-1])
    perm = np.random.default_rng(5).permutation(len(EDGES))
    assert not np.array_equal(perm, np.arange(len(EDGES)))
    assert np.array_equal(run([ta[i] for i in perm], [tb[i] for i in perm], name), want[perm])
    # twice: the same integers
    assert np.array_equal(run(ta, tb, name), got)


# ---- scales ------------------------------------------------------------------------------------------------------------------------
def test_two_scales_drop_odd_rows_and_columns():
    shapes = ((45, 23), (22, 22), (47, 50))
    a, b, want = images("u8", shapes, 3, scales=2)
    got = run([dev(x) for x in a], [dev(x) for x in b], "u8", scales=2)
    assert np.array_equal(got, want)


def test_five_scales():
    shapes = ((176, 176), (177, 191), (190, 176))
    a, b, want = images("u8", shapes, 2, scales=5)
    ta, tb = [dev(x) for x in a], [dev(x) for x in b]
    got = run(ta, tb, "u8", scales=5)
    assert np.array_equal(got, want)
    assert np.array_equal(run(ta, tb, "u8", scales=5), got)
    # the figures through the package's own path are the evaluator's floats
    Hs, Ws = [s[0] for s in shapes], [s[1] for s in shapes]
    ms = utils.ssim_device(ta, tb, multiscale=True)
    assert ms.tolist() == [E.msssim_figure(want[k].tolist(), Hs[k], Ws[k]) for k in range(3)]
    ss = utils.ssim_device(ta, tb)
    assert ss.tolist() == [E.ssim_figure(want[k].tolist(), Hs[k], Ws[k]) for k in range(3)]


# ---- each image against rcb_ssim on that image alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,Cc,scales", [("u8", 3, 1), ("u16_12", 1, 1), ("u8", 3, 2)])
def test_each_row_is_what_rcb_ssim_gives_for_the_image_alone(name, Cc, scales):
    shapes = tuple(EDGES) if scales == 1 else ((45, 23), (22, 22), (47, 50))
    a, b, _ = images(name, shapes, Cc, scales=scales)
    ta, tb = [dev(x) for x in a], [dev(x) for x in b]
    got = ops.ssim_sums_list(ta, tb, sample_format=fmt_of(name), scales=scales)
    for k in range(len(shapes)):
        alone, _ = ops.ssim_sums(ta[k][None], tb[k][None], sample_format=fmt_of(name), scales=scales)
        assert torch.equal(got[k], alone[0]), k


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
def test_mixed_layouts_in_one_list():
    """a transposed view, a channel-first view, a window of a larger image, an expanded channel, `a` as views of ONE buffer at
    offsets, `b` in separate allocations: all in one call, all the sums of contiguous copies"""
    shapes = ((27, 43), (43, 27), (30, 31), (26, 26), (11, 50))
    a, b, _ = images("u8", shapes, 3)
    gray = a[3][..., :1]
    src_a = [a[0], a[1], a[2], np.repeat(gray, 3, -1), a[4]]
    want = np.asarray([E.sums(x.astype(np.int64), y.astype(np.int64), 255, 1) for x, y in zip(src_a, b)], dtype=np.int64)
    # a: every image a view into one buffer, each in a layout of its own
    sizes = [x.size for x in src_a]
    pool = torch.zeros(sum(sizes) + 4096, device=DEV, dtype=torch.uint8)
    va, off = [], 7                                          # (an odd start: nothing is aligned)
    t0 = dev(src_a[0])
    pool[off:off + sizes[0]] = t0.transpose(0, 1).contiguous().reshape(-1)
    va.append(pool[off:off + sizes[0]].view(43, 27, 3).transpose(0, 1))                     # transposed
    off += sizes[0] + 3
    pool[off:off + sizes[1]] = dev(src_a[1]).permute(2, 0, 1).contiguous().reshape(-1)
    va.append(pool[off:off + sizes[1]].view(3, 43, 27).permute(1, 2, 0))                    # channel-first
    off += sizes[1] + 1
    H, W = shapes[2]
    big = pool[off:off + (H + 5) * (W + 7) * 3].view(H + 5, W + 7, 3)
    big[2:2 + H, 3:3 + W] = dev(src_a[2])
    va.append(big[2:2 + H, 3:3 + W])                                                        # a window
    off += (H + 5) * (W + 7) * 3 + 5
    pool[off:off + 26 * 26] = dev(np.ascontiguousarray(gray)).reshape(-1)
    va.append(pool[off:off + 26 * 26].view(26, 26, 1).expand(26, 26, 3))                    # an expanded channel
    off += 26 * 26 + 2
    pool[off:off + sizes[4]] = dev(src_a[4]).reshape(-1)
    va.append(pool[off:off + sizes[4]].view(11, 50, 3))
    assert va[3].stride(2) == 0 and not va[0].is_contiguous() and not va[1].is_contiguous() and not va[2].is_contiguous()
    assert all(torch.equal(v, dev(x)) for v, x in zip(va, src_a))
    assert len({v.untyped_storage().data_ptr() for v in va}) == 1
    # b: separate allocations, two of them in layouts of their own
    vb = [dev(y) for y in b]
    vb[1] = vb[1].transpose(0, 1).contiguous().transpose(0, 1)
    vb[4] = vb[4].permute(2, 0, 1).contiguous().permute(1, 2, 0)
    got = ops.ssim_sums_list(va, vb).cpu().numpy()
    assert np.array_equal(got, want)
    cont = ops.ssim_sums_list([v.contiguous() for v in va], [v.contiguous() for v in vb]).cpu().numpy()
    assert np.array_equal(got, cont)
    # two scales through the same views (the pooling kernel reads the strides too): the sizes that allow them
    keep = [0, 1, 2, 3]
    got2 = ops.ssim_sums_list([va[k] for k in keep], [vb[k] for k in keep], scales=2).cpu().numpy()
    want2 = np.asarray([E.sums(src_a[k].astype(np.int64), b[k].astype(np.int64), 255, 2) for k in keep], dtype=np.int64)
    assert np.array_equal(got2, want2)


# ---- the frames of clips -----------------------------------------------------------------------------------------------------------
def test_frames_of_clips():
    n, T, H, W, Cc = 2, 3, 27, 30, 3
    a, b = make("smooth", FMTS["u8"], (n * T, H, W, Cc), seed=21)
    want = E.batch_sums(a.astype(np.int64), b.astype(np.int64), 255).reshape(n, T, 1, Cc, 2)
    ta, tb = dev(a).view(n, T, H, W, Cc), dev(b).view(n, T, H, W, Cc)
    got = ops.ssim_sums_frames(ta, tb)
    assert tuple(got.shape) == (n, T, 1, Cc, 2) and np.array_equal(got.cpu().numpy(), want)
    # the n and T axes exchanged in memory (a), and the frame axis innermost but for the channels (b)
    pa = ta.transpose(0, 1).contiguous().transpose(0, 1)
    pb = tb.permute(0, 2, 3, 1, 4).contiguous().permute(0, 3, 1, 2, 4)
    assert pa.stride(0) < pa.stride(1) and pb.stride(1) == Cc and torch.equal(pa, ta) and torch.equal(pb, tb)
    assert np.array_equal(ops.ssim_sums_frames(pa, pb).cpu().numpy(), want)
    figs = utils.ssim_frames_device(pa, pb)
    assert figs.shape == (n, T) and figs.dtype == np.float64
    assert figs.tolist() == [[E.ssim_figure(want[i, t].tolist(), H, W) for t in range(T)] for i in range(n)]
    with pytest.raises(ValueError, match="too small"):
        utils.ssim_frames_device(pa, pb, multiscale=True)
    with pytest.raises(_lib.RcbError):
        ops.ssim_sums_frames(ta, tb[:, :2])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def raw_list(a, b, fmt, scales=1, **over):
    """rcb_ssim_list on two lists of CONTIGUOUS device images packed into one buffer per operand, with guarded sums, workspace and
    table -> (rc, sums or None, untouched: sums still holds its sentinel).  `over` replaces single arguments."""
    lib = _lib.load()
    n, Cc = len(a), int(a[0].shape[-1]) if a else 3
    kind, depth = fmt
    sizes = np.asarray([[t.shape[0], t.shape[1]] for t in a], dtype=np.int32).reshape(n, 2)
    spans = np.zeros((n, 4), dtype=np.int64)
    off = 0
    for k, t in enumerate(a):
        spans[k] = [off, t.shape[1] * Cc, Cc, 1]
        off += t.numel()
    buf_a = torch.cat([t.reshape(-1) for t in a]) if n else torch.zeros(1, device=DEV, dtype=torch.uint8)
    buf_b = torch.cat([t.reshape(-1) for t in b]) if n else torch.zeros(1, device=DEV, dtype=torch.uint8)
    g = dict(kind=kind, depth=depth, n=n, sizes=sizes, a_spans=spans, b_spans=spans.copy(), C=Cc, scales=scales, a_elems=off,
             b_elems=off, null=(), ws_delta=0, tab_delta=0, tab_shift=0)
    g.update(over)
    L = E.level_max(kind if kind in (0, 2) else 0, depth if 9 <= depth <= 16 else 9)
    c1, c2 = E.constants(L)
    win = np.ascontiguousarray(utils.ssim_window())
    n_sums = max(n, 1) * max(min(g["scales"], 5), 1) * Cc * 2
    _, sums, check_s = _guarded(n_sums, torch.int64, SENT_I)
    need = int(lib.rcb_ssim_list_workspace_bytes(n, _vp(sizes), Cc, scales))
    n_tab = int(lib.rcb_ssim_list_table_bytes(n, scales))
    _, ws, check_w = _guarded(max(need, 16), torch.uint8, SENT_B, pad=64)
    _, tab, check_t = _guarded(max(n_tab, 8) + 8, torch.uint8, SENT_B, pad=64)
    assert ws.data_ptr() % 16 == 0 and tab.data_ptr() % 8 == 0
    sz, sa, sb = (np.ascontiguousarray(g[k]) for k in ("sizes", "a_spans", "b_spans"))
    rc = lib.rcb_ssim_list(None if "a" in g["null"] else _vp(buf_a), g["a_elems"], None if "b" in g["null"] else _vp(buf_b),
                           g["b_elems"], g["kind"], g["depth"], g["n"], None if "sizes" in g["null"] else _vp(sz),
                           None if "a_spans" in g["null"] else _vp(sa), None if "b_spans" in g["null"] else _vp(sb), g["C"],
                           None if "win" in g["null"] else _vp(win), c1, c2, g["scales"], None if "sums" in g["null"] else _vp(sums),
                           None if "ws" in g["null"] else _vp(ws), max(need, 0) + g["ws_delta"],
                           None if "table" in g["null"] else C.c_void_p(tab.data_ptr() + g["tab_shift"]), max(n_tab, 0) + g["tab_delta"],
                           ops.stream_ptr())
    torch.cuda.synchronize()
    check_s(), check_w(), check_t()
    untouched = bool((sums == SENT_I).all().item())
    if rc != 0 or n == 0:
        return rc, None, untouched
    return rc, sums.view(n, scales, Cc, 2).cpu().numpy(), untouched


def test_refusals_launch_nothing():
    lib = _lib.load()
    fmt = FMTS["u8"]
    shapes = ((43, 45), (26, 40), (22, 31))
    a, b, want = images("u8", shapes, 3, scales=2)
    ta, tb = [dev(x) for x in a], [dev(x) for x in b]
    rc, sums, untouched = raw_list(ta, tb, fmt, scales=2)
    assert rc == 0 and not untouched and np.array_equal(sums, want)      # the call the refusals below are one step away from
    total = sum(x.size for x in a)

    def spans(k, col, value):
        s = np.zeros((3, 4), dtype=np.int64)
        o = 0
        for i, x in enumerate(a):
            s[i] = [o, x.shape[1] * 3, 3, 1]
            o += x.size
        s[k, col] = value
        return s
    small = np.asarray([[43, 45], [10, 40], [22, 31]], dtype=np.int32)
    short = np.asarray([[43, 45], [21, 40], [22, 31]], dtype=np.int32)
    bad = [(dict(a_elems=total - 1), ERR_SHAPE), (dict(b_elems=total - 1), ERR_SHAPE),       # a reach one element past the end
           (dict(a_spans=spans(0, 1, -135)), ERR_ARG), (dict(b_spans=spans(2, 3, -1)), ERR_ARG), (dict(a_spans=spans(1, 0, -1)), ERR_ARG),
           (dict(a_spans=spans(2, 0, total - 22 * 31 * 3 + 1)), ERR_SHAPE),
           (dict(tab_delta=-1), ERR_SHAPE), (dict(tab_shift=4), ERR_SHAPE), (dict(ws_delta=-1), ERR_SHAPE), (dict(null=("ws",)), ERR_SHAPE),
           (dict(kind=1), ERR_ARG), (dict(kind=3), ERR_ARG), (dict(kind=2, depth=8), ERR_ARG), (dict(depth=8), ERR_ARG),
           (dict(sizes=small), ERR_SHAPE), (dict(sizes=short), ERR_SHAPE), (dict(scales=3), ERR_SHAPE), (dict(scales=0), ERR_ARG),
           (dict(scales=6), ERR_ARG), (dict(C=33), ERR_SHAPE), (dict(n=-1), ERR_SHAPE),
           (dict(null=("sizes",)), ERR_ARG), (dict(null=("a_spans",)), ERR_ARG), (dict(null=("b_spans",)), ERR_ARG),
           (dict(null=("table",)), ERR_ARG), (dict(null=("a",)), ERR_ARG), (dict(null=("b",)), ERR_ARG), (dict(null=("sums",)), ERR_ARG),
           (dict(null=("win",)), ERR_ARG)]
    for kw, code in bad:
        rc, _, untouched = raw_list(ta, tb, fmt, **{"scales": 2, **kw})
        assert rc == code and untouched, (kw, rc)
        assert lib.rcb_last_error_string()
    rc, _, untouched = raw_list(ta, tb, fmt, scales=2, sizes=small)
    assert b"image 1" in lib.rcb_last_error_string()
    # no images: succeeds and launches nothing
    rc, _, untouched = raw_list([], [], fmt, scales=2, null=("a", "b", "sums", "ws", "table", "sizes", "a_spans", "b_spans"))
    assert rc == 0 and untouched


def test_wrapper_checks():
    a, b, _ = images("u16_12", ((22, 22), (30, 23)), 1)
    ta, tb = [dev(x) for x in a], [dev(x) for x in b]
    fmt = SampleFormat.u16(12)
    with pytest.raises(ValueError, match="sample_format"):
        ops.ssim_sums_list(ta, tb)
    with pytest.raises(_lib.RcbError):
        ops.ssim_sums_list(ta, tb, sample_format=SampleFormat.u8())
    with pytest.raises(_lib.RcbError):
        ops.ssim_sums_list(ta, tb[:1], sample_format=fmt)
    with pytest.raises(_lib.RcbError):
        ops.ssim_sums_list(ta, [tb[0], tb[1][:, :22]], sample_format=fmt)
    with pytest.raises(_lib.RcbError, match="image 0"):
        ops.ssim_sums_list(ta, tb, sample_format=fmt, scales=3)
    with pytest.raises(_lib.RcbError):
        ops.ssim_sums_list([], [], sample_format=fmt)
    with pytest.raises(ValueError, match="too small"):
        utils.ssim_device(ta, tb, sample_format=fmt, multiscale=True)
    # an int16 tensor holds the same bits as the uint16 one
    s1 = ops.ssim_sums_list(ta, tb, sample_format=fmt, scales=2)
    s2 = ops.ssim_sums_list([t.view(torch.int16) for t in ta], tb, sample_format=fmt, scales=2)
    assert torch.equal(s1, s2) and tuple(s1.shape) == (2, 2, 1, 2)
