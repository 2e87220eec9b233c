"""The premises of tests/ycc_emul.py, the evaluator tests/test_hip_ycc.py holds rcb_ycc_to_rgb, rcb_rgb_to_ycc and rcb_ycc_sse to
(include/rcb.h, N4 418), and of utils.ycc_matrix, which forms the constants the device is given.  No GPU."""
import math
import os
import re
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ycc_emul as E  # noqa: E402
from recombiner_amd import _lib, utils  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

STANDARDS = {"bt601": (Fr(299, 1000), Fr(114, 1000)), "bt709": (Fr(2126, 10000), Fr(722, 10000)),
             "bt2020": (Fr(2627, 10000), Fr(593, 10000))}


def fmt_of(d):
    return SampleFormat.u8() if d == 8 else SampleFormat.u16(d)


def restated(kr, kb, full, d):
    """the header's constants in exact rational arithmetic, written out once more: (m, off, n) as Fractions"""
    kg = 1 - kr - kb
    L = (1 << d) - 1
    sy, sc = (Fr(1), Fr(1)) if full else (Fr(219 * 2 ** (d - 8), L), Fr(224 * 2 ** (d - 8), L))
    off = [Fr(0), Fr(2 ** (d - 1)), Fr(2 ** (d - 1))] if full else [Fr(16 * 2 ** (d - 8)), Fr(128 * 2 ** (d - 8)), Fr(128 * 2 ** (d - 8))]
    db, dr = 2 * (1 - kb), 2 * (1 - kr)
    m = [[kr * sy, kg * sy, kb * sy], [-kr / db * sc, -kg / db * sc, sc / 2], [sc / 2, -kg / dr * sc, -kb / dr * sc]]
    n = [[1 / sy, Fr(0), dr / sc], [1 / sy, -kb * db / kg / sc, -kr * dr / kg / sc], [1 / sy, db / sc, Fr(0)]]
    return m, off, n


def ulps(value, exact):
    """|value - exact| in units of the last place of `value` (0 for a zero that is exact)"""
    if exact == 0:
        return 0.0 if value == 0.0 else math.inf
    return float(abs(Fr(value) - exact) / Fr(math.ulp(value)))


@pytest.mark.parametrize("standard", sorted(STANDARDS) + ["pair"])
@pytest.mark.parametrize("full", [True, False])
def test_matrix_agrees_with_a_fraction_restatement(standard, full):
    for d in (8, 10, 12, 16):
        if standard == "pair":
            pair = (0.25, 0.125)                             # (floats stand for their exact values)
            got, (kr, kb) = utils.ycc_matrix(pair, full, fmt_of(d)), (Fr(pair[0]), Fr(pair[1]))
        else:
            got, (kr, kb) = utils.ycc_matrix(standard, full, fmt_of(d)), STANDARDS[standard]
        m, off, n = restated(kr, kb, full, d)
        for k in range(3):
            assert Fr(float(got.off[k])) == off[k] == Fr(float(got.o[k]))
            for j in range(3):
                assert ulps(float(got.m[k, j]), m[k][j]) <= 1.0, (standard, full, d, "m", k, j)
                assert ulps(float(got.n[k, j]), n[k][j]) <= 1.0, (standard, full, d, "n", k, j)
        assert got.m.dtype == got.n.dtype == got.off.dtype == got.o.dtype == np.float64
    # the forward and the inverse are each other's inverse in exact arithmetic
    m, _, n = restated(*STANDARDS["bt709"], False, 10)
    for i in range(3):
        for j in range(3):
            assert sum(n[i][k] * m[k][j] for k in range(3)) == (1 if i == j else 0)


def test_matrix_refusals():
    with pytest.raises(ValueError, match="standard"):
        utils.ycc_matrix("bt470", True, None)
    with pytest.raises(ValueError, match="kg"):
        utils.ycc_matrix((0.6, 0.5), True, None)
    with pytest.raises(ValueError, match="u8 and u16"):
        utils.ycc_matrix("bt601", True, SampleFormat.f32())


@pytest.mark.parametrize("standard", sorted(STANDARDS))
def test_gray_gives_neutral_chroma_and_its_own_luma_at_full_range(standard):
    for d in range(8, 17):
        L = (1 << d) - 1
        mx = utils.ycc_matrix(standard, True, fmt_of(d))
        v = np.arange(L + 1, dtype=np.int64) if d <= 12 else np.unique(np.r_[0:300, L - 300:L + 1, np.arange(0, L + 1, 97)])
        rgb = np.repeat(v[None, :, None], 3, axis=2)          # [1, W, 3]
        for ss in (0, 1, 2):
            y, cb, cr = E.rgb_to_ycc(rgb, mx.m, mx.off, L, ss)
            assert np.array_equal(y[0], v)
            assert (cb == 1 << (d - 1)).all() and (cr == 1 << (d - 1)).all()


@pytest.mark.parametrize("standard", sorted(STANDARDS))
def test_limited_range_maps_black_and_white_to_the_nominal_levels(standard):
    for d in range(8, 17):
        L = (1 << d) - 1
        mx = utils.ycc_matrix(standard, False, fmt_of(d))
        rgb = np.asarray([[[0, 0, 0], [L, L, L]]], dtype=np.int64)
        y, cb, cr = E.rgb_to_ycc(rgb, mx.m, mx.off, L, 0)
        assert y.tolist() == [[16 << (d - 8), 235 << (d - 8)]]
        assert cb.tolist() == cr.tolist() == [[128 << (d - 8)] * 2]
        back = E.ycc_to_rgb(y, cb, cr, mx.n, mx.o, L, 0)
        assert back.tolist() == rgb.tolist()
    mx = utils.ycc_matrix(standard, False, None)
    assert E.rgb_to_ycc(np.asarray([[[0, 0, 0], [255, 255, 255]]]), mx.m, mx.off, 255, 0)[0].tolist() == [[16, 235]]
    mx = utils.ycc_matrix(standard, False, SampleFormat.u16(10))
    assert E.rgb_to_ycc(np.asarray([[[0, 0, 0], [1023, 1023, 1023]]]), mx.m, mx.off, 1023, 0)[0].tolist() == [[64, 940]]


def test_footroom_and_headroom_are_not_clamped_away():
    """the clamp is to [0, L] only: a limited-range Y below 16 or above 235 goes to RGB as it is"""
    mx = utils.ycc_matrix("bt601", False, None)
    y = np.asarray([[3, 250]])
    c = np.full((1, 2), 128)
    got = E.ycc_to_rgb(y, c, c, mx.n, mx.o, 255, 0)
    assert got[0, 0].tolist() == [0, 0, 0] and got[0, 1].tolist() == [255, 255, 255]
    mid = E.ycc_to_rgb(np.asarray([[17]]), np.asarray([[128]]), np.asarray([[128]]), mx.n, mx.o, 255, 0)
    assert mid[0, 0].tolist() == [1, 1, 1]


def test_replicating_up_and_block_mean_down_returns_the_chroma_planes():
    rng = np.random.default_rng(1)
    for ss, (H, W) in ((1, (6, 8)), (2, (6, 8)), (2, (2, 2))):
        Hc, Wc = E.chroma_size(H, W, ss)
        c = rng.uniform(-200.0, 200.0, size=(2, Hc, Wc))
        rows = np.arange(H) >> 1 if ss == 2 else np.arange(H)
        up = c[:, rows, :][:, :, np.arange(W) >> 1]
        assert np.array_equal(E.chroma_mean(up, ss), c)       # (a + a, 2a + 2a and the scalings by 0.5 / 0.25 are exact)
    # and through the integers: planes -> rgb at 4:4:4 of the replicated planes -> the same planes, where nothing is clamped
    mx = utils.ycc_matrix("bt601", True, None)
    y = rng.integers(60, 190, size=(4, 6))
    cb, cr = rng.integers(100, 156, size=(2, 2, 3))
    rgb = E.ycc_to_rgb(y, cb, cr, mx.n, mx.o, 255, 2)
    same = E.ycc_to_rgb(y, np.repeat(np.repeat(cb, 2, 0), 2, 1), np.repeat(np.repeat(cr, 2, 0), 2, 1), mx.n, mx.o, 255, 0)
    assert np.array_equal(rgb, same)


def test_odd_sizes_clip_the_far_row_and_column():
    """3 x 5 by hand: the block of chroma sample (i, j) is rows {2i, min(2i+1, 2)} x columns {2j, min(2j+1, 4)}"""
    p = np.arange(15, dtype=np.float64).reshape(3, 5) * 1.25
    c420 = E.chroma_mean(p, 2)
    assert c420.shape == (2, 3)
    want = [[((p[0, 0] + p[0, 1]) + (p[1, 0] + p[1, 1])) * 0.25, ((p[0, 2] + p[0, 3]) + (p[1, 2] + p[1, 3])) * 0.25,
             ((p[0, 4] + p[0, 4]) + (p[1, 4] + p[1, 4])) * 0.25],
            [((p[2, 0] + p[2, 1]) + (p[2, 0] + p[2, 1])) * 0.25, ((p[2, 2] + p[2, 3]) + (p[2, 2] + p[2, 3])) * 0.25,
             ((p[2, 4] + p[2, 4]) + (p[2, 4] + p[2, 4])) * 0.25]]
    assert c420.tolist() == want
    c422 = E.chroma_mean(p, 1)
    assert c422.shape == (3, 3)
    assert c422.tolist() == [[(p[r, 0] + p[r, 1]) * 0.5, (p[r, 2] + p[r, 3]) * 0.5, (p[r, 4] + p[r, 4]) * 0.5] for r in range(3)]
    assert E.chroma_size(3, 5, 0) == (3, 5) and E.chroma_size(1, 1, 2) == (1, 1) and E.chroma_size(1, 7, 1) == (1, 4)
    # the inverse reads (y >> 1, x >> 1): position (2, 4) of a 3 x 5 frame reads chroma (1, 2)
    mx = utils.ycc_matrix("bt601", True, None)
    y = np.full((3, 5), 128)
    cb = np.full((2, 3), 128)
    cr = np.full((2, 3), 128)
    cr[1, 2] = 200
    got = E.ycc_to_rgb(y, cb, cr, mx.n, mx.o, 255, 2)
    changed = (got != 128).any(axis=-1)
    assert changed.tolist() == [[False] * 5, [False] * 5, [False] * 4 + [True]]


# ---- mutants: each is a plausible misreading of the header, and the evaluator must differ from it on the inputs the GPU tests use
def _planes(rgb, mx, ss, chroma=E.chroma_mean):
    p = E.forward_unrounded(rgb, mx.m)
    return [E.quantise(chroma(p[k], ss) + mx.off[k], 255) for k in (1, 2)]


def test_mutant_chroma_rounded_before_the_mean():
    rng = np.random.default_rng(2)
    rgb = rng.integers(0, 256, size=(17, 65, 3))
    mx = utils.ycc_matrix("bt601", True, None)

    def rounded_first(p, ss):
        return E.chroma_mean(np.rint(p), ss)
    for ss in (1, 2):
        good, bad = _planes(rgb, mx, ss), _planes(rgb, mx, ss, rounded_first)
        assert any((g != b).any() for g, b in zip(good, bad))


def test_mutant_mean_without_edge_clipping():
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, size=(5, 7, 3))
    mx = utils.ycc_matrix("bt601", True, None)

    def zero_padded(p, ss):                                  # the far row / column read as 0 instead of replicated
        H, W = p.shape
        Hc, Wc = E.chroma_size(H, W, ss)
        full = np.zeros((2 * Hc if ss == 2 else H, 2 * Wc))
        full[:H, :W] = p
        return E.chroma_mean(full, ss)
    for ss in (1, 2):
        good, bad = _planes(rgb, mx, ss), _planes(rgb, mx, ss, zero_padded)
        assert all(g.shape == b.shape for g, b in zip(good, bad))
        assert any((g != b).any() for g, b in zip(good, bad))
        assert all(np.array_equal(g[:2, :3], b[:2, :3]) for g, b in zip(good, bad))     # (only the far edge can tell)


def test_mutant_chroma_index_rounded_up():
    rng = np.random.default_rng(4)
    y = rng.integers(16, 236, size=(5, 7))
    mx = utils.ycc_matrix("bt709", True, None)
    for ss in (1, 2):
        Hc, Wc = E.chroma_size(5, 7, ss)
        cb, cr = rng.integers(16, 241, size=(2, Hc, Wc))
        good = E.ycc_to_rgb(y, cb, cr, mx.n, mx.o, 255, ss)
        cols = np.minimum((np.arange(7) + 1) >> 1, Wc - 1)
        bad = E.ycc_to_rgb(y, cb[:, cols], cr[:, cols], mx.n, mx.o, 255, 2 if ss == 2 else 0) if ss == 1 else \
            E.ycc_to_rgb(y, cb[np.arange(5) >> 1][:, cols], cr[np.arange(5) >> 1][:, cols], mx.n, mx.o, 255, 0)
        assert good.shape == bad.shape and (good != bad).any()


def contracted_changes(mx, L=255):
    """How many of the 3 * 2^24 integers of the full 8-bit RGB cube at 4:4:4 change when every a * b + c of p_k is rounded ONCE (a
    fused multiply-add, formed exactly with Fraction): p_k = fma(m2, b, fma(m1, g, m0 * r)).  Both forms lie within 4 ulp(256) <
    3e-13 of each other, so only the values within 1e-6 of a rounding boundary can change; those are evaluated exactly."""
    changed = [0, 0, 0]
    m = [[Fr(float(v)) for v in row] for row in mx.m]
    for lo in range(0, 1 << 24, 1 << 20):
        v = np.arange(lo, lo + (1 << 20), dtype=np.int64)
        rgb = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1)
        p = E.forward_unrounded(rgb, mx.m)
        for k in range(3):
            t = p[k] + mx.off[k]
            near = np.nonzero(np.abs((t - np.floor(t)) - 0.5) < 1e-6)[0]
            plain = E.quantise(t[near], L)
            for i, q in zip(near, plain):
                r, g, b = (int(c) for c in rgb[i])
                first = float(mx.m[k, 0]) * r                 # (a lone product is rounded as it is)
                second = float(m[k][1] * g + Fr(first))
                third = float(m[k][2] * b + Fr(second))
                if int(E.quantise(np.float64(third) + mx.off[k], L)) != int(q):
                    changed[k] += 1
    return changed


@pytest.mark.parametrize("standard,full", [("bt601", True), ("bt709", False)])
def test_mutant_contracted_evaluation_changes_the_cube(standard, full):
    """the matrices tests/test_hip_ycc.py runs the cube with: a build that contracts a * b + c would be told apart there"""
    changed = contracted_changes(utils.ycc_matrix(standard, full, None))
    print("contracted evaluation, %s %s range: %r of 3 * 2^24 values change" % (standard, "full" if full else "limited", changed))
    assert sum(changed) > 0


def test_within_one_step_of_pillow():
    """BT.601 full range at 8 bits is Pillow's convert("YCbCr") but for its fixed-point tables, which are not copied: at most
    one step apart; the shares go to profiles/r24_ycc_vs_pillow.txt"""
    Image = pytest.importorskip("PIL.Image")
    import PIL
    rng = np.random.default_rng(24)
    rgb = rng.integers(0, 256, size=(256, 256, 3), dtype=np.uint8)
    theirs = np.asarray(Image.fromarray(rgb, "RGB").convert("YCbCr")).astype(np.int64)
    mx = utils.ycc_matrix("bt601", True, None)
    ours = np.stack(E.rgb_to_ycc(rgb, mx.m, mx.off, 255, 0), axis=-1)
    diff = np.abs(ours - theirs)
    shares = [(diff[..., k] != 0).mean() * 100.0 for k in range(3)]
    text = ("tests/test_ycc_emul_cpu.py::test_within_one_step_of_pillow -- the fp64 definition of include/rcb.h (N4 418; BT.601 full range,\n"
            "8 bit, 4:4:4, ONE rounding) against Pillow's Image.convert(\"YCbCr\") (fixed-point tables) on a seeded random 256 x 256 image\n"
            "plane  differing samples  largest difference\n"
            + "".join("%-5s  %6.2f %%           %d\n" % (name, shares[k], diff[..., k].max()) for k, name in enumerate(("Y", "Cb", "Cr"))))
    try:
        path = os.path.join(ROOT, "profiles", "r24_ycc_vs_pillow.txt")
        if not os.path.exists(path) or open(path).read() != text:
            with open(path, "w") as f:
                f.write(text)
    except OSError:
        pass
    print(text, "Pillow", PIL.__version__)
    assert diff.max() <= 1


def test_sse_is_the_python_int_sum_and_psnr_divides_integers():
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 65536, size=(2, 2, 3, 5, 7, 3))
    mx = utils.ycc_matrix("bt2020", True, SampleFormat.u16(16))
    sse = E.ycc_sse(a, b, mx.m, mx.off, 65535, 2)
    assert sse.shape == (2, 3, 3)
    ya, cba, _ = E.rgb_to_ycc(a[1, 2], mx.m, mx.off, 65535, 2)
    yb, cbb, _ = E.rgb_to_ycc(b[1, 2], mx.m, mx.off, 65535, 2)
    assert sse[1, 2, 0] == sum(int(u - v) ** 2 for u, v in zip(ya.ravel(), yb.ravel()))
    assert sse[1, 2, 1] == sum(int(u - v) ** 2 for u, v in zip(cba.ravel(), cbb.ravel()))
    assert (E.ycc_sse(a, a, mx.m, mx.off, 65535, 2) == 0).all()
    psnr = utils.psnr_ycc_from_sse(sse.astype(np.int64), 5, 7, 2, SampleFormat.u16(16))
    assert psnr.shape == (2, 3, 4)
    assert psnr[1, 2, 0] == 10.0 * math.log10((65535 * 65535 * 35) / int(sse[1, 2, 0]))
    assert psnr[1, 2, 2] == 10.0 * math.log10((65535 * 65535 * 12) / int(sse[1, 2, 2]))
    assert psnr[0, 0, 3] == (6.0 * psnr[0, 0, 0] + psnr[0, 0, 1] + psnr[0, 0, 2]) / 8.0
    zero = utils.psnr_ycc_from_sse(np.asarray([0, 4, 0]), 2, 2, 0, None)
    assert zero[0] == math.inf and zero[2] == math.inf and zero[3] == math.inf and zero[1] == 10.0 * math.log10(255 * 255 * 4 / 4)
    # the extreme case of the GPU test stays below 2^58: 16-bit all-L against all-0 at 2^26 positions
    assert 65535 ** 2 * (1 << 26) < 1 << 58


def test_yuv_planes_are_views_of_one_buffer():
    import torch
    n, T, H, W = 2, 3, 5, 7
    Hc, Wc = 3, 4
    frame = H * W + 2 * Hc * Wc
    buf = torch.arange(n * T * frame + 5, dtype=torch.int64).to(torch.uint8)[5:]     # (a storage offset is kept)
    raw = buf.numpy().reshape(n, T, frame)
    for layout in ("i420", "yv12", "nv12"):
        (y, cb, cr), ss = utils.yuv_planes(buf, n, T, H, W, layout)
        assert ss == 2 and all(p.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr() for p in (y, cb, cr))
        assert np.array_equal(y.numpy(), raw[:, :, :H * W].reshape(n, T, H, W))
        chroma = raw[:, :, H * W:]
        if layout == "nv12":
            first, second = chroma[..., 0::2], chroma[..., 1::2]
        else:
            first, second = chroma[..., :Hc * Wc], chroma[..., Hc * Wc:]
        if layout == "yv12":
            first, second = second, first
        assert np.array_equal(cb.numpy(), first.reshape(n, T, Hc, Wc)) and np.array_equal(cr.numpy(), second.reshape(n, T, Hc, Wc))
    (y, cb, cr), ss = utils.yuv_planes(torch.zeros(3 * 4 * 6, dtype=torch.uint8), 1, 1, 4, 6, "yuv444p")
    assert ss == 0 and cb.shape == (1, 1, 4, 6) and cr.storage_offset() == 48
    (y, cb, cr), ss = utils.yuv_planes(torch.zeros(5 * 7 + 2 * 5 * 4, dtype=torch.uint16), 1, 1, 5, 7, "yuv422p", SampleFormat.u16(10))
    assert ss == 1 and cb.shape == (1, 1, 5, 4)
    with pytest.raises(ValueError, match="need"):
        utils.yuv_planes(torch.zeros(10, dtype=torch.uint8), 1, 1, 4, 4, "i420")
    with pytest.raises(ValueError, match="layout"):
        utils.yuv_planes(torch.zeros(100, dtype=torch.uint8), 1, 1, 4, 4, "yuyv")


def test_the_three_entries_are_declared_and_bound():
    names = ("rcb_ycc_to_rgb", "rcb_rgb_to_ycc", "rcb_ycc_sse")
    hdr = open(os.path.join(ROOT, "include", "rcb.h")).read()
    for name in names:
        assert name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert _lib.ABI_VERSION >= 418 and int(re.search(r"#define RCB_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION
    assert len(_lib.PROTOTYPES["rcb_ycc_to_rgb"][1]) == 18 and len(_lib.PROTOTYPES["rcb_rgb_to_ycc"][1]) == 17
    assert len(_lib.PROTOTYPES["rcb_ycc_sse"][1]) == 19
    from recombiner_amd import build
    assert "colour.hip" in build.SOURCES
