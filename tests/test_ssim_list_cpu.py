"""The host side of rcb_ssim_list (N4 415) without a device: the planner against the same arithmetic written here from the header,
the workspace rule, the refusals, and utils.ssim_from_sums / msssim_from_sums with one size per image on sums the evaluator
(tests/ssim_emul.py) produced."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ssim_emul as E

from recombiner_amd import _lib, utils

T, THREADS, TAPS = 16, 256, 11                     # tile edge, outputs per pooling workgroup, window taps (csrc/ssim.hip)
SIDES = [11, 26, 27, 42, 43, 177]
ERR_ARG, ERR_SHAPE = -1, -2


def _cdiv(a, b):
    return -(-a // b)


def _level_elems(H, W, Cc, s):
    """uint32 elements of one operand's block sums at scale s, rounded up to 16 bytes: rcb_ssim_workspace_bytes's rule"""
    return _cdiv((H >> s) * (W >> s) * Cc, 4) * 4


def plan_here(sizes, Cc, scales):
    """the plan of include/rcb.h in Python: rows [scales][n][5] and totals [scales][2]"""
    n = len(sizes)
    rows = np.zeros((scales, n, 5), dtype=np.int64)
    totals = np.zeros((scales, 2), dtype=np.int64)
    ws = 0
    for k, (H, W) in enumerate(sizes):
        for s in range(scales):
            Hs, Ws = H >> s, W >> s
            rows[s, k] = [totals[s, 0], totals[s, 1], ws if s else 0, Hs, Ws]
            totals[s, 0] += _cdiv(Hs - 10, T) * _cdiv(Ws - 10, T)
            if s:
                totals[s, 1] += _cdiv(Hs * Ws * Cc, THREADS)
                ws += 2 * _level_elems(H, W, Cc, s)
    return rows, totals


def _sizes_arg(sizes):
    a = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(-1, 2))
    return a, C.c_void_p(a.ctypes.data)


def plan_lib(sizes, Cc, scales, max_ints=None):
    lib = _lib.load()
    n = len(sizes)
    ints = scales * (5 * n + 2)
    out = np.full(ints + 4, -77, dtype=np.int64)
    keep, arg = _sizes_arg(sizes)
    rc = lib.rcb_ssim_list_plan(n, arg if n else None, Cc, scales, C.c_void_p(out.ctypes.data), ints if max_ints is None else max_ints)
    return rc, out, ints


def _lists():
    """a sweep of lists over SIDES^2: every pair once in one long list, every side squared alone, seeded shuffles of mixed lengths"""
    pairs = list(itertools.product(SIDES, SIDES))
    out = [pairs, [(s, s) for s in SIDES]] + [[p] for p in pairs[::5]]
    out += [[p for p in pairs if min(p) >= 22], [(177, 177)] * 3]                       # lists that allow two and five scales
    rng = np.random.default_rng(415)
    for n in (2, 3, 7, 19):
        out.append([pairs[i] for i in rng.integers(0, len(pairs), n)])
    return out


def _max_scales(sizes):
    return max(s for s in range(1, 6) if min(min(h, w) for h, w in sizes) >> (s - 1) >= TAPS)


def test_plan_against_the_arithmetic():
    lib = _lib.load()
    seen = set()
    for sizes in _lists():
        for Cc in (1, 3):
            for scales in (1, 2, 5):
                if scales > _max_scales(sizes):
                    rc, out, _ = plan_lib(sizes, Cc, scales)
                    assert rc == ERR_SHAPE and np.all(out == -77)
                    continue
                seen.add(scales)
                n = len(sizes)
                rc, out, ints = plan_lib(sizes, Cc, scales)
                assert rc == ints and np.all(out[ints:] == -77)
                rows, totals = out[:5 * scales * n].reshape(scales, n, 5), out[5 * scales * n:ints].reshape(scales, 2)
                want_rows, want_totals = plan_here(sizes, Cc, scales)
                assert np.array_equal(rows, want_rows) and np.array_equal(totals, want_totals)
                for s in range(scales):
                    for col in (0, 1) if s else (0,):
                        per = [(_cdiv((h >> s) - 10, T) * _cdiv((w >> s) - 10, T)) if col == 0 else _cdiv((h >> s) * (w >> s) * Cc, THREADS)
                               for h, w in sizes]
                        # exclusive, monotone, closed by the total
                        assert rows[s, 0, col] == 0 and np.all(np.diff(rows[s, :, col]) == per[:-1])
                        assert np.all(np.diff(rows[s, :, col]) > 0) and rows[s, -1, col] + per[-1] == totals[s, col]
                    assert np.array_equal(rows[s, :, 3], [h >> s for h, _ in sizes]) and np.array_equal(rows[s, :, 4], [w >> s for _, w in sizes])
                # workspace: 16-byte aligned blocks of both operands, pairwise disjoint, inside the size the library asks for
                keep, arg = _sizes_arg(sizes)
                need = lib.rcb_ssim_list_workspace_bytes(n, arg, Cc, scales)
                assert need == sum(lib.rcb_ssim_workspace_bytes(1, h, w, Cc, scales) for h, w in sizes)
                spans = []
                for s in range(1, scales):
                    for k, (h, w) in enumerate(sizes):
                        le = _level_elems(h, w, Cc, s)
                        off = int(rows[s, k, 2])
                        assert off % 4 == 0 and le % 4 == 0
                        spans += [(off, off + (h >> s) * (w >> s) * Cc), (off + le, off + le + (h >> s) * (w >> s) * Cc)]
                spans.sort()
                assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
                assert not spans or (spans[0][0] == 0 and spans[-1][1] * 4 <= need)
                assert (need == 0) == (scales == 1)
                # image k's block is laid out as rcb_ssim lays out one image: offsets relative to the block's start
                if scales > 1:
                    start = 0
                    for k, (h, w) in enumerate(sizes):
                        rel, cur = [int(rows[s, k, 2]) - start for s in range(1, scales)], 0
                        for s in range(1, scales):
                            assert rel[s - 1] == cur
                            cur += 2 * _level_elems(h, w, Cc, s)
                        assert cur * 4 == lib.rcb_ssim_workspace_bytes(1, h, w, Cc, scales)
                        start += cur
    assert seen == {1, 2, 5}


def test_table_bytes_and_the_empty_list():
    lib = _lib.load()
    assert lib.rcb_ssim_list_table_bytes(0, 1) >= 0 and lib.rcb_ssim_list_table_bytes(-1, 1) == -1
    assert lib.rcb_ssim_list_table_bytes(3, 0) == -1 and lib.rcb_ssim_list_table_bytes(3, 6) == -1
    sizes = [lib.rcb_ssim_list_table_bytes(n, 2) for n in range(1, 6)]
    assert all(v % 8 == 0 for v in sizes) and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert lib.rcb_ssim_list_table_bytes(4, 5) > lib.rcb_ssim_list_table_bytes(4, 1)
    rc, out, ints = plan_lib([], 3, 2)
    assert rc == ints == 4 and np.all(out[:4] == 0)
    assert lib.rcb_ssim_list_workspace_bytes(0, None, 3, 2) == 0


def test_refusals():
    lib = _lib.load()
    good = [(26, 27), (43, 42)]
    rc, out, ints = plan_lib(good, 3, 2)
    assert rc == ints
    cases = [([(26, 27), (10, 40)], 3, 1, ERR_SHAPE, "image 1"),          # an image under 11
             ([(40, 10)], 3, 1, ERR_SHAPE, "image 0"),
             ([(177, 177), (26, 177)], 1, 5, ERR_SHAPE, "image 1"),       # more scales than the smallest image allows
             ([(43, 43), (21, 40)], 1, 2, ERR_SHAPE, "image 1"),
             (good, 33, 1, ERR_SHAPE, "channels"), (good, 0, 1, ERR_SHAPE, "channels"),
             (good, 3, 0, ERR_ARG, "scales"), (good, 3, 6, ERR_ARG, "scales")]
    for sizes, Cc, scales, code, word in cases:
        rc, out, _ = plan_lib(sizes, Cc, scales)
        assert rc == code and np.all(out == -77), (sizes, Cc, scales, rc)
        assert word in lib.rcb_last_error_string().decode(), lib.rcb_last_error_string()
        keep, arg = _sizes_arg(sizes)
        assert lib.rcb_ssim_list_workspace_bytes(len(sizes), arg, Cc, scales) == -1
    # null sizes, a null or short plan, a negative count
    out = np.full(64, -77, dtype=np.int64)
    assert lib.rcb_ssim_list_plan(2, None, 3, 1, C.c_void_p(out.ctypes.data), 64) == ERR_ARG and np.all(out == -77)
    assert "sizes" in lib.rcb_last_error_string().decode()
    assert lib.rcb_ssim_list_workspace_bytes(2, None, 3, 1) == -1
    keep, arg = _sizes_arg(good)
    assert lib.rcb_ssim_list_plan(2, arg, 3, 2, None, 64) == ERR_SHAPE
    rc, out, ints = plan_lib(good, 3, 2, max_ints=2 * (5 * 2 + 2) - 1)
    assert rc == ERR_SHAPE and np.all(out == -77)
    assert lib.rcb_ssim_list_plan(-1, arg, 3, 2, C.c_void_p(out.ctypes.data), 64) == ERR_SHAPE


def _cases():
    rng = np.random.default_rng(7)
    out = []
    for H, W in ((27, 43), (11, 30), (43, 27)):
        a = rng.integers(0, 256, (H, W, 2))
        b = np.clip(a + rng.integers(-9, 10, (H, W, 2)), 0, 255)
        out.append((a, b))
    return out


def test_figures_from_sums_with_one_size_per_image():
    cases = _cases()
    per = [E.sums(a, b, 255, 1) for a, b in cases]
    sums = np.asarray(per, dtype=np.int64)
    Hs, Ws = [a.shape[0] for a, _ in cases], [a.shape[1] for a, _ in cases]
    want = [E.ssim_figure(s, h, w) for s, h, w in zip(per, Hs, Ws)]
    got = utils.ssim_from_sums(sums, Hs, Ws)
    assert got.dtype == np.float64 and got.tolist() == want
    assert utils.ssim_from_sums(sums, np.asarray(Hs), tuple(Ws)).tolist() == want
    # scalars are what they were: one size for every image
    assert utils.ssim_from_sums(sums[:1], 27, 43).tolist() == want[:1]
    assert utils.ssim_from_sums(sums[[0, 0]], 27, 43).tolist() == [want[0]] * 2
    assert utils.ssim_from_sums(sums, 27, Ws)[0] == want[0]                 # a scalar beside a sequence
    with pytest.raises(ValueError, match="values of"):
        utils.ssim_from_sums(sums, Hs[:2], Ws)
    with pytest.raises(ValueError, match="scales"):
        utils.ssim_from_sums(sums, [27, 10, 43], Ws)


def test_msssim_from_sums_with_one_size_per_image():
    yy, xx = np.meshgrid(np.arange(191), np.arange(191), indexing="ij")
    base = np.rint(127.5 + 100.0 * np.sin(yy / 9.0) * np.cos(xx / 7.0)).astype(np.int64)
    rng = np.random.default_rng(3)
    per, shapes = [], [(176, 191), (177, 176)]
    for H, W in shapes:
        a = base[:H, :W, None]
        b = np.clip(a + rng.integers(-6, 7, a.shape), 0, 255)
        per.append(E.sums(a, b, 255, 5))
    sums = np.asarray(per, dtype=np.int64)
    Hs, Ws = [s[0] for s in shapes], [s[1] for s in shapes]
    want = [E.msssim_figure(s, h, w) for s, (h, w) in zip(per, shapes)]
    assert utils.msssim_from_sums(sums, Hs, Ws).tolist() == want and 0.0 < want[0] < 1.0
    assert utils.ssim_from_sums(sums, Hs, Ws).tolist() == [E.ssim_figure(s, h, w) for s, (h, w) in zip(per, shapes)]
    assert utils.msssim_from_sums(sums[1:], 177, 176).tolist() == want[1:]
    with pytest.raises(ValueError, match="scales"):
        utils.msssim_from_sums(sums, [176, 175], Ws)
