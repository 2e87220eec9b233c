"""CPU premises of the mixed-size batches (N4 413): the per-signal evaluator (tests/ragged_emul.py) against np.pad and slicing, the
bucket plan (utils.ragged_plan) on the golden geometries, bitstream version 4, and the metric from per-signal element counts."""
import struct
import zlib

import numpy as np
import pytest

import ragged_emul as R
import recon_emul as E
import sample16_emul as Q
import signal_emul as S
from golden_util import cfg_of, load
from test_extent_emul_cpu import _levels, _v1_bytes

from recombiner_amd import bitstream, config, utils
from recombiner_amd.utils import SampleFormat

PN, PS, C = (2, 3), (4, 4), 3
SIZES = [(8, 12), (7, 11), (5, 4), (1, 1), (8, 1)]


def _signals(fmt, seed=3):
    rng = np.random.RandomState(seed)
    dt = Q.np_dtype(fmt)
    if fmt[0] == 1:
        return [rng.rand(*s, C).astype(np.float32) for s in SIZES]
    lo, hi = (-32768, 32768) if fmt[0] == 3 else (0, 256 if fmt[0] == 0 else Q.m_of(fmt) + 1)
    return [rng.randint(lo, hi, size=(*s, C)).astype(dt) for s in SIZES]


# ---- the evaluator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [Q.U8, Q.F32FMT, Q.u16(12), Q.S16])
def test_targets_are_the_edge_padded_signals_cut_per_signal(fmt):
    sigs = _signals(fmt)
    y = R.targets(sigs, PN, PS, fmt)
    per, P = int(np.prod(PN)), int(np.prod(PS))
    assert y.shape == (len(sigs) * per, P, C) and y.dtype == np.float32
    G = tuple(a * b for a, b in zip(PN, PS))
    for k, (sig, size) in enumerate(zip(sigs, SIZES)):
        padded = np.pad(sig, [(0, G[0] - size[0]), (0, G[1] - size[1]), (0, 0)], mode="edge")
        whole = E.stitch(y[k * per:(k + 1) * per], PN, PS)[0]
        assert np.array_equal(S.bits(whole), S.bits(Q.to_target(padded, fmt)))


@pytest.mark.parametrize("fmt", [Q.U8, Q.u16(9), Q.S16])
def test_finish_crops_and_transposes_per_signal(fmt):
    rng = np.random.RandomState(4)
    per, P, n = int(np.prod(PN)), int(np.prod(PS)), len(SIZES)
    y = rng.rand(n * per, P, C).astype(np.float32)
    t = rng.rand(n * per, P, C).astype(np.float32)
    swaps = [False, True, False, True, False]
    out = R.finish(y, t, PN, PS, fmt, SIZES, swaps)
    for k, size in enumerate(SIZES):
        rows = slice(k * per, (k + 1) * per)
        q, v = Q.finish(E.stitch(y[rows], PN, PS)[0][:size[0], :size[1]], fmt)
        tt = E.stitch(t[rows], PN, PS)[0][:size[0], :size[1]]
        if swaps[k]:
            q, v = q.transpose(1, 0, 2), v.transpose(1, 0, 2)
        assert out["q"][k].shape == ((size[1], size[0], C) if swaps[k] else (*size, C)) and out["q"][k].flags["C_CONTIGUOUS"]
        assert np.array_equal(out["q"][k], q) and np.array_equal(S.bits(out["whole"][k]), S.bits(np.ascontiguousarray(v)))
        direct = ((tt.astype(np.float32) - (v.transpose(1, 0, 2) if swaps[k] else v)).astype(np.float64) ** 2).sum()
        assert abs(out["sse"][k] - direct) <= 1e-12 * max(direct, 1.0) and out["n_bad"][k] == 0
    # a NaN in one signal's padding changes nothing; inside its extent only that signal's figures
    y2 = E.stitch(y.copy(), PN, PS)
    y2[1, 7, 11] = np.nan                                     # signal 1 is (7, 11): position (7, 11) is padding
    back = R.finish(S.patch(y2, PN, PS), t, PN, PS, fmt, SIZES, swaps)
    assert np.array_equal(back["sse"], out["sse"]) and not back["n_bad"].any()
    y2[1, 6, 10] = np.nan
    bad = R.finish(S.patch(y2, PN, PS), t, PN, PS, fmt, SIZES, swaps)
    assert np.isnan(bad["sse"][1]) and bad["n_bad"][1] == C and np.array_equal(np.delete(bad["sse"], 1), np.delete(out["sse"], 1))


# ---- the plan -----------------------------------------------------------------------------------------------------------------
def test_ragged_plan_on_the_golden_geometries():
    p2 = cfg_of(load("test_patch2d.npz"))
    swaps, buckets = utils.ragged_plan(p2, [(40, 70), (70, 40), (64, 100)])
    assert swaps == [False, True, False] and len(buckets) == 1
    assert buckets[0]["patch_nums"] == [2, 4] and buckets[0]["indices"] == [0, 1, 2]
    assert buckets[0]["sizes"] == [(40, 70), (40, 70), (64, 100)] and buckets[0]["config"]["patch_nums"][:2] == [2, 4]
    swaps, buckets = utils.ragged_plan(p2, [(40, 70), (30, 60), (70, 40), (64, 100)])
    assert swaps == [False, False, True, False]
    assert [b["patch_nums"] for b in buckets] == [[2, 4], [1, 2]] and [b["indices"] for b in buckets] == [[0, 2, 3], [1]]
    swaps, buckets = utils.ragged_plan(p2, [(70, 40)], landscape=False)
    assert swaps == [False] and buckets[0]["patch_nums"] == [3, 2] and buckets[0]["sizes"] == [(70, 40)]
    p1 = cfg_of(load("test_patch1d.npz"))
    swaps, buckets = utils.ragged_plan(p1, [(410,), (300,), (500,), (640,)])
    assert swaps == [False] * 4
    assert [b["patch_nums"] for b in buckets] == [[4], [2]] and [b["indices"] for b in buckets] == [[0, 2, 3], [1]]
    cif = config.configs["cifar"]
    swaps, buckets = utils.ragged_plan(cif, [(28, 30), (32, 32), (31, 17)])
    assert swaps == [False, False, True] and len(buckets) == 1 and buckets[0]["indices"] == [0, 1, 2]
    assert buckets[0]["sizes"] == [(28, 30), (32, 32), (17, 31)] and buckets[0]["config"] == cif
    with pytest.raises(ValueError):
        utils.ragged_plan(cif, [(28, 30), (33, 32)], landscape=False)
    with pytest.raises(ValueError):
        utils.ragged_plan(cif, [(28, 30, 2)])


# ---- bitstream version 4 --------------------------------------------------------------------------------------------------------
EXT, SW = [(40, 70), (40, 70), (64, 100)], [False, True, False]


def _v4(levels=None, fmt=SampleFormat.u8()):
    return bitstream.pack_indices(_levels() if levels is None else levels, extents=EXT, swaps=SW, sample_format=fmt)


def _resealed(b):
    return b[:-4] + struct.pack("<I", zlib.crc32(b[:-4]) & 0xFFFFFFFF)


@pytest.mark.parametrize("fmt", [SampleFormat.u8(), SampleFormat.f32(), SampleFormat.u16(12), SampleFormat.s16()])
def test_version_4_round_trip(fmt):
    levels = _levels()
    blob = _v4(levels, fmt)
    off = 8 + 8 * 3
    assert struct.unpack_from("<H", blob, 4)[0] == 4 and len(blob) == len(_v1_bytes(levels)) + 5 + 3 * 9 + 2
    assert struct.unpack_from("<BI", blob, off) == (2, 3)
    assert struct.unpack_from("<IIB", blob, off + 5 + 9) == (40, 70, 1) and blob[off + 5 + 27:off + 5 + 29] == bytes([fmt.kind, fmt.depth])
    assert struct.unpack_from("<I", blob, len(blob) - 4)[0] == zlib.crc32(blob[:-4]) & 0xFFFFFFFF      # from the magic on
    assert bitstream.unpack_header(blob) == dict(version=4, extent=None, sample_format=fmt, extents=EXT, swaps=SW)
    got, ext = bitstream.unpack(blob)
    assert ext is None and all(np.array_equal(a, b) and a.dtype == np.int64 for a, b in zip(got, levels))
    assert bitstream.payload_bits(blob) == sum(a.size for a in levels) * 16
    one = bitstream.pack_indices(levels[:1], extents=[(410,), (500,)], sample_format=fmt)                 # 1-D, no swaps given
    assert bitstream.unpack_header(one)["extents"] == [(410,), (500,)] and bitstream.unpack_header(one)["swaps"] == [False, False]


def test_malformed_version_4_streams_are_rejected():
    levels = _levels()
    blob = _v4(levels)
    off = 8 + 8 * 3
    head_end = off + 5 + 27 + 2
    for at in range(4, head_end):                              # every flipped header, size, flag or format byte
        bad = bytearray(blob)
        bad[at] ^= 0x01
        with pytest.raises(ValueError):
            bitstream.unpack(bytes(bad))
    bad = bytearray(blob)
    bad[head_end] ^= 0x80                                      # a flipped payload byte
    with pytest.raises(ValueError, match="checksum"):
        bitstream.unpack(bytes(bad))
    for cut in list(range(off, head_end + 1)) + [len(blob) - 1, len(blob) - 5]:
        with pytest.raises(ValueError):
            bitstream.unpack(blob[:cut])
    with pytest.raises(ValueError):
        bitstream.unpack(blob + b"\0")
    flag_at = off + 5 + 8
    for flags in (2, 3, 0x80, 0xFF):                           # a reserved flag bit, with a checksum that matches
        with pytest.raises(ValueError, match="flags"):
            bitstream.unpack(_resealed(blob[:flag_at] + bytes([flags]) + blob[flag_at + 1:]))
    with pytest.raises(ValueError, match="empty axis"):
        bitstream.unpack(_resealed(blob[:off + 5] + struct.pack("<I", 0) + blob[off + 9:]))
    with pytest.raises(ValueError):                            # no signals (the rest of the block cut out to keep the length right)
        bitstream.unpack(_resealed(blob[:off + 1] + struct.pack("<I", 0) + blob[off + 5 + 27:]))
    one_d = bitstream.pack_indices(levels, extents=[(410,)], sample_format=SampleFormat.f32())
    with pytest.raises(ValueError, match="flags"):             # the swap is 2-D only
        bitstream.unpack(_resealed(one_d[:off + 9] + b"\x01" + one_d[off + 10:]))
    for kw in (dict(extents=[]), dict(extents=[(1, 2), (3,)]), dict(extents=[(0, 4)]), dict(extents=[(1, 2, 3, 4)]),
               dict(extents=[(410,)], swaps=[True]), dict(extents=[(4, 4)], swaps=[True, False]), dict(extents=[(4, 4)], extent=(4, 4))):
        with pytest.raises(ValueError):
            bitstream.pack_indices(levels, sample_format=SampleFormat.u8(), **kw)
    with pytest.raises(ValueError):                            # version 4 always carries a format
        bitstream.pack_indices(levels, extents=[(4, 4)])


def test_relabelled_versions_are_rejected_and_versions_1_to_3_are_unchanged():
    levels = _levels()
    v1 = bitstream.pack_indices(levels)
    v2 = bitstream.pack_indices(levels, extent=(375, 500))
    v3 = bitstream.pack_indices(levels, extent=(375, 500), sample_format=SampleFormat.u16(12))
    v3n = bitstream.pack_indices(levels, sample_format=SampleFormat.s16())
    v4 = _v4(levels)
    assert v1 == _v1_bytes(levels)
    off = 8 + 8 * 3
    ext = struct.pack("<BII", 2, 375, 500)
    body = v1[off:-4]
    assert v2 == v1[:4] + struct.pack("<H", 2) + v1[6:off] + ext + body + struct.pack("<I", zlib.crc32(ext + body) & 0xFFFFFFFF)
    ext3 = ext + bytes([2, 12])
    assert v3 == v1[:4] + struct.pack("<H", 3) + v1[6:off] + ext3 + body + struct.pack("<I", zlib.crc32(ext3 + body) & 0xFFFFFFFF)
    for old in (v1, v2, v3, v3n):
        with pytest.raises(ValueError):
            bitstream.unpack(old[:4] + struct.pack("<H", 4) + old[6:])
    for v in (1, 2, 3, 5):
        with pytest.raises(ValueError):
            bitstream.unpack(v4[:4] + struct.pack("<H", v) + v4[6:])
    # a one-signal 1-D version-4 stream is as long as a version-3 stream of one axis less 4 bytes: no length coincides with 1 .. 3
    for n_sig, nd in ((1, 1), (1, 2), (2, 1), (1, 3)):
        b4 = bitstream.pack_indices(levels, extents=[(5,) * nd] * n_sig, sample_format=SampleFormat.u8())
        for v in (1, 2, 3):
            with pytest.raises(ValueError):
                bitstream.unpack(b4[:4] + struct.pack("<H", v) + b4[6:])


def test_the_older_decoders_name_the_list_decoder():
    blob = _v4(_levels()[:1])
    with pytest.raises(ValueError, match="decode_signal_list"):
        bitstream.decode_signal(config.configs["kodak"], "kodak", None, blob, None, 8)
    with pytest.raises(ValueError, match="decode_signal_list"):
        bitstream.decode_signal_any(config.configs["kodak"], "kodak", None, blob)
    with pytest.raises(ValueError, match="decode_signal"):     # and the list decoder the older ones
        bitstream.decode_signal_list(config.configs["kodak"], "kodak", None, bitstream.pack_indices(_levels()[:1], extent=(28, 30)))
    p2 = cfg_of(load("test_patch2d.npz"))
    two = bitstream.pack_indices(_levels(), extents=[(40, 70), (30, 60)], sample_format=SampleFormat.u8())
    with pytest.raises(ValueError, match="one grid"):          # before it touches the checkpoint or the device
        bitstream.decode_signal_list(p2, "kodak", None, two)
    with pytest.raises(ValueError, match="patches each"):      # 8 rows, 3 signals of 8 patches
        bitstream.decode_signal_list(p2, "kodak", None, _v4())
    with pytest.raises(ValueError, match="integer form"):
        bitstream.decode_signal_list(p2, "kodak", None, _v4(fmt=SampleFormat.f32()), as_integer=True)


# ---- the metric from per-signal counts -------------------------------------------------------------------------------------------
def test_metric_from_sse_with_count_arrays():
    rng = np.random.RandomState(8)
    counts = np.array([28 * 30 * 3, 32 * 32 * 3, 31 * 17 * 3])
    errs = [rng.rand(c) * 0.1 for c in counts]
    sse = np.array([np.sum(e.astype(np.float64) ** 2) for e in errs])
    per = utils.metric_from_sse(sse, counts, "cifar")
    assert per.shape == (3,) and np.allclose(per, [-10 * np.log10(np.mean(e ** 2)) for e in errs], rtol=0, atol=1e-12)
    rm = utils.metric_from_sse(sse, counts, "protein")
    assert np.allclose(rm, [25 * np.sqrt(3 * np.mean(e ** 2)) for e in errs], rtol=1e-14, atol=0)
    for ds in ("kodak", "video", "audio"):
        pooled = utils.metric_from_sse(sse, counts, ds)
        assert isinstance(pooled, float) and abs(pooled + 10 * np.log10(np.mean(np.concatenate(errs) ** 2))) <= 1e-12
    # equal counts: the scalar form's figures; the scalar form itself is unchanged
    same = np.full(3, 100)
    assert np.array_equal(utils.metric_from_sse(sse, same, "cifar"), utils.metric_from_sse(sse, 100, "cifar"))
    assert abs(utils.metric_from_sse(sse, same, "kodak") - utils.metric_from_sse(sse, 100, "kodak")) <= 1e-12
    assert utils.metric_from_sse(sse, 100, "kodak") == (-10.0 * np.log10(sse.sum() / (100.0 * 3))).item()
    with pytest.raises(ValueError):
        utils.metric_from_sse(sse, counts[:2], "cifar")


# ---- the stream format did not move ----------------------------------------------------------------------------------------------
def test_bitstream_bytes_and_outcomes_match_the_recorded_ones():
    """tools/bitstream_digests.py: the bytes pack_indices writes for versions 1 to 4, and what unpack, unpack_header and payload_bits
    make of one stream per version intact, with any single byte changed and cut at any length -- the value or the ValueError's
    text -- against tests/golden/bitstream_outcomes.json, which was recorded before the container code was rewritten"""
    import importlib.util
    import json
    import os
    from golden_util import GOLDEN, ROOT
    spec = importlib.util.spec_from_file_location("bitstream_digests", os.path.join(ROOT, "tools", "bitstream_digests.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(GOLDEN, "bitstream_outcomes.json")) as f:
        recorded = json.load(f)
    got = dict(tool.lines(bitstream, SampleFormat))
    assert sorted(got) == sorted(recorded)
    assert {k: v for k, v in got.items() if recorded[k] != v} == {}
