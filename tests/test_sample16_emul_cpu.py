"""The premises of tests/sample16_emul.py (the numpy evaluator of the 16-bit sample formats of include/rcb.h, N4 412), exhaustively and
without a GPU: the s16 normalisation is the reference's formula bit for bit, the round trip holds for every representable value, exact
ties exist and round to even, the ends of the range and the non-finite inputs give the stated q and v, and a few mutants of the
evaluator are caught by these very checks.  Then the host side of the feature: bitstream version 3 and utils.SampleFormat."""
import struct
import zlib

import numpy as np
import pytest
import torch

import sample16_emul as Q
import signal_emul as S
from test_extent_emul_cpu import _levels, _v1_bytes

from recombiner_amd import bitstream, config
from recombiner_amd.utils import SampleFormat

F32 = np.float32
DEPTHS = list(range(9, 17))
FORMATS = [Q.u16(b) for b in DEPTHS] + [Q.S16]
ALL_U16 = np.arange(65536, dtype=np.uint16)
ALL_S16 = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)


def every_value(fmt):
    return ALL_S16 if fmt == Q.S16 else np.arange(Q.m_of(fmt) + 1, dtype=np.uint16)


# ---- the evaluator under test, and mutants of it ----------------------------------------------------------------------------------
def finish_trunc(x, fmt):
    """mutant: truncation instead of rint"""
    c = Q.clip01(x)
    if fmt[0] == 2:
        M = F32(Q.m_of(fmt))
        qi = np.trunc(c * M).astype(np.int64)
        return qi.astype(np.uint16), qi.astype(F32) / M
    u = np.minimum(np.trunc(c * F32(65536)), F32(65535))
    return (u.astype(np.int64) - 32768).astype(np.int16), u / F32(65536)


def finish_pow2(x, fmt):
    """mutant: M = 2^b (u16 only)"""
    c = Q.clip01(x)
    M = F32(1 << fmt[1])
    qi = np.rint(c * M).astype(np.int64)
    return qi.astype(np.uint16), qi.astype(F32) / M


def to_target_pow2(q, fmt):
    return np.asarray(q).astype(F32) / F32(1 << fmt[1])


def finish_no_clamp(x, fmt):
    """mutant: s16 without the clamp at 65535"""
    u = np.rint(Q.clip01(x) * F32(65536))
    return (u.astype(np.int64) - 32768).astype(np.int16), u / F32(65536)


def finish_float_q(x, fmt):
    """mutant: v taken from the float q (u16): keeps the sign of a negative zero"""
    c = Q.clip01(x)
    c = np.where(c == 0, np.copysign(c, np.asarray(x, dtype=F32)), c).astype(F32)     # (a maximum that keeps the sign of its zero)
    M = F32(Q.m_of(fmt))
    q = np.rint(c * M)
    return q.astype(np.int64).astype(np.uint16), q / M


# ---- the checks, each a function of (to_target, finish) so that the mutants can be put through them ---------------------------------
def check_round_trip(fmt, to_target=Q.to_target, finish=Q.finish):
    q = every_value(fmt)
    back, v = finish(to_target(q, fmt), fmt)
    return back.dtype == q.dtype and np.array_equal(back, q) and np.array_equal(S.bits(v), S.bits(Q.to_target(q, fmt)))


def check_ties(fmt, finish=Q.finish):
    x, k = Q.tie_inputs(fmt)
    even = k + (k & 1)                                          # the even neighbour of k + 1/2
    bias = 32768 if fmt == Q.S16 else 0
    q, _ = finish(x, fmt)
    return len(x) > 50 and (k & 1).any() and (~k & 1).any() and np.array_equal(q.astype(np.int64) + bias, even)


def check_ends(fmt, finish=Q.finish):
    M = Q.m_of(fmt) if fmt[0] == 2 else 65535
    bias = 32768 if fmt == Q.S16 else 0
    one = F32(1)
    x = np.array([0.0, -0.0, 1.0, np.nextafter(one, F32(2)), np.nextafter(F32(0), F32(-1)), np.inf, -np.inf, np.nan, 1e-40, -1e-40,
                  -3.5, 7.0], dtype=F32)
    want_q = np.array([0, 0, M, M, 0, M, 0, 0, 0, 0, 0, M], dtype=np.int64)
    q, v = finish(x, fmt)
    top = F32(M) / F32(M if fmt[0] == 2 else 65536)
    want_v = np.where(want_q == 0, F32(0), top).astype(F32)
    return np.array_equal(q.astype(np.int64) + bias, want_q) and np.array_equal(S.bits(v), S.bits(want_v))   # (+0.0: its bits)


# ---- premises ------------------------------------------------------------------------------------------------------------------------
def test_s16_in_is_the_reference_formula_for_all_65536_values():
    """data/audio.py:50-54 forms (q / 32768 + 1) / 2 on float32 tensors; the header's ((float)q + 32768) / 65536 has the same bits"""
    q = ALL_S16
    ref = (q.astype(F32) / F32(32768) + F32(1)) / F32(2)
    got = Q.to_target(q, Q.S16)
    assert ref.dtype == got.dtype == F32 and np.array_equal(S.bits(got), S.bits(ref))
    assert got.min() == 0 and got.max() == F32(65535) / F32(65536) and len(np.unique(got)) == 65536
    assert torch.equal((torch.from_numpy(q).float() / 32768 + 1) / 2, torch.from_numpy(got))


@pytest.mark.parametrize("fmt", FORMATS)
def test_round_trip_of_every_value(fmt):
    assert check_round_trip(fmt)
    y = Q.to_target(every_value(fmt), fmt)
    assert y.min() == 0 and (y.max() == 1 if fmt[0] == 2 else y.max() < 1) and (np.diff(y) > 0).all()


@pytest.mark.parametrize("depth", DEPTHS)
def test_u16_values_above_m_are_not_clamped(depth):
    fmt = Q.u16(depth)
    y = Q.to_target(ALL_U16, fmt)
    M = Q.m_of(fmt)
    assert np.array_equal(S.bits(y), S.bits(ALL_U16.astype(F32) / F32(M)))
    assert (y[M + 1:] > 1).all() and y[M] == 1


@pytest.mark.parametrize("fmt", FORMATS)
def test_exact_ties_exist_and_round_to_even(fmt):
    x, k = Q.tie_inputs(fmt)
    scale = F32(Q.m_of(fmt)) if fmt[0] == 2 else F32(65536)
    assert np.array_equal((x * scale).astype(np.float64), k + 0.5)
    assert check_ties(fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_ends_of_the_range_and_non_finite_inputs(fmt):
    assert check_ends(fmt)
    q, v = Q.finish(np.array([-0.0, -1e-30], dtype=F32), fmt)
    assert not np.signbit(v).any()                              # q = 0 gives +0.0 whatever the sign of x
    q8, v8 = Q.finish(np.array([0.25], dtype=F32), Q.U8)        # the older kinds go to the older evaluators
    assert q8.dtype == np.uint8 and q8[0] == 64 and v8[0] == F32(64) / F32(255)
    qf, vf = Q.finish(np.array([3.5, np.nan], dtype=F32), Q.F32FMT)
    assert qf is None and vf[0] == F32(3.5) and np.isnan(vf[1])


def test_mutants_of_the_evaluator_are_caught():
    for fmt in (Q.u16(9), Q.u16(12), Q.u16(16), Q.S16):
        assert not check_ties(fmt, finish_trunc), fmt                                   # truncation instead of rintf
    for fmt in (Q.u16(9), Q.u16(10), Q.u16(16)):
        assert not check_ends(fmt, finish_pow2), fmt                                    # M = 2^b
        assert not check_round_trip(fmt, to_target_pow2, Q.finish), fmt                 # (on either side alone)
        assert not check_ends(fmt, finish_float_q), fmt                                 # v from the float q: -0.0
        assert check_round_trip(fmt, finish=finish_float_q)                             # (which only the sign of zero shows)
    assert not check_ends(Q.S16, finish_no_clamp)                                       # a missing 65535 clamp
    assert check_round_trip(Q.S16, finish=finish_no_clamp)                              # (no in(q) reaches 1: only x = 1 does)


def test_padded_and_cropped_forms_compose_the_older_evaluators():
    """targets(pad) = the format's arithmetic on extent_emul's edge-padded patches; finish_whole(size) crops like finish_crop and, for
    the u8 format, gives its every array"""
    import extent_emul as X
    pn, ps, Cc, _ = X.CASES["2d"]
    size = (7, 11)
    rng = np.random.RandomState(3)
    q = rng.randint(0, 4096, size=(2, *size, Cc)).astype(np.uint16)
    y = Q.targets(q, pn, ps, Q.u16(12), pad=True)
    assert np.array_equal(S.bits(y), S.bits(S.patch(X.pad_edge(q, pn, ps), pn, ps).astype(F32) / F32(4095)))
    got = Q.finish_whole(y, y, pn, ps, Q.u16(12), size=size)
    assert got["q"].dtype == np.uint16 and np.array_equal(got["q"], q) and (got["sse"] == 0).all() and (got["n_bad"] == 0).all()
    x = rng.uniform(-0.2, 1.2, size=y.shape).astype(F32)
    a, b = Q.finish_whole(x, y, pn, ps, Q.U8, size=size), X.finish_crop(x, y, pn, ps, size, mode=0)
    assert np.array_equal(a["q"], b["u8"]) and np.array_equal(S.bits(a["whole"]), S.bits(b["whole"]))
    assert np.array_equal(a["sse"], b["sse"]) and np.array_equal(a["terms"], b["terms"]) and np.array_equal(a["n_bad"], b["n_bad"])


# ---- utils.SampleFormat ----------------------------------------------------------------------------------------------------------------
def test_sample_format_validation():
    assert SampleFormat.u8().dtype == torch.uint8 and SampleFormat.f32().dtype == torch.float32
    assert SampleFormat.u16(12).dtype == torch.uint16 and SampleFormat.s16().dtype == torch.int16
    assert (SampleFormat.u16(12).kind, SampleFormat.u16(12).depth) == (2, 12) and (SampleFormat.s16().kind, SampleFormat.s16().depth) == (3, 0)
    assert SampleFormat.u16(10) == SampleFormat(2, 10) != SampleFormat.u16(12) and SampleFormat.s16() != SampleFormat.u16(16)
    assert len({SampleFormat.u8(), SampleFormat.u8(), SampleFormat.f32()}) == 2 and "u16(12)" in repr(SampleFormat.u16(12))
    assert SampleFormat.u16(12).accepts(torch.int16) and SampleFormat.u16(12).accepts(torch.uint16)
    assert not SampleFormat.s16().accepts(torch.uint16) and not SampleFormat.u8().accepts(torch.int16)
    assert SampleFormat.implied("kodak") == SampleFormat.u8() and SampleFormat.implied("audio") == SampleFormat.f32()
    for bad in (lambda: SampleFormat.u16(8), lambda: SampleFormat.u16(17), lambda: SampleFormat.u16(0), lambda: SampleFormat(4),
                lambda: SampleFormat(-1), lambda: SampleFormat(0, 8), lambda: SampleFormat(3, 16), lambda: SampleFormat(1, 1),
                lambda: SampleFormat(2.0, 12), lambda: SampleFormat("u16", 12), lambda: SampleFormat(2, 12.0), lambda: SampleFormat(True)):
        with pytest.raises(ValueError):
            bad()


# ---- bitstream version 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", [(40000,), (375, 500), (30, 100, 130), None])
@pytest.mark.parametrize("fmt", [SampleFormat.u16(9), SampleFormat.u16(12), SampleFormat.u16(16), SampleFormat.s16(), SampleFormat.u8()])
def test_version_3_round_trip(extent, fmt):
    levels = _levels()
    blob = bitstream.pack_indices(levels, extent=extent, sample_format=fmt)
    nd = 0 if extent is None else len(extent)
    assert len(blob) == len(_v1_bytes(levels)) + 1 + 4 * nd + 2 and struct.unpack_from("<H", blob, 4)[0] == 3
    got, ext = bitstream.unpack(blob)
    assert ext == (None if extent is None else tuple(extent))
    assert len(got) == 3 and all(np.array_equal(a, b) and a.dtype == np.int64 for a, b in zip(got, levels))
    assert bitstream.unpack_header(blob) == dict(version=3, extent=ext, sample_format=fmt)
    assert bitstream.payload_bits(blob) == sum(a.size for a in levels) * 16
    # the layout: shapes, u8 nd | nd x u32 size, u8 kind | u8 depth, the payload; the CRC covers both blocks and the payload
    off = 8 + 8 * 3
    assert blob[off] == nd and blob[off + 1 + 4 * nd] == fmt.kind and blob[off + 2 + 4 * nd] == fmt.depth
    assert struct.unpack_from("<I", blob, len(blob) - 4)[0] == zlib.crc32(blob[off:-4]) & 0xFFFFFFFF


def test_versions_1_and_2_are_byte_identical():
    levels = _levels()
    v1, v2 = bitstream.pack_indices(levels), bitstream.pack_indices(levels, extent=(375, 500))
    assert v1 == bitstream.pack_indices(levels, sample_format=None) == _v1_bytes(levels)
    ext = struct.pack("<BII", 2, 375, 500)
    body = v1[8 + 8 * 3:-4]
    assert v2 == v1[:4] + struct.pack("<H", 2) + v1[6:8 + 8 * 3] + ext + body + struct.pack("<I", zlib.crc32(ext + body) & 0xFFFFFFFF)
    assert bitstream.unpack_header(v1) == dict(version=1, extent=None, sample_format=None)
    assert bitstream.unpack_header(v2) == dict(version=2, extent=(375, 500), sample_format=None)

    class Level:
        def __init__(self, a):
            self.idx_groupwise, self.mask_groupwise, self.pre = a, np.ones(a.shape, dtype=bool), ""

    class Model:                                            # what bitstream.encode reads of a TestBNNmodel
        patch = True

        def __init__(self, dataset):
            self.dataset = dataset
            self._l1, self._l2, self._l3 = (Level(a) for a in levels)
    # the preset's implied format writes no version 3
    assert bitstream.encode(Model("kodak"), sample_format=SampleFormat.u8()) == v1 == bitstream.encode(Model("kodak"))
    assert bitstream.encode(Model("audio"), extent=(375, 500), sample_format=SampleFormat.f32()) == v2
    v3 = bitstream.encode(Model("audio"), extent=(40000,), sample_format=SampleFormat.s16())
    assert bitstream.unpack_header(v3) == dict(version=3, extent=(40000,), sample_format=SampleFormat.s16())
    assert bitstream.unpack_header(bitstream.encode(Model("kodak"), sample_format=SampleFormat.u16(10)))["sample_format"] == SampleFormat.u16(10)
    with pytest.raises(ValueError, match="SampleFormat"):
        bitstream.encode(Model("kodak"), sample_format=(2, 12))
    with pytest.raises(ValueError, match="SampleFormat"):
        bitstream.pack_indices(levels, sample_format="u16")


def test_malformed_version_3_streams_are_rejected():
    levels = _levels()
    blob = bitstream.pack_indices(levels, extent=(375, 500), sample_format=SampleFormat.u16(12))
    off = 8 + 8 * 3
    fo = off + 9                                             # the format block
    for cut in (off, off + 1, off + 5, fo, fo + 1, fo + 2, len(blob) - 1, len(blob) - 5):       # truncated anywhere
        with pytest.raises(ValueError):
            bitstream.unpack_header(blob[:cut])
        with pytest.raises(ValueError):
            bitstream.unpack(blob[:cut])

    def resealed(b):
        return b[:-4] + struct.pack("<I", zlib.crc32(b[off:-4]) & 0xFFFFFFFF)
    for kind, depth in ((4, 0), (255, 0), (2, 8), (2, 17), (2, 0), (0, 8), (1, 12), (3, 16)):     # an unknown kind or depth
        with pytest.raises(ValueError, match="unsupported bitstream header"):
            bitstream.unpack(resealed(blob[:fo] + bytes([kind, depth]) + blob[fo + 2:]))
    assert bitstream.unpack_header(resealed(blob[:fo] + bytes([3, 0]) + blob[fo + 2:]))["sample_format"] == SampleFormat.s16()
    for at, bit in ((fo, 0x01), (fo + 1, 0x01), (fo + 1, 0x04)):                           # a flipped format byte that stays valid
        bad = bytearray(blob)
        bad[at] ^= bit
        with pytest.raises(ValueError, match="checksum|unsupported"):
            bitstream.unpack(bytes(bad))
    bad = bytearray(blob)
    bad[fo + 1] = 10                                                                        # u16(12) -> u16(10): only the CRC tells
    with pytest.raises(ValueError, match="checksum"):
        bitstream.unpack_header(bytes(bad))
    with pytest.raises(ValueError, match="axes"):
        bitstream.unpack(resealed(blob[:off] + bytes([4]) + blob[off + 1:]))
    bare = bitstream.pack_indices(levels, sample_format=SampleFormat.s16())
    assert bitstream.unpack(bare)[1] is None
    with pytest.raises(ValueError):                                                         # version 2 allows no empty extent
        bitstream.unpack(bare[:4] + struct.pack("<H", 2) + bare[6:])
    with pytest.raises(ValueError):
        bitstream.unpack(blob[:4] + struct.pack("<H", 4) + blob[6:])                        # an unknown version


def test_decoders_check_the_format_before_they_touch_the_device():
    cfg = config.configs["audio"]
    v3 = bitstream.pack_indices(_levels()[:1], extent=(100,), sample_format=SampleFormat.s16())
    with pytest.raises(ValueError, match="decode_signal_any"):                              # an extent: the cropping decoder's
        bitstream.decode_signal(cfg, "audio", None, v3, None, 8)
    with pytest.raises(ValueError, match="carries"):                                        # the stream and the caller disagree
        bitstream.decode_signal(cfg, "audio", None, v3, None, 8, sample_format=SampleFormat.u16(16))
    v2 = bitstream.pack_indices(_levels()[:1], extent=(100,))
    with pytest.raises(ValueError, match="no 8-bit form"):                                  # as ever, without a format
        bitstream.decode_signal_any(cfg, "audio", None, v2, as_uint8=True)
    with pytest.raises(ValueError, match="no 8-bit form"):
        bitstream.decode_signal_any(cfg, "audio", None, v2, as_integer=True)
    f32 = bitstream.pack_indices(_levels()[:1], extent=(100,), sample_format=SampleFormat.f32())
    with pytest.raises(ValueError, match="no integer form"):
        bitstream.decode_signal_any(config.configs["kodak"], "kodak", None, f32, as_integer=True)


def test_drivers_want_a_format_for_16_bit_tensors():
    from recombiner_amd import drivers
    cfg = config.configs["audio"]
    for dtype in (torch.int16, torch.uint16):
        sig = torch.zeros(1, 100, 1, dtype=dtype)
        for call in (drivers.compress_signals, drivers.compress_signals_any):
            with pytest.raises(ValueError, match="sample_format"):
                call(cfg, "audio", None, sig)
    with pytest.raises(ValueError, match="sample_format"):
        drivers.compress_signals_any(cfg, "audio", None, torch.zeros(1, 100, 1, dtype=torch.uint16), sample_format=SampleFormat.s16())
    with pytest.raises(ValueError, match="sample_format"):
        drivers.compress_signals_any(cfg, "audio", None, torch.zeros(1, 100, 1), sample_format=SampleFormat.u16(12))
