"""rcb_signal_patch (N4: whole signals -> patch targets on the device) against the numpy evaluator tests/signal_emul.py, whose
premises tests/test_signal_emul_cpu.py checks.  Every comparison is bit for bit (fp32 through an int32 view): both source kinds, both
memory paths, strided / offset / broadcast views, guard words around y, the round trip through rcb_recon_finish, refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import signal_emul as S

pytestmark = pytest.mark.gpu

from recombiner_amd import _lib, ops  # noqa: E402
from recombiner_amd._lib import RcbError  # noqa: E402

DEV = "cuda"
F32 = np.float32

# name -> (patch_nums, patch_size, C): the smallest shapes at which each path and each index term can go wrong
SHAPES = {
    "1d_odd_run": ((3,), (5,), 1),                  # run not a multiple of 4
    "2d_run18": ((2, 3), (4, 6), 3),                # run 18: element path
    "2d_run24": ((2, 3), (4, 8), 3),                # run 24: fast path
    "unpatched": ((1, 1), (4, 4), 4),               # patch_nums of ones
    "3d_fast": ((1, 2, 2), (3, 4, 4), 3),           # 3-D, run 12: fast path
    "3d_elem": ((2, 1, 3), (2, 3, 5), 2),           # all three axes and counts differ, run 10: element path
    # a workgroup moves 8192 elements of a signal: just over it, and one quad more, on either path
    "chunk_elem": ((3,), (2731,), 1),               # 8193 elements
    "chunk_elem_q": ((1,), (8197,), 1),             # 8197
    "chunk_fast": ((3,), (2732,), 1),               # 8196 elements, run 2732 = 4 * 683
    "chunk_fast_q": ((2,), (4100,), 1),             # 8200
}
SMALL = ["1d_odd_run", "2d_run18", "2d_run24", "unpatched", "3d_fast", "3d_elem"]
FAST, ELEM = "2d_run24", "2d_run18"
SENTINEL = -12345.5

# NaNs with distinct payloads (quiet and signalling, both signs), +-0, +-inf, denormals, the largest finite value
SPECIAL_BITS = np.array([0x7fc00000, 0x7fc00001, 0x7f800001, 0xffc12345, 0x7fffffff, 0xff800002, 0x7fa5a5a5, 0x00000000, 0x80000000,
                         0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x00400000, 0x7f7fffff], dtype=np.uint32)


def grid(name):
    pn, ps, Cc = SHAPES[name]
    return pn, ps, Cc, tuple(a * b for a, b in zip(pn, ps))


def source(shape, kind, seed):
    """a CPU tensor of `shape`: uint8 holding every byte value (once the shape has 256 elements), or fp32 holding the special bit
    patterns at random places among random values"""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    if kind == "u8":
        a = (np.arange(n) % 256).astype(np.uint8)[rng.permutation(n)]
        assert n < 256 or len(np.unique(a)) == 256
    else:
        a = rng.standard_normal(n).astype(F32)
        m = min(n, len(SPECIAL_BITS))
        a.view(np.uint32)[rng.permutation(n)[:m]] = SPECIAL_BITS[rng.permutation(len(SPECIAL_BITS))[:m]]
    return torch.from_numpy(a.reshape(shape))


def run(view, layout, pad=64):
    """ops.signal_patch into a slice of a sentinel-filled buffer (pad floats before and after: 64 keeps y 16-byte aligned, an odd
    pad does not); the sentinel must be intact around the slice -> y as numpy"""
    per, P = int(np.prod(layout.patch_nums)), int(np.prod(layout.patch_size))
    shape = (view.shape[0] * per, P, view.shape[-1])
    n = int(np.prod(shape))
    buf = torch.full((pad + n + pad,), SENTINEL, device=DEV)
    out = buf[pad:pad + n].view(shape)
    got = ops.signal_patch(view, layout, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:pad] == F32(SENTINEL)).all() and (host[pad + n:] == F32(SENTINEL)).all(), "guard words overwritten"
    return host[pad:pad + n].reshape(shape)


def check(base, make_view, layout, pad=64):
    """base: CPU tensor; make_view: the same view arithmetic applied to the CPU tensor (-> the evaluator, through a zero-copy
    numpy view) and to its device copy (-> the kernel).  -> y"""
    want = S.targets(make_view(base).numpy(), layout.patch_nums, layout.patch_size)
    got = run(make_view(base.to(DEV)), layout, pad)
    assert got.dtype == F32 and got.shape == want.shape
    bad = np.flatnonzero(S.bits(got) != S.bits(want))
    assert bad.size == 0, f"{bad.size} of {want.size} elements differ, first at flat index {bad[:5]}"
    return got


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("n_data", [1, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_contiguous_sources(name, n_data, kind):
    pn, ps, Cc, G = grid(name)
    base = source((n_data, *G, Cc), kind, seed=len(name) + n_data)
    y = check(base, lambda t: t, ops.PeLayout(pn, ps))
    assert y.shape == (n_data * int(np.prod(pn)), int(np.prod(ps)), Cc)
    if kind == "f32":
        assert np.isnan(y).sum() == np.isnan(base.numpy()).sum() > 0


@pytest.mark.parametrize("name", [FAST, ELEM])
def test_every_byte_value(name):
    pn, ps, Cc, G = grid(name)
    base = source((2, *G, Cc), "u8", seed=5)
    assert len(np.unique(base.numpy())) == 256
    y = check(base, lambda t: t, ops.PeLayout(pn, ps))
    assert np.array_equal(np.unique(S.bits(y)), S.bits(S.unit8(np.arange(256, dtype=np.uint8))))


def _views(G, Cc, n):
    """name -> (shape of the base buffer, view arithmetic): each gives [n, *G, C]"""
    G0, G1 = G
    return {
        "channels_first": ((n, Cc, G0, G1), lambda t: t.movedim(1, -1)),
        "transposed": ((n, G1, G0, Cc), lambda t: t.transpose(1, 2)),
        "window_odd": ((n, G0 + 5, G1 + 7, Cc), lambda t: t[:, 3:3 + G0, 5:5 + G1]),
        # origin (2, 4) in rows of 32 pixels: every run start stays a multiple of 4 elements for C = 3
        "window_even": ((n, G0 + 5, 32, Cc), lambda t: t[:, 2:2 + G0, 4:4 + G1]),
        "offset_one": ((n * G0 * G1 * Cc + 1,), lambda t: t[1:].view(n, G0, G1, Cc)),
        "channel_stride0": ((n, G0, G1, 1), lambda t: t.expand(n, G0, G1, Cc)),
        "signal_stride0": ((1, G0, G1, Cc), lambda t: t.expand(n, G0, G1, Cc)),
    }


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("view", ["channels_first", "transposed", "window_odd", "window_even", "offset_one", "channel_stride0",
                                  "signal_stride0"])
@pytest.mark.parametrize("name", [FAST, ELEM])
def test_strided_views(name, view, kind):
    """the strides go to the kernel as they are: nothing is made contiguous on the way"""
    pn, ps, Cc, G = grid(name)
    shape, make = _views(G, Cc, 2)[view]
    base = source(shape, kind, seed=11)
    assert view in ("offset_one", "signal_stride0") or not make(base).is_contiguous()
    check(base, make, ops.PeLayout(pn, ps))


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_misaligned_views_of_a_fast_shape_equal_the_aligned_result(kind):
    """the same signals behind a storage offset of one element, inside a larger buffer at an odd origin, and into a y that is not
    16-byte aligned: the element path must give the bits of the 16-byte path"""
    pn, ps, Cc, G = grid(FAST)
    layout = ops.PeLayout(pn, ps)
    sig = source((2, *G, Cc), kind, seed=21)
    ref = check(sig, lambda t: t, layout)
    shifted = torch.cat([sig.reshape(-1)[:1], sig.reshape(-1)])
    got = check(shifted, lambda t: t[1:].view(2, *G, Cc), layout)
    assert np.array_equal(S.bits(got), S.bits(ref))
    big = source((2, G[0] + 5, G[1] + 7, Cc), kind, seed=22)
    big[:, 3:3 + G[0], 5:5 + G[1]] = sig
    got = check(big, lambda t: t[:, 3:3 + G[0], 5:5 + G[1]], layout)
    assert np.array_equal(S.bits(got), S.bits(ref))
    for pad in (1, 3):
        assert np.array_equal(S.bits(check(sig, lambda t: t, layout, pad=pad)), S.bits(ref))


@pytest.mark.parametrize("name", ["2d_run18", "2d_run24", "3d_fast", "3d_elem"])
def test_round_trip_through_recon_finish(name):
    """8-bit signals cut into targets and scored against themselves: rcb_recon_finish stitches the source bytes back exactly, with
    zero squared error (premise: test_round8_gives_every_byte_back)"""
    pn, ps, Cc, G = grid(name)
    layout = ops.PeLayout(pn, ps)
    u8 = source((3, *G, Cc), "u8", seed=31).to(DEV)
    y = ops.signal_patch(u8, layout)
    back, whole, sse, n_bad = ops.recon_finish(y, target=y, layout=layout, want_u8=True, want_whole=True)
    assert back.dtype == torch.uint8 and torch.equal(back, u8)
    assert np.array_equal(S.bits(whole.cpu().numpy()), S.bits(S.unit8(u8.cpu().numpy())))
    assert sse.cpu().tolist() == [0.0] * 3 and n_bad.cpu().tolist() == [0] * 3


def test_source_offsets_beyond_32_bits():
    """two signals 2^31 + 16 bytes apart in one buffer: the source side is addressed with 64-bit offsets"""
    pn, ps, Cc, G = grid(FAST)
    E = int(np.prod(G)) * Cc
    gap = 2 ** 31 + 16
    buf = torch.empty(gap + E, dtype=torch.uint8, device=DEV)
    sig = source((2, *G, Cc), "u8", seed=41)
    buf[:E] = sig[0].reshape(-1).to(DEV)
    buf[gap:] = sig[1].reshape(-1).to(DEV)
    view = torch.as_strided(buf, (2, *G, Cc), (gap, G[1] * Cc, Cc, 1))
    got = run(view, ops.PeLayout(pn, ps))
    del view, buf
    assert np.array_equal(S.bits(got), S.bits(S.targets(sig.numpy(), pn, ps)))


def test_destination_offsets_beyond_32_bits():
    """more than 2^31 elements of y (one signal of 8192 elements repeated with signal stride 0): the first signal, the one across the
    2^31st element and the last are complete"""
    pn, ps, Cc = (2,), (1024,), 4
    E = 2 * 1024 * 4
    n = 2 ** 31 // E + 2
    sig = source((1, 2048, Cc), "f32", seed=51)
    y = ops.signal_patch(sig.to(DEV).expand(n, 2048, Cc), ops.PeLayout(pn, ps))
    assert tuple(y.shape) == (2 * n, 1024, Cc) and y.numel() > 2 ** 31
    want = S.bits(S.targets(sig.numpy(), pn, ps))
    for d in (0, 2 ** 31 // E - 1, 2 ** 31 // E, n - 1):
        assert np.array_equal(S.bits(y[2 * d:2 * d + 2].cpu().numpy()), want), d
    del y


# ---- refusals and the empty case ------------------------------------------------------------------------------------------------
def _raw(src, kind, n_data, pn, ps, Cc, ds, strides, cs, y, nd=None):
    nd = len(pn) if nd is None else nd
    k = max(len(pn), 1)
    rc = _lib.load().rcb_signal_patch(src, kind, n_data, nd, (C.c_int32 * k)(*pn), (C.c_int32 * k)(*ps), Cc, ds,
                                      (C.c_int64 * k)(*strides), cs, y, _lib.stream_ptr())
    _lib.check(rc, "rcb_signal_patch")


def _valid_call_works():
    pn, ps, Cc, G = grid(FAST)
    check(source((1, *G, Cc), "u8", seed=61), lambda t: t, ops.PeLayout(pn, ps))


def _layout(pn, ps):
    lay = ops.PeLayout([1], [1])
    lay.patch_nums, lay.patch_size = list(pn), list(ps)
    return lay


def test_refusals_of_the_wrapper_and_the_library():
    """every refusal raises RcbError with the library's message and launches nothing (y keeps its sentinel); a valid call follows"""
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)   # noqa: E731
    cases = [
        ("grid dimensions", lambda: ops.signal_patch(z(2, 3), _layout([], []))),
        ("grid dimensions", lambda: ops.signal_patch(z(1, 2, 2, 2, 2, 3), _layout([1] * 4, [2] * 4))),
        ("channels", lambda: ops.signal_patch(z(1, 4, 33), ops.PeLayout([2], [2]))),
        ("channels", lambda: ops.signal_patch(z(1, 4, 0), ops.PeLayout([2], [2]))),
        ("patches of", lambda: ops.signal_patch(z(1, 0, 3), _layout([0], [4]))),
        ("patches of", lambda: ops.signal_patch(z(1, 0, 3), _layout([4], [0]))),
        ("2^31 - 1 elements per signal", lambda: ops.signal_patch(z(1, 1, 1, 1).expand(1, 65536, 32768, 1), ops.PeLayout([1, 1], [65536, 32768]))),
        ("2^31 - 1", lambda: ops.signal_patch(z(1, 1, 1, 1).expand(1, 32768, 32768, 2), ops.PeLayout([1, 1], [32768, 32768]))),
        ("uint8 or fp32", lambda: ops.signal_patch(z(1, 4, 3, dtype=torch.int32), ops.PeLayout([2], [2]))),
        ("GPU tensor", lambda: ops.signal_patch(torch.zeros(1, 4, 3), ops.PeLayout([2], [2]))),
        ("the layout's is", lambda: ops.signal_patch(z(1, 5, 3), ops.PeLayout([2], [2]))),
        ("axes", lambda: ops.signal_patch(z(1, 4, 4, 3), ops.PeLayout([2], [2]))),
        ("output of shape", lambda: ops.signal_patch(z(1, 4, 3), ops.PeLayout([2], [2]), out=z(2, 2, 4))),
    ]
    src, y = z(1, 4, 3), torch.full((2, 2, 3), SENTINEL, device=DEV)
    sp, yp = C.c_void_p(src.data_ptr()), C.c_void_p(y.data_ptr())
    cases += [
        ("source kind", lambda: _raw(sp, 2, 1, [2], [2], 3, 12, [3], 1, yp)),
        ("source kind", lambda: _raw(sp, -1, 1, [2], [2], 3, 12, [3], 1, yp)),
        ("negative stride", lambda: _raw(sp, 1, 1, [2], [2], 3, 12, [-3], 1, yp)),
        ("negative stride", lambda: _raw(sp, 1, 1, [2], [2], 3, -12, [3], 1, yp)),
        ("negative stride", lambda: _raw(sp, 1, 1, [2], [2], 3, 12, [3], -1, yp)),
        ("null src or y", lambda: _raw(None, 1, 1, [2], [2], 3, 12, [3], 1, yp)),
        ("null src or y", lambda: _raw(sp, 1, 1, [2], [2], 3, 12, [3], 1, None)),
        ("grid dimensions", lambda: _raw(sp, 1, 1, [2], [2], 3, 12, [3], 1, yp, nd=0)),
        ("patches of", lambda: _raw(sp, 1, 1, [-2], [2], 3, 12, [3], 1, yp)),
        ("signals", lambda: _raw(sp, 1, -1, [2], [2], 3, 12, [3], 1, yp)),
    ]
    for text, call in cases:
        with pytest.raises(RcbError, match=text.replace("^", r"\^")):
            call()
    assert (y == SENTINEL).all()
    _raw(None, 1, 0, [2], [2], 3, 12, [3], 1, None)                      # no signals: nothing to address
    _valid_call_works()


def test_no_signals_give_an_empty_tensor():
    pn, ps, Cc, G = grid(FAST)
    for dt in (torch.uint8, torch.float32):
        y = ops.signal_patch(torch.zeros(0, *G, Cc, dtype=dt, device=DEV), ops.PeLayout(pn, ps))
        assert tuple(y.shape) == (0, int(np.prod(ps)), Cc) and y.dtype == torch.float32 and y.is_cuda
    _valid_call_works()
