"""rcb_signal_patch_pad and rcb_recon_finish_crop (N4 411: signals of any size -- edge-pad on the way in, crop on the way out) against
the numpy evaluator tests/extent_emul.py, whose premises tests/test_extent_emul_cpu.py checks.  Every comparison is bit for bit (fp32
through an int32 view) except the sums on arbitrary inputs, which are held to the reordering bound of tests/test_hip_recon.py against
the evaluator and bit for bit against rcb_recon_finish on a target that equals the reconstruction outside the extent."""
import ctypes as C

import numpy as np
import pytest
import torch

import extent_emul as X
import recon_emul as E
import signal_emul as S
from test_hip_recon import _border_intact, _bordered, dev, fill, sse_bound
from test_hip_signal import SENTINEL, source

pytestmark = pytest.mark.gpu

from recombiner_amd import _lib, ops  # noqa: E402
from recombiner_amd._lib import RcbError  # noqa: E402

DEV = "cuda"
F32 = np.float32
N = X.N_DATA
BORDER = ((torch.uint8, 0xA5), (torch.float32, -7.5), (torch.float64, -7.5), (torch.int32, -77))


def geo(name):
    pn, ps, Cc, _ = X.CASES[name]
    return pn, ps, Cc, X.grid_of(pn, ps), ops.PeLayout(pn, ps)


# ---- rcb_signal_patch_pad -------------------------------------------------------------------------------------------------------
def run_pad(view, layout, pad=64):
    """ops.signal_patch_pad into a slice of a sentinel-filled buffer (pad floats before and after: 64 keeps y 16-byte aligned, an odd
    pad does not); the sentinel must be intact around the slice -> y as numpy"""
    per, P = int(np.prod(layout.patch_nums)), int(np.prod(layout.patch_size))
    shape = (view.shape[0] * per, P, view.shape[-1])
    n = int(np.prod(shape))
    buf = torch.full((pad + n + pad,), SENTINEL, device=DEV)
    out = buf[pad:pad + n].view(shape)
    got = ops.signal_patch_pad(view, layout, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:pad] == F32(SENTINEL)).all() and (host[pad + n:] == F32(SENTINEL)).all(), "guard words overwritten"
    return host[pad:pad + n].reshape(shape)


def check_pad(base, make_view, layout, pad=64):
    """base: CPU tensor; make_view: the same view arithmetic on the CPU tensor (-> the evaluator, through a zero-copy numpy view) and
    on its device copy (-> the kernel).  -> y"""
    want = X.targets(make_view(base).numpy(), layout.patch_nums, layout.patch_size)
    got = run_pad(make_view(base.to(DEV)), layout, pad)
    assert got.dtype == F32 and got.shape == want.shape
    bad = np.flatnonzero(S.bits(got) != S.bits(want))
    assert bad.size == 0, f"{bad.size} of {want.size} elements differ, first at flat index {bad[:5]}"
    return got


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("name,size", X.ALL)
def test_pad_of_contiguous_sources(name, size, kind):
    """uint8 and fp32 (NaN payloads, +-0, +-inf, denormals among the values) on every shape, guard words around y; a y that is not
    16-byte aligned (the element path of the same shape) gives the same bits; size = G gives ops.signal_patch's"""
    pn, ps, Cc, G, layout = geo(name)
    base = source((N, *size, Cc), kind, seed=len(name) + sum(size))
    y = check_pad(base, lambda t: t, layout)
    assert np.array_equal(S.bits(check_pad(base, lambda t: t, layout, pad=3)), S.bits(y))
    if kind == "f32" and base.numel() >= 15:
        assert np.isnan(y).sum() >= np.isnan(base.numpy()).sum() > 0
    if tuple(size) == G:
        assert np.array_equal(S.bits(ops.signal_patch(base.to(DEV), layout).cpu().numpy()), S.bits(y))


@pytest.mark.parametrize("name,size", [("2d", (7, 11)), ("2d_aligned", (6, 10))])
def test_pad_of_every_byte_value(name, size):
    """on the element path (rows of 33 source elements) and on the path that loads quads (rows of 40)"""
    pn, ps, Cc, G, layout = geo(name)
    base = source((N, *size, Cc), "u8", seed=5)
    assert len(np.unique(base.numpy())) == 256
    y = check_pad(base, lambda t: t, layout)
    assert np.array_equal(np.unique(S.bits(y)), S.bits(S.unit8(np.arange(256, dtype=np.uint8))))


def _views(size, Cc, n):
    """name -> (shape of the base buffer, view arithmetic): each gives [n, s0, s1, C]"""
    s0, s1 = size
    return {
        "channels_first": ((n, Cc, s0, s1), lambda t: t.movedim(1, -1)),
        "window_odd": ((n, s0 + 5, s1 + 7, Cc), lambda t: t[:, 3:3 + s0, 5:5 + s1]),
        # origin (2, 4) in rows of 32 pixels behind a storage offset of 4 elements: for C = 4 every run start stays 16-byte aligned
        "window_even": ((n * (s0 + 5) * 32 * Cc + 4,), lambda t: t[4:].view(n, s0 + 5, 32, Cc)[:, 2:2 + s0, 4:4 + s1]),
        "offset_one": ((n * s0 * s1 * Cc + 1,), lambda t: t[1:].view(n, s0, s1, Cc)),
        "channel_stride0": ((n, s0, s1, 1), lambda t: t.expand(n, s0, s1, Cc)),
        "signal_stride0": ((1, s0, s1, Cc), lambda t: t.expand(n, s0, s1, Cc)),
    }


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("view", ["channels_first", "window_odd", "window_even", "offset_one", "channel_stride0", "signal_stride0"])
@pytest.mark.parametrize("name,size", [("2d", (7, 11)), ("2d", (5, 4)), ("2d_aligned", (6, 10)), ("2d_elem", (4, 7))])
def test_pad_of_strided_views(name, size, view, kind):
    """channel-last and channel-first, a window of a larger tensor behind a storage offset, an expanded channel: the strides go to the
    kernel as they are"""
    pn, ps, Cc, G, layout = geo(name)
    shape, make = _views(size, Cc, N)[view]
    check_pad(source(shape, kind, seed=11), make, layout)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_pad_on_either_memory_path_gives_the_same_bits(kind):
    """the aligned case (quads of 4 existing source elements: one load) against the same signals behind a storage offset of one
    element and inside a larger buffer at an odd origin (element by element)"""
    pn, ps, Cc, G, layout = geo("2d_aligned")
    size = (6, 10)
    sig = source((N, *size, Cc), kind, seed=21)
    ref = check_pad(sig, lambda t: t, layout)
    shifted = torch.cat([sig.reshape(-1)[:1], sig.reshape(-1)])
    assert np.array_equal(S.bits(check_pad(shifted, lambda t: t[1:].view(N, *size, Cc), layout)), S.bits(ref))
    big = source((N, size[0] + 5, size[1] + 7, Cc), kind, seed=22)
    big[:, 3:3 + size[0], 5:5 + size[1]] = sig
    assert np.array_equal(S.bits(check_pad(big, lambda t: t[:, 3:3 + size[0], 5:5 + size[1]], layout)), S.bits(ref))


def test_pad_source_offsets_beyond_32_bits():
    """two signals 2^31 + 16 bytes apart in one buffer: the source side is addressed with 64-bit offsets"""
    pn, ps, Cc, G, layout = geo("2d_aligned")
    size = (6, 10)
    n_el = size[0] * size[1] * Cc
    gap = 2 ** 31 + 16
    buf = torch.empty(gap + n_el, dtype=torch.uint8, device=DEV)
    sig = source((2, *size, Cc), "u8", seed=41)
    buf[:n_el] = sig[0].reshape(-1).to(DEV)
    buf[gap:] = sig[1].reshape(-1).to(DEV)
    view = torch.as_strided(buf, (2, *size, Cc), (gap, size[1] * Cc, Cc, 1))
    got = run_pad(view, layout)
    del view, buf
    assert np.array_equal(S.bits(got), S.bits(X.targets(sig.numpy(), pn, ps)))


# ---- rcb_recon_finish_crop ------------------------------------------------------------------------------------------------------
def inputs(name, kind, seed):
    pn, ps, Cc, G, layout = geo(name)
    rows, P = N * int(np.prod(pn)), int(np.prod(ps))
    if kind == "dyadic":
        return E.dyadic((rows, P, Cc), seed), E.dyadic((rows, P, Cc), seed + 1)
    if kind == "normal":
        rng = np.random.RandomState(seed)
        return rng.randn(rows, P, Cc).astype(F32), rng.randn(rows, P, Cc).astype(F32)
    return fill((rows, P, Cc), kind, seed), np.random.RandomState(seed + 1).rand(rows, P, Cc).astype(F32)


def run_crop(y, t, layout, size, mode, shift=0, u8=True, whole=True):
    """ops.recon_finish(size=) into outputs with a canary border (shift = 1: off their 16-byte alignment), which must stay intact"""
    Cc = y.shape[-1]
    shape = (N, *size, Cc)
    bufs = [_bordered(shape, torch.uint8, 0xA5, shift) if u8 and mode == 0 else (None, None),
            _bordered(shape, torch.float32, -7.5, shift) if whole else (None, None),
            _bordered((N,), torch.float64, -7.5, shift), _bordered((N,), torch.int32, -77, shift)]
    out = ops.recon_finish(dev(y), None if t is None else dev(t), layout=layout, size=size, mode=mode,
                                out=tuple(v for _, v in bufs))
    torch.cuda.synchronize()
    for (buf, v), (_, f) in zip(bufs, BORDER):
        assert buf is None or _border_intact(buf, v.numel(), f, shift)
    return out


def assert_whole_mode0(whole, want, y, pn, ps, size):
    """`whole` of the 8-bit mode against the evaluator, bit for bit -- but for an input of exactly -0.0: the header defines v through
    fmaxf(x, 0), which IEEE 754 lets return either zero for (-0, +0); numpy's maximum keeps its first operand (the evaluator's v is
    -0.0), the device's v_max_f32 orders -0 below +0 (v is +0.0).  That is rcb_recon_finish's own arithmetic, which this entry must
    keep (tests/test_hip_recon.py compares the same output by value); there the two must both be zero."""
    got, want = whole.cpu().numpy(), np.asarray(want)
    x = E.stitch(np.asarray(y), pn, ps)[(slice(None),) + tuple(slice(0, s) for s in size)]
    neg0 = (x == 0) & np.signbit(x)
    assert got.shape == want.shape == x.shape
    assert np.array_equal(S.bits(got)[~neg0], S.bits(want)[~neg0])
    assert (got[neg0] == 0).all() and (want[neg0] == 0).all()


@pytest.mark.parametrize("kind", ["random", "special"])
@pytest.mark.parametrize("name,size", X.ALL)
def test_crop_mode0_matches_the_evaluator(name, size, kind):
    pn, ps, Cc, G, layout = geo(name)
    y, t = inputs(name, kind, 1)
    want = X.finish_crop(y, t, pn, ps, size, mode=0)
    for shift in (0, 1):
        u8, whole, sse, n_bad = run_crop(y, t, layout, size, 0, shift)
        assert tuple(u8.shape) == want["u8"].shape == (N, *size, Cc)
        assert torch.equal(u8.cpu(), torch.from_numpy(want["u8"]))
        assert_whole_mode0(whole, want["whole"], y, pn, ps, size)
        assert np.array_equal(n_bad.cpu().numpy(), want["n_bad"])
        got = sse.cpu().numpy()
        fin = want["n_bad"] == 0
        assert np.isnan(got[~fin]).all()
        err, bound = np.abs(got - want["sse"])[fin], sse_bound(want["terms"])[fin]       # n = the elements inside the extent
        assert want["terms"].shape[1] == int(np.prod(size)) * Cc
        if fin.any():
            print(f"{name} {size} {kind} shift {shift}: worst sse error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
            assert (err <= bound).all()


@pytest.mark.parametrize("name,size", X.ALL)
def test_crop_mode1_is_exact_on_dyadic_inputs_and_within_the_bound_elsewhere(name, size):
    pn, ps, Cc, G, layout = geo(name)
    y, t = inputs(name, "dyadic", 3)
    want = X.finish_crop(y, t, pn, ps, size, mode=1)
    u8, whole, sse, n_bad = run_crop(y, t, layout, size, 1)
    assert u8 is None and np.array_equal(S.bits(whole.cpu().numpy()), S.bits(want["whole"]))
    assert torch.equal(sse.cpu(), torch.from_numpy(want["sse"])) and int(n_bad.abs().sum()) == 0
    y, t = inputs(name, "normal", 5)
    want = X.finish_crop(y, t, pn, ps, size, mode=1)
    _, _, sse, _ = run_crop(y, t, layout, size, 1, whole=False)
    assert (np.abs(sse.cpu().numpy() - want["sse"]) <= sse_bound(want["terms"])).all()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,size", X.ALL)
def test_crop_sse_is_recon_finish_on_a_target_that_equals_v_outside(name, size, mode):
    """bit for bit on arbitrary inputs: v = what rcb_recon_finish itself makes of y (its `whole` without a layout), put into the target
    at every position outside the extent, gives d = 0 there -- the same +0.0 in the same chain of additions.  Also: a datapoint
    alone gives the bits it has in the batch, a second run the same bits, and size = G every output of rcb_recon_finish"""
    pn, ps, Cc, G, layout = geo(name)
    y, t = inputs(name, "random" if mode == 0 else "normal", 7)
    yd, td = dev(y), dev(t)
    _, v, _, _ = ops.recon_finish(yd, None, layout=None, mode=mode, want_whole=True)
    m = torch.from_numpy(S.patch(X.inside(N, pn, ps, Cc, size), pn, ps)).to(DEV)
    assert m.shape == yd.shape and int(m.sum()) == N * int(np.prod(size)) * Cc
    _, _, want, want_bad = ops.recon_finish(yd, torch.where(m, td, v), layout=layout, mode=mode)
    _, _, sse, n_bad = ops.recon_finish(yd, td, layout=layout, size=size, mode=mode)
    assert torch.equal(sse.view(torch.int64), want.view(torch.int64)) and torch.equal(n_bad, want_bad)
    assert bool(torch.isfinite(sse).all()) and (tuple(size) == G or not torch.equal(sse, ops.recon_finish(yd, td, layout=layout, mode=mode)[2]))
    assert torch.equal(ops.recon_finish(yd, td, layout=layout, size=size, mode=mode)[2], sse)
    per = yd.shape[0] // N
    for d in range(N):
        alone = ops.recon_finish(yd[d * per:(d + 1) * per], td[d * per:(d + 1) * per], layout=layout, size=size, mode=mode)[2]
        assert torch.equal(alone.view(torch.int64), sse[d:d + 1].view(torch.int64))
    if tuple(size) == G:
        a = ops.recon_finish(yd, td, layout=layout, mode=mode, want_u8=mode == 0, want_whole=True)
        b = ops.recon_finish(yd, td, layout=layout, size=size, mode=mode, want_u8=mode == 0, want_whole=True)
        assert (a[0] is None and b[0] is None) or torch.equal(a[0], b[0])
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and a[1].shape == b[1].shape
        assert torch.equal(a[2].view(torch.int64), b[2].view(torch.int64)) and torch.equal(a[3], b[3])


@pytest.mark.parametrize("name,size", [("1d", (9,)), ("2d", (7, 11)), ("2d", (5, 4)), ("2d_aligned", (6, 10)), ("3d", (2, 7, 5)),
                                       ("unpatched", (3, 4))])
def test_crop_ignores_what_lies_outside_the_extent(name, size):
    """NaN and inf at EVERY position outside the extent, in y and in the target, change no output bit; one inside is counted and makes
    only its own datapoint's sse NaN"""
    pn, ps, Cc, G, layout = geo(name)
    y, t = inputs(name, "random", 9)
    clean = run_crop(y, t, layout, size, 0)
    m = S.patch(X.inside(N, pn, ps, Cc, size), pn, ps)
    assert not m.all()
    yb, tb = y.copy(), t.copy()
    yb[~m] = np.nan
    tb[~m] = np.inf
    got = run_crop(yb, tb, layout, size, 0)
    assert all(torch.equal(a, b) for a, b in zip(got, clean)) and got[3].cpu().tolist() == [0] * N
    raw = run_crop(yb, tb, layout, size, 1)
    assert torch.equal(raw[2], run_crop(y, t, layout, size, 1)[2]) and raw[3].cpu().tolist() == [0] * N
    per = y.shape[0] // N
    inside_1 = np.argwhere(m[per:2 * per])                      # datapoint 1: its first and its last element inside the extent
    yb[(per + inside_1[0][0], *inside_1[0][1:])] = np.nan
    tb[(per + inside_1[-1][0], *inside_1[-1][1:])] = -np.inf
    u8, whole, sse, n_bad = run_crop(yb, tb, layout, size, 0)
    assert n_bad.cpu().tolist() == [0, 2, 0] and bool(torch.isnan(sse[1])) and torch.equal(sse[[0, 2]], clean[2][[0, 2]])
    want = X.finish_crop(yb, tb, pn, ps, size, mode=0)
    assert torch.equal(u8.cpu(), torch.from_numpy(want["u8"])) and np.array_equal(n_bad.cpu().numpy(), want["n_bad"])
    assert torch.equal(u8[[0, 2]], clean[0][[0, 2]])


@pytest.mark.parametrize("name,size", X.ALL)
def test_round_trip_of_8_bit_signals(name, size):
    """recon_finish(signal_patch_pad(u8), size=) scored against itself returns the source bytes with sse 0"""
    pn, ps, Cc, G, layout = geo(name)
    u8 = source((N, *size, Cc), "u8", seed=31).to(DEV)
    y = ops.signal_patch_pad(u8, layout)
    back, whole, sse, n_bad = ops.recon_finish(y, target=y, layout=layout, size=size, want_u8=True, want_whole=True)
    assert back.dtype == torch.uint8 and torch.equal(back, u8)
    assert np.array_equal(S.bits(whole.cpu().numpy()), S.bits(S.unit8(u8.cpu().numpy())))
    assert sse.cpu().tolist() == [0.0] * N and n_bad.cpu().tolist() == [0] * N


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _raw_pad(src, kind, n_data, pn, ps, size, Cc, ds, strides, cs, y, nd=None):
    nd = len(pn) if nd is None else nd
    k = max(len(pn), 1)
    arr = None if size is None else (C.c_int32 * k)(*size)
    rc = _lib.load().rcb_signal_patch_pad(src, kind, n_data, nd, (C.c_int32 * k)(*pn), (C.c_int32 * k)(*ps), arr, Cc, ds,
                                          (C.c_int64 * k)(*strides), cs, y, _lib.stream_ptr())
    _lib.check(rc, "rcb_signal_patch_pad")


def _layout(pn, ps):
    lay = ops.PeLayout([1], [1])
    lay.patch_nums, lay.patch_size = list(pn), list(ps)
    return lay


def test_refusals_of_signal_patch_pad():
    """rcb_signal_patch's refusals, a null size and a size outside [1, G]: RcbError with the library's message, nothing launched (y
    keeps its sentinel); a valid call follows"""
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)   # noqa: E731
    cases = [
        ("grid dimensions", lambda: ops.signal_patch_pad(z(2, 3), _layout([], []))),
        ("grid dimensions", lambda: ops.signal_patch_pad(z(1, 2, 2, 2, 2, 3), _layout([1] * 4, [2] * 4))),
        ("channels", lambda: ops.signal_patch_pad(z(1, 4, 33), ops.PeLayout([2], [2]))),
        ("channels", lambda: ops.signal_patch_pad(z(1, 4, 0), ops.PeLayout([2], [2]))),
        ("patches of", lambda: ops.signal_patch_pad(z(1, 1, 3), _layout([0], [4]))),
        ("patches of", lambda: ops.signal_patch_pad(z(1, 1, 3), _layout([4], [0]))),
        ("2^31 - 1 elements per signal", lambda: ops.signal_patch_pad(z(1, 2, 2, 1), ops.PeLayout([1, 1], [65536, 32768]))),
        ("2^31 - 1", lambda: ops.signal_patch_pad(z(1, 2, 2, 2), ops.PeLayout([1, 1], [32768, 32768]))),
        ("uint8 or fp32", lambda: ops.signal_patch_pad(z(1, 4, 3, dtype=torch.int32), ops.PeLayout([2], [2]))),
        ("GPU tensor", lambda: ops.signal_patch_pad(torch.zeros(1, 4, 3), ops.PeLayout([2], [2]))),
        ("positions", lambda: ops.signal_patch_pad(z(1, 5, 3), ops.PeLayout([2], [2]))),            # larger than the grid
        ("positions", lambda: ops.signal_patch_pad(z(1, 0, 3), ops.PeLayout([2], [2]))),            # an empty axis
        ("positions", lambda: ops.signal_patch_pad(z(1, 4, 5, 3), ops.PeLayout([2, 2], [2, 2]))),
        ("axes", lambda: ops.signal_patch_pad(z(1, 4, 4, 3), ops.PeLayout([2], [2]))),
        ("output of shape", lambda: ops.signal_patch_pad(z(1, 3, 3), ops.PeLayout([2], [2]), out=z(2, 2, 4))),
    ]
    src, y = z(1, 3, 3), torch.full((2, 2, 3), SENTINEL, device=DEV)
    sp, yp = C.c_void_p(src.data_ptr()), C.c_void_p(y.data_ptr())
    cases += [
        ("null size", lambda: _raw_pad(sp, 1, 1, [2], [2], None, 3, 9, [3], 1, yp)),
        ("positions", lambda: _raw_pad(sp, 1, 1, [2], [2], [5], 3, 9, [3], 1, yp)),
        ("positions", lambda: _raw_pad(sp, 1, 1, [2], [2], [0], 3, 9, [3], 1, yp)),
        ("positions", lambda: _raw_pad(sp, 1, 1, [2], [2], [-3], 3, 9, [3], 1, yp)),
        ("source kind", lambda: _raw_pad(sp, 2, 1, [2], [2], [3], 3, 9, [3], 1, yp)),
        ("negative stride", lambda: _raw_pad(sp, 1, 1, [2], [2], [3], 3, 9, [-3], 1, yp)),
        ("negative stride", lambda: _raw_pad(sp, 1, 1, [2], [2], [3], 3, -9, [3], 1, yp)),
        ("negative stride", lambda: _raw_pad(sp, 1, 1, [2], [2], [3], 3, 9, [3], -1, yp)),
        ("null src or y", lambda: _raw_pad(None, 1, 1, [2], [2], [3], 3, 9, [3], 1, yp)),
        ("null src or y", lambda: _raw_pad(sp, 1, 1, [2], [2], [3], 3, 9, [3], 1, None)),
        ("grid dimensions", lambda: _raw_pad(sp, 1, 1, [2], [2], [3], 3, 9, [3], 1, yp, nd=0)),
        ("patches of", lambda: _raw_pad(sp, 1, 1, [-2], [2], [3], 3, 9, [3], 1, yp)),
        ("signals", lambda: _raw_pad(sp, 1, -1, [2], [2], [3], 3, 9, [3], 1, yp)),
    ]
    for text, call in cases:
        with pytest.raises(RcbError, match=text.replace("^", r"\^")):
            call()
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()
    _raw_pad(None, 1, 0, [2], [2], [3], 3, 9, [3], 1, None)                  # no signals: nothing to address
    assert tuple(ops.signal_patch_pad(z(0, 3, 3), ops.PeLayout([2], [2])).shape) == (0, 2, 3)
    _raw_pad(sp, 1, 1, [2], [2], [3], 3, 9, [3], 1, yp)                      # the valid call
    assert np.array_equal(y.cpu().numpy(), X.targets(src.cpu().numpy(), [2], [2]))


def _raw_crop(y, t, n_rows, P, Cc, nd, pn, ps, size, mode, u8, whole, sse, n_bad, ws):
    arr = lambda v: None if v is None else (C.c_int32 * 4)(*(list(v) + [0] * (4 - len(v))))      # noqa: E731
    p = lambda v: C.c_void_p(0 if v is None else v.data_ptr())          # noqa: E731
    return _lib.load().rcb_recon_finish_crop(p(y), p(t), n_rows, P, Cc, nd, arr(pn), arr(ps), arr(size), mode, p(u8), p(whole),
                                             p(sse), p(n_bad), p(ws), 0 if ws is None else ws.numel(), _lib.stream_ptr())


def test_refusals_of_recon_finish_crop():
    """rcb_recon_finish's refusals, nd = 0, a null size and a size outside [1, G]: the library returns RCB_ERR_* with a message before it
    launches anything (the outputs and their canary borders keep their fill), and ops.recon_finish(size=) raises RcbError"""
    pn, ps, Cc, rows, P, size = (2, 3), (4, 5), 3, 12, 20, (7, 11)
    y, t = dev(fill((rows, P, Cc), "random", 1)), dev(fill((rows, P, Cc), "random", 2))
    shape = (2, *size, Cc)
    bufs = [_bordered(shape, dt, f) if i < 2 else _bordered((2,), dt, f) for i, (dt, f) in enumerate(BORDER)]
    u8, whole, sse, n_bad = (v for _, v in bufs)
    ws = torch.empty(1 << 16, device=DEV, dtype=torch.uint8)
    lib = _lib.load()
    base = dict(y=y, t=t, n_rows=rows, P=P, Cc=Cc, nd=2, pn=pn, ps=ps, size=size, mode=0, u8=u8, whole=whole, sse=sse, n_bad=n_bad,
                ws=ws)
    assert _raw_crop(**base) == 0                                         # (the valid call, for contrast)
    torch.cuda.synchronize()
    assert float(sse[0]) != -7.5
    for (_, v), (_, f) in zip(bufs, BORDER):
        v.fill_(f)
    refused = {
        "null size": dict(size=None),
        "size above the grid": dict(size=(9, 11)),
        "size above the grid, last axis": dict(size=(7, 16)),
        "size 0": dict(size=(0, 11)),
        "negative size": dict(size=(7, -1)),
        "nd = 0": dict(nd=0, pn=(), ps=(), size=(), n_rows=rows, P=P),
        "nd > 3": dict(nd=4, pn=(1, 1, 2, 3), ps=(1, 1, 4, 5), size=(1, 1, 7, 11)),
        "C = 0": dict(Cc=0),
        "C = 33": dict(Cc=33),
        "P != prod(patch_size)": dict(ps=(4, 4)),
        "rows no multiple of prod(patch_nums)": dict(n_rows=11),
        "u8 with mode 1": dict(mode=1),
        "sse without target": dict(t=None),
        "2^31 elements per stitched datapoint": dict(pn=(1 << 15, 1 << 14), ps=(4, 5), n_rows=1 << 29),
        "workspace too small": dict(ws=ws[:8]),
        "null y": dict(y=None),
        "null patch geometry": dict(pn=None),
    }
    for what, change in refused.items():
        rc = _raw_crop(**dict(base, **change))
        assert rc < 0, what
        assert len(lib.rcb_last_error_string()) > 10, what
    torch.cuda.synchronize()
    for (buf, _), (_, f) in zip(bufs, BORDER):
        assert bool((buf == f).all())                                  # nothing was launched
    lay = ops.PeLayout(pn, ps)
    calls = {
        "no layout": lambda: ops.recon_finish(y, t, size=size),
        "size of another rank": lambda: ops.recon_finish(y, t, layout=lay, size=(7,)),
        "size above the grid": lambda: ops.recon_finish(y, t, layout=lay, size=(9, 11)),
        "size 0": lambda: ops.recon_finish(y, t, layout=lay, size=(7, 0)),
        "P != prod(patch_size)": lambda: ops.recon_finish(y, t, layout=ops.PeLayout(pn, (4, 4)), size=(7, 11)),
        "rows no multiple": lambda: ops.recon_finish(y[:11], t[:11], layout=lay, size=size),
        "u8 with mode 1": lambda: ops.recon_finish(y, t, layout=lay, size=size, mode=1, want_u8=True),
        "cpu tensor": lambda: ops.recon_finish(y.cpu(), None, layout=lay, size=size),
        "fp64": lambda: ops.recon_finish(y.double(), None, layout=lay, size=size),
        "strided": lambda: ops.recon_finish(y.transpose(0, 1), None, layout=lay, size=size),
        "target shape": lambda: ops.recon_finish(y, t[:6], layout=lay, size=size),
        "output shape": lambda: ops.recon_finish(y, t, layout=lay, size=size, out=(None, torch.empty(2, 8, 15, 3, device=DEV), None, None)),
        "empty": lambda: ops.recon_finish(y[:0], None, layout=lay, size=size),
    }
    for what, call in calls.items():
        with pytest.raises(RcbError):
            call()
            pytest.fail(what)
    assert ops.recon_finish(y, t, layout=lay, size=size)[2].shape == (2,)
