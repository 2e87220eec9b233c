"""rcb_signal_patch_fmt and rcb_recon_finish_fmt (N4 412: 16-bit PCM audio and 9- to 16-bit images on the device) against the numpy
evaluator tests/sample16_emul.py, whose premises tests/test_sample16_emul_cpu.py checks.  Every comparison is bit for bit (fp32 through
an int32 view, the integers as integers) except the sums on arbitrary inputs, which are held to the a-priori reordering bound of
tests/test_hip_recon.py (n * 2^-53 * sum of the terms).  Guard words surround every output.  The 16-bit buffers on the device are int16
tensors viewed as uint16 where the format wants that: the kernels see the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import extent_emul as X
import recon_emul as E
import sample16_emul as Q
import signal_emul as S
from test_hip_extent import _views
from test_hip_recon import _border_intact, _bordered, dev, fill, sse_bound
from test_hip_signal import SENTINEL, source

pytestmark = pytest.mark.gpu

from recombiner_amd import _lib, ops  # noqa: E402
from recombiner_amd._lib import RcbError  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

DEV = "cuda"
F32 = np.float32
N = X.N_DATA
QFILL = 0x5A5A
# extent_emul's shapes (nd 1 .. 3, C 1 / 3 / 4, R % 4 and L % 4 zero and not, an extent that ends inside a quad, an extent of 1 on an
# axis) and the 1-D signal that crosses the 8192-element chunk of a workgroup, whole and cut short inside a quad
CASES = dict(X.CASES, chunk=((2,), (4100,), 1, [(8200,), (8197,)]))
ALL = [(name, size) for name, (_, _, _, sizes) in CASES.items() for size in sizes]
FORMATS = {"u16_12": Q.u16(12), "s16": Q.S16}


def sf(fmt):
    return SampleFormat(*fmt)


def geo(name):
    pn, ps, Cc, _ = CASES[name]
    return pn, ps, Cc, X.grid_of(pn, ps), ops.PeLayout(pn, ps)


def samples(shape, fmt, seed):
    """a CPU tensor of stored samples: the whole 16-bit range for s16; 0 .. M for u16 with a few words above M among them (those are
    not clamped); the older kinds get tests/test_hip_signal.py's sources"""
    if fmt[0] < 2:
        return source(shape, "u8" if fmt[0] == 0 else "f32", seed)
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    if fmt[0] == 3:
        a = rng.randint(-32768, 32768, size=n).astype(np.int16)
        a[rng.permutation(n)[:min(n, 4)]] = np.array([-32768, 32767, 0, -1], dtype=np.int16)[:min(n, 4)]
    else:
        M = Q.m_of(fmt)
        a = rng.randint(0, M + 1, size=n).astype(np.uint16)
        a[rng.permutation(n)[:min(n, 4)]] = np.array([0, M, min(M + 1, 65535), 65535], dtype=np.uint16)[:min(n, 4)]
    return torch.from_numpy(a.reshape(shape))


# ---- rcb_signal_patch_fmt ------------------------------------------------------------------------------------------------------------
def run_patch(view, layout, fmt, padded=True, guard=64, old=False):
    """ops.signal_patch(_pad)(sample_format=) into a slice of a sentinel-filled buffer (guard floats before and after: 64 keeps y
    16-byte aligned, an odd guard does not); the sentinel must be intact around the slice -> y as numpy.  old: without a format"""
    per, P = int(np.prod(layout.patch_nums)), int(np.prod(layout.patch_size))
    shape = (view.shape[0] * per, P, view.shape[-1])
    n = int(np.prod(shape))
    buf = torch.full((guard + n + guard,), SENTINEL, device=DEV)
    out = buf[guard:guard + n].view(shape)
    call = ops.signal_patch_pad if padded else ops.signal_patch
    got = call(view, layout, out=out) if old else call(view, layout, out=out, sample_format=sf(fmt))
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:guard] == F32(SENTINEL)).all() and (host[guard + n:] == F32(SENTINEL)).all(), "guard words overwritten"
    return host[guard:guard + n].reshape(shape)


def check_patch(base, make_view, layout, fmt, padded=True, guard=64):
    want = Q.targets(make_view(base).numpy(), layout.patch_nums, layout.patch_size, fmt, pad=padded)
    got = run_patch(make_view(base.to(DEV)), layout, fmt, padded, guard)
    assert got.dtype == F32 and got.shape == want.shape
    bad = np.flatnonzero(S.bits(got) != S.bits(want))
    assert bad.size == 0, f"{bad.size} of {want.size} elements differ, first at flat index {bad[:5]}"
    return got


EVERY = [Q.u16(9), Q.u16(10), Q.u16(12), Q.u16(16), Q.S16]


@pytest.mark.parametrize("fmt", EVERY, ids=lambda f: "s16" if f == Q.S16 else "u16_%d" % f[1])
def test_every_16_bit_value(fmt):
    """one 1-D signal of 65536 samples x 1 channel (8 chunks) holds every 16-bit word: y is the evaluator's (a u16 word above M is not
    clamped); then every REPRESENTABLE value goes round: recon_finish(signal_patch(q)) returns q and v = in(q), sse == 0, n_bad == 0"""
    layout = ops.PeLayout((8,), (8192,))
    words = np.arange(65536, dtype=np.uint16)[np.random.RandomState(3).permutation(65536)]
    q = words.view(np.int16) if fmt == Q.S16 else words
    y = check_patch(torch.from_numpy(q.reshape(1, 65536, 1).copy()), lambda t: t, layout, fmt, padded=False)
    assert len(np.unique(S.bits(y))) == 65536
    if fmt[0] == 2:
        q = q & np.uint16(Q.m_of(fmt))                          # 0 .. M, each 65536 / (M + 1) times
        assert len(np.unique(q)) == Q.m_of(fmt) + 1
    src = torch.from_numpy(q.reshape(1, 65536, 1).copy()).to(DEV)
    yd = ops.signal_patch(src, layout, sample_format=sf(fmt))
    back, whole, sse, n_bad = ops.recon_finish(yd, yd, layout=layout, sample_format=sf(fmt), want_int=True, want_whole=True)
    assert back.dtype == sf(fmt).dtype and back.shape == src.shape
    assert np.array_equal(back.cpu().numpy(), src.cpu().numpy())
    assert np.array_equal(S.bits(whole.cpu().numpy()), S.bits(Q.to_target(q.reshape(1, 65536, 1), fmt)))
    assert sse.cpu().tolist() == [0.0] and n_bad.cpu().tolist() == [0]


@pytest.mark.parametrize("fmt", FORMATS.values(), ids=FORMATS.keys())
@pytest.mark.parametrize("name,size", ALL)
def test_targets_of_contiguous_sources(name, size, fmt):
    """the padded form on every shape; a y that is not 16-byte aligned (the element path of the same shape) gives the same bits; with
    size = G the uncropped form (a null `size`) gives them too"""
    pn, ps, Cc, G, layout = geo(name)
    base = samples((N, *size, Cc), fmt, seed=len(name) + sum(size))
    y = check_patch(base, lambda t: t, layout, fmt)
    assert np.array_equal(S.bits(check_patch(base, lambda t: t, layout, fmt, guard=3)), S.bits(y))
    if tuple(size) == G:
        assert np.array_equal(S.bits(check_patch(base, lambda t: t, layout, fmt, padded=False)), S.bits(y))


def _views16(size, Cc, n):
    s0, s1 = size
    return dict(_views(size, Cc, n), transposed=((n, s1, s0, Cc), lambda t: t.transpose(1, 2)))


@pytest.mark.parametrize("fmt", FORMATS.values(), ids=FORMATS.keys())
@pytest.mark.parametrize("view", ["channels_first", "transposed", "window_odd", "window_even", "offset_one", "channel_stride0",
                                  "signal_stride0"])
@pytest.mark.parametrize("name,size", [("2d", (7, 11)), ("2d", (8, 12)), ("2d_aligned", (6, 10))])
def test_targets_of_strided_views(name, size, view, fmt):
    """channel-first storage, transposed axes, a window of a larger signal behind a storage offset (window_even keeps every run start
    8-byte aligned for C = 4: quads are loaded; offset_one breaks the alignment: they are not), a stride-0 channel and signal"""
    pn, ps, Cc, G, layout = geo(name)
    shape, make = _views16(size, Cc, N)[view]
    check_patch(samples(shape, fmt, seed=11), make, layout, fmt)


@pytest.mark.parametrize("fmt", FORMATS.values(), ids=FORMATS.keys())
@pytest.mark.parametrize("name,size", [("2d_aligned", (6, 10)), ("2d", (8, 12)), ("chunk", (8200,))])
def test_both_source_paths_give_the_same_bits(name, size, fmt):
    """the aligned signals (quads of 4 existing source elements: one 8-byte load) against the same signals one element further on
    (element by element)"""
    pn, ps, Cc, G, layout = geo(name)
    sig = samples((N, *size, Cc), fmt, seed=21)
    ref = check_patch(sig, lambda t: t, layout, fmt)
    flat = sig.numpy().reshape(-1)
    shifted = torch.from_numpy(np.concatenate([flat[:1], flat]))
    assert np.array_equal(S.bits(check_patch(shifted, lambda t: t[1:].view(N, *size, Cc), layout, fmt)), S.bits(ref))


def test_u16_source_as_an_int16_tensor():
    """`uint16` support in torch is thin: a u16 source may arrive as int16, its bits reinterpreted"""
    pn, ps, Cc, G, layout = geo("2d")
    q = samples((N, 7, 11, Cc), Q.u16(16), seed=5)
    want = Q.targets(q.numpy(), pn, ps, Q.u16(16), pad=True)
    got = ops.signal_patch_pad(q.view(torch.int16).to(DEV), layout, sample_format=SampleFormat.u16(16))
    assert np.array_equal(S.bits(got.cpu().numpy()), S.bits(want)) and (want > 0.5).any()


def test_16_bit_source_offsets_beyond_32_bits():
    """two signals 2^31 + 16 ELEMENTS apart in one int16 buffer: the source side is addressed with 64-bit offsets"""
    pn, ps, Cc, G, layout = geo("2d_aligned")
    size = (6, 10)
    n_el = size[0] * size[1] * Cc
    gap = 2 ** 31 + 16
    try:
        buf = torch.empty(gap + n_el, dtype=torch.int16, device=DEV)
    except (torch.OutOfMemoryError, RuntimeError) as e:
        pytest.skip(f"no {2 * (gap + n_el)} bytes of device memory: {e}")
    sig = samples((2, *size, Cc), Q.S16, seed=41)
    buf[:n_el] = sig[0].reshape(-1).to(DEV)
    buf[gap:] = sig[1].reshape(-1).to(DEV)
    view = torch.as_strided(buf, (2, *size, Cc), (gap, size[1] * Cc, Cc, 1))
    got = run_patch(view, layout, Q.S16)
    del view, buf
    assert np.array_equal(S.bits(got), S.bits(Q.targets(sig.numpy(), pn, ps, Q.S16, pad=True)))


# ---- rcb_recon_finish_fmt ------------------------------------------------------------------------------------------------------------
def inputs(name, fmt, kind, seed):
    """-> (y, t) [rows, P, C]: `random`, `special` (the format's ties, their neighbours, the ends of the range, -0 and +-inf among
    random values -- a random part of that set where the case is smaller -- and a NaN at the first sample of signal 1) or `dyadic`
    (inputs on which every term and every partial sum is exact: see the test that uses them)"""
    pn, ps, Cc, G, layout = geo(name)
    shape = (N * int(np.prod(pn)), int(np.prod(ps)), Cc)
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    t = rng.rand(*shape).astype(F32)
    if kind == "dyadic":
        y = E.dyadic(shape, seed) if fmt == Q.S16 else rng.choice(np.array([0.0, 1.0, -0.5, 2.0], dtype=F32), size=shape)
        return y, E.dyadic(shape, seed + 1)
    y = rng.uniform(-0.2, 1.2, size=n).astype(F32)
    if kind == "special":
        sp = Q.special_values(fmt)
        m = min(n, len(sp))
        y[rng.permutation(n)[:m]] = sp[rng.permutation(len(sp))[:m]]
        y.reshape(shape)[int(np.prod(pn)), 0, 0] = np.nan            # (patch 0, pixel 0: inside every extent)
    return y.reshape(shape), t


def run_finish(y, t, layout, size, fmt, shift=0, want_q=True, want_whole=True, old_mode=None):
    """ops.recon_finish(sample_format=) into outputs with a canary border (shift = 1: every output one element off its alignment), which
    must stay intact -> (q, whole, sse, n_bad) as numpy.  old_mode: the same call without a format, through the older entries"""
    Cc = y.shape[-1]
    per = int(np.prod(layout.patch_nums))
    shape = (y.shape[0] // per, *(size if size is not None else X.grid_of(layout.patch_nums, layout.patch_size)), Cc)
    qdt = torch.uint8 if fmt[0] < 2 else torch.int16
    qfill = 0xA5 if fmt[0] < 2 else QFILL
    bufs = [_bordered(shape, qdt, qfill, shift) if want_q and fmt[0] != 1 else (None, None),
            _bordered(shape, torch.float32, -7.5, shift) if want_whole else (None, None),
            _bordered((shape[0],), torch.float64, -7.5, shift), _bordered((shape[0],), torch.int32, -77, shift)]
    out = [v for _, v in bufs]
    if out[0] is not None and fmt[0] == 2:
        out[0] = out[0].view(torch.uint16)
    kw = dict(mode=old_mode) if old_mode is not None else dict(sample_format=sf(fmt))
    got = ops.recon_finish(dev(y), None if t is None else dev(t), layout=layout, size=size, out=tuple(out), **kw)
    torch.cuda.synchronize()
    for (buf, v), f in zip(bufs, (qfill, -7.5, -7.5, -77)):
        assert buf is None or _border_intact(buf, v.numel(), f, shift), "canary border overwritten"
    return tuple(None if g is None else g.cpu().numpy() for g in got)


def assert_matches(got, want, label):
    q, whole, sse, n_bad = got
    assert q.dtype == want["q"].dtype and np.array_equal(q, want["q"])
    assert whole.shape == want["whole"].shape and np.array_equal(S.bits(whole), S.bits(want["whole"]))
    assert np.array_equal(n_bad, want["n_bad"])
    fin = want["n_bad"] == 0
    assert np.isnan(sse[~fin]).all()
    err, bound = np.abs(sse - want["sse"])[fin], sse_bound(want["terms"])[fin]
    if fin.any():
        print(f"{label}: worst sse error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
        assert (err <= bound).all()


@pytest.mark.parametrize("fmt", FORMATS.values(), ids=FORMATS.keys())
@pytest.mark.parametrize("kind", ["random", "special"])
@pytest.mark.parametrize("name,size", ALL)
def test_finish_matches_the_evaluator(name, size, kind, fmt):
    """q_out and whole bit for bit, sse within the reordering bound, on aligned outputs (a quad of q is one 8-byte store where L % 4 == 0)
    and on outputs one element further on (element by element); with size = G the uncropped form gives the same"""
    pn, ps, Cc, G, layout = geo(name)
    y, t = inputs(name, fmt, kind, 1)
    want = Q.finish_whole(y, t, pn, ps, fmt, size=size)
    assert kind == "random" or (want["n_bad"][1] > 0 and np.isnan(want["sse"][1]))
    for shift in (0, 1):
        assert_matches(run_finish(y, t, layout, size, fmt, shift), want, f"{name} {size} {kind} shift {shift}")
    if tuple(size) == G:
        for shift in (0, 1):
            assert_matches(run_finish(y, t, layout, None, fmt, shift), want, f"{name} uncropped {kind} shift {shift}")


@pytest.mark.parametrize("fmt", EVERY, ids=lambda f: "s16" if f == Q.S16 else "u16_%d" % f[1])
def test_finish_of_every_tie_and_special_value(fmt):
    """rows that are datapoints (nd = 0 of the uncropped form): the whole tie set of the format, each value one ulp to either side, the
    ends of the range, -0.0 (v = +0.0), +-inf -- q and v bit for bit"""
    sp = Q.special_values(fmt)
    P = 37
    y = np.resize(sp, (-(-len(sp) // P), P, 1)).astype(F32)
    q, whole, _, n_bad = ops.recon_finish(dev(y), None, sample_format=sf(fmt), want_int=True, want_whole=True)
    wq, wv = Q.finish(y, fmt)
    assert q.dtype == sf(fmt).dtype and np.array_equal(q.cpu().numpy(), wq)
    assert np.array_equal(S.bits(whole.cpu().numpy()), S.bits(wv)) and not np.signbit(whole.cpu().numpy()).any()
    assert int(n_bad.sum()) == int((~np.isfinite(y)).sum()) > 0


@pytest.mark.parametrize("fmt", FORMATS.values(), ids=FORMATS.keys())
@pytest.mark.parametrize("name,size", ALL)
def test_sse_is_exact_on_dyadic_inputs(name, size, fmt):
    """s16: y and t multiples of 2^-6 in [-1, 1] -- v is c itself (65535 / 65536 for c = 1), d a multiple of 2^-16 below 2, d^2 a
    multiple of 2^-32 below 4, and fewer than 2^14 of them: 48 bits, every partial sum exact.  u16: y in {0, 1, -0.5, 2}, so v in
    {0, 1}, t as above: d a multiple of 2^-6.  The order of the additions cannot show: the sum is the evaluator's, bit for bit"""
    pn, ps, Cc, G, layout = geo(name)
    y, t = inputs(name, fmt, "dyadic", 3)
    want = Q.finish_whole(y, t, pn, ps, fmt, size=size)
    q, whole, sse, n_bad = run_finish(y, t, layout, size, fmt)
    assert np.array_equal(q, want["q"]) and np.array_equal(S.bits(whole), S.bits(want["whole"]))
    assert np.array_equal(sse.view(np.int64), want["sse"].view(np.int64)) and not n_bad.any()


@pytest.mark.parametrize("fmt", FORMATS.values(), ids=FORMATS.keys())
@pytest.mark.parametrize("name,size", [("1d", (9,)), ("2d", (7, 11)), ("2d", (8, 12)), ("2d_aligned", (6, 10)), ("3d", (2, 7, 5)),
                                       ("chunk", (8197,))])
def test_crop_sse_is_the_full_form_on_a_target_that_equals_v_outside(name, size, fmt):
    """bit for bit on arbitrary inputs, the statement of tests/test_hip_extent.py for the older modes: v = what the full form itself
    makes of y, put into the target at every position outside the extent, gives d = 0 there.  Also: a signal alone gives the bits it
    has inside the batch, and a second run the same bits"""
    pn, ps, Cc, G, layout = geo(name)
    f = sf(fmt)
    y, t = inputs(name, fmt, "random", 7)
    yd, td = dev(y), dev(t)
    _, v, _, _ = ops.recon_finish(yd, None, layout=None, sample_format=f, want_whole=True)
    m = torch.from_numpy(S.patch(X.inside(N, pn, ps, Cc, size), pn, ps)).to(DEV)
    _, _, want, want_bad = ops.recon_finish(yd, torch.where(m, td, v), layout=layout, sample_format=f)
    _, _, sse, n_bad = ops.recon_finish(yd, td, layout=layout, size=size, sample_format=f)
    assert torch.equal(sse.view(torch.int64), want.view(torch.int64)) and torch.equal(n_bad, want_bad)
    assert bool(torch.isfinite(sse).all()) and bool((sse > 0).all())
    assert torch.equal(ops.recon_finish(yd, td, layout=layout, size=size, sample_format=f)[2].view(torch.int64), sse.view(torch.int64))
    per = yd.shape[0] // N
    for d in range(N):
        alone = ops.recon_finish(yd[d * per:(d + 1) * per], td[d * per:(d + 1) * per], layout=layout, size=size, sample_format=f)[2]
        assert torch.equal(alone.view(torch.int64), sse[d:d + 1].view(torch.int64))


@pytest.mark.parametrize("fmt", FORMATS.values(), ids=FORMATS.keys())
@pytest.mark.parametrize("name,size", ALL)
def test_round_trip_of_16_bit_signals(name, size, fmt):
    """recon_finish(signal_patch_pad(q), size=) scored against itself returns the source words with sse 0"""
    pn, ps, Cc, G, layout = geo(name)
    q = samples((N, *size, Cc), fmt, seed=31)
    if fmt[0] == 2:
        q = torch.from_numpy(q.numpy() & np.uint16(Q.m_of(fmt)))           # the representable values
    y = ops.signal_patch_pad(q.to(DEV), layout, sample_format=sf(fmt))
    back, whole, sse, n_bad = ops.recon_finish(y, target=y, layout=layout, size=size, sample_format=sf(fmt), want_u8=True,
                                               want_whole=True)
    assert back.dtype == sf(fmt).dtype and np.array_equal(back.cpu().numpy(), q.numpy())
    assert np.array_equal(S.bits(whole.cpu().numpy()), S.bits(Q.to_target(q.numpy(), fmt)))
    assert sse.cpu().tolist() == [0.0] * N and n_bad.cpu().tolist() == [0] * N


# ---- the older kinds and modes through the new entries; the older entries as they were ------------------------------------------------
@pytest.mark.parametrize("fmt", [Q.U8, Q.F32FMT], ids=["u8", "f32"])
@pytest.mark.parametrize("name,size", [("1d", (9,)), ("2d", (7, 11)), ("2d", (8, 12)), ("2d_aligned", (6, 10)), ("3d", (2, 7, 5)),
                                       ("chunk", (8200,))])
def test_kinds_0_and_1_give_every_bit_of_the_older_entries(name, size, fmt):
    """signals: the padded and (size = G) uncropped forms, aligned and one element further on.  reconstructions: modes 0 and 1 on
    special inputs (-0.0 among them: mode 0 keeps its own zero), aligned and shifted outputs, cropped and (size = G) uncropped"""
    pn, ps, Cc, G, layout = geo(name)
    sig = samples((N, *size, Cc), fmt, seed=51)
    flat = sig.reshape(-1)
    shifted = torch.cat([flat[:1], flat]).to(DEV)[1:].view(N, *size, Cc)
    for view in (sig.to(DEV), shifted):
        for padded in (True, False) if tuple(size) == G else (True,):
            for guard in (64, 3):
                a = run_patch(view, layout, fmt, padded, guard, old=True)
                assert np.array_equal(S.bits(a), S.bits(run_patch(view, layout, fmt, padded, guard)))
    rows, P = N * int(np.prod(pn)), int(np.prod(ps))
    y = fill((rows, P, Cc), "special", 1)
    y.reshape(-1)[:3] = [-0.0, np.nan, np.inf]
    t = np.random.RandomState(2).rand(rows, P, Cc).astype(F32)
    for crop in (size, None) if tuple(size) == G else (size,):
        for shift in (0, 1):
            a = run_finish(y, t, layout, crop, fmt, shift, old_mode=fmt[0])
            b = run_finish(y, t, layout, crop, fmt, shift)
            assert (a[0] is None and b[0] is None and fmt[0] == 1) or np.array_equal(a[0], b[0])
            assert np.array_equal(S.bits(a[1]), S.bits(b[1])) and np.array_equal(a[2].view(np.int64), b[2].view(np.int64))
            assert np.array_equal(a[3], b[3])


def _p(v):
    return C.c_void_p(0 if v is None else v.data_ptr())


def _arr(v, ctype=C.c_int32):
    return None if v is None else (ctype * 4)(*(list(v) + [0] * (4 - len(v))))


def test_the_older_entries_still_refuse_kind_2_and_mode_2():
    lib = _lib.load()
    src = torch.zeros(1, 4, 4, dtype=torch.int16, device=DEV)
    y = torch.full((2, 2, 4), SENTINEL, device=DEV)
    st = _lib.stream_ptr()
    for kind in (2, 3):
        assert lib.rcb_signal_patch(_p(src), kind, 1, 1, _arr([2]), _arr([2]), 4, 16, _arr([4], C.c_int64), 1, _p(y), st) == -1
        assert b"source kind" in lib.rcb_last_error_string()
        assert lib.rcb_signal_patch_pad(_p(src), kind, 1, 1, _arr([2]), _arr([2]), _arr([3]), 4, 16, _arr([4], C.c_int64), 1, _p(y),
                                        st) == -1
        assert b"source kind" in lib.rcb_last_error_string()
    ws = torch.empty(1 << 12, device=DEV, dtype=torch.uint8)
    whole = torch.full((1, 4, 4), SENTINEL, device=DEV)
    for mode in (2, 3):
        assert lib.rcb_recon_finish(_p(y), None, 2, 2, 4, 1, _arr([2]), _arr([2]), mode, None, _p(whole), None, None, _p(ws),
                                    ws.numel(), st) == -1
        assert b"mode" in lib.rcb_last_error_string()
        assert lib.rcb_recon_finish_crop(_p(y), None, 2, 2, 4, 1, _arr([2]), _arr([2]), _arr([3]), mode, None, _p(whole), None, None,
                                         _p(ws), ws.numel(), st) == -1
        assert b"mode" in lib.rcb_last_error_string()
    torch.cuda.synchronize()
    assert (whole == SENTINEL).all() and (y == SENTINEL).all()
    with pytest.raises(RcbError, match="uint8 or fp32"):
        ops.signal_patch(src, ops.PeLayout([2], [2]))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _raw_patch(src, kind, depth, n_data, pn, ps, size, Cc, ds, strides, cs, y, nd=None):
    nd = len(pn) if nd is None else nd
    return _lib.load().rcb_signal_patch_fmt(src, kind, depth, n_data, nd, _arr(pn), _arr(ps), _arr(size), Cc, ds,
                                            _arr(strides, C.c_int64), cs, y, _lib.stream_ptr())


def test_refusals_of_signal_patch_fmt():
    """an unknown kind, a depth outside 9 .. 16 for u16, a depth for any other kind, and what the older entries refuse: RCB_ERR_* with a
    message, nothing launched (y keeps its sentinel); valid calls of either form follow"""
    src = torch.arange(9, dtype=torch.int16, device=DEV).view(1, 3, 3)
    y = torch.full((2, 2, 3), SENTINEL, device=DEV)
    sp, yp = _p(src), _p(y)
    base = dict(src=sp, kind=2, depth=12, n_data=1, pn=[2], ps=[2], size=[3], Cc=3, ds=9, strides=[3], cs=1, y=yp)
    refused = {
        "kind 4": dict(kind=4, depth=0), "kind -1": dict(kind=-1, depth=0),
        "depth 8": dict(depth=8), "depth 17": dict(depth=17), "depth 0 for u16": dict(depth=0), "depth -1": dict(depth=-1),
        "depth for u8": dict(kind=0, depth=8), "depth for f32": dict(kind=1, depth=12), "depth for s16": dict(kind=3, depth=16),
        "nd 0": dict(nd=0), "nd 4": dict(pn=[1, 1, 1, 2], ps=[1, 1, 1, 2], size=[1, 1, 1, 3], strides=[0, 0, 0, 3]),
        "33 channels": dict(Cc=33), "no channels": dict(Cc=0), "no patches": dict(pn=[0]), "negative patch size": dict(ps=[-2]),
        "size above the grid": dict(size=[5]), "size 0": dict(size=[0]), "negative axis stride": dict(strides=[-3]),
        "negative signal stride": dict(ds=-9), "negative channel stride": dict(cs=-1), "null src": dict(src=None), "null y": dict(y=None),
        "negative n_data": dict(n_data=-1), "null geometry": dict(pn=None, nd=1),
        "2^31 elements per signal": dict(pn=[1 << 15], ps=[1 << 15], size=[3], Cc=2),
    }
    lib = _lib.load()
    for what, change in refused.items():
        rc = _raw_patch(**dict(base, **change))
        assert rc < 0, what
        assert len(lib.rcb_last_error_string()) > 10, what
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()
    assert _raw_patch(**dict(base, src=None, y=None, n_data=0)) == 0                  # no signals: nothing to address
    assert _raw_patch(**base) == 0                                                     # the padded form
    assert np.array_equal(S.bits(y.cpu().numpy()), S.bits(Q.targets(src.cpu().numpy().view(np.uint16), [2], [2], Q.u16(12), pad=True)))
    src4 = torch.arange(-6, 6, dtype=torch.int16, device=DEV).view(1, 4, 3)
    assert _raw_patch(**dict(base, src=_p(src4), kind=3, depth=0, size=None, ds=12)) == 0      # the uncropped form: a null size
    assert np.array_equal(S.bits(y.cpu().numpy()), S.bits(Q.targets(src4.cpu().numpy(), [2], [2], Q.S16)))
    z = lambda *shape, dtype=torch.int16: torch.zeros(*shape, dtype=dtype, device=DEV)   # noqa: E731
    lay = ops.PeLayout([2], [2])
    for text, call in [
        ("reads torch.int16", lambda: ops.signal_patch(z(1, 4, 3, dtype=torch.uint8), lay, sample_format=SampleFormat.s16())),
        ("reads torch.uint16", lambda: ops.signal_patch(z(1, 4, 3, dtype=torch.float32), lay, sample_format=SampleFormat.u16(10))),
        ("reads torch.uint8", lambda: ops.signal_patch_pad(z(1, 3, 3), lay, sample_format=SampleFormat.u8())),
        ("reads torch.int16", lambda: ops.signal_patch(z(1, 4, 3).view(torch.uint16), lay, sample_format=SampleFormat.s16())),
        ("uint8 or fp32", lambda: ops.signal_patch_pad(z(1, 3, 3), lay)),
        ("GPU tensor", lambda: ops.signal_patch(torch.zeros(1, 4, 3, dtype=torch.int16), lay, sample_format=SampleFormat.s16())),
        ("the layout's is", lambda: ops.signal_patch(z(1, 5, 3), lay, sample_format=SampleFormat.s16())),
        ("positions", lambda: ops.signal_patch_pad(z(1, 5, 3), lay, sample_format=SampleFormat.s16())),
        ("output of shape", lambda: ops.signal_patch(z(1, 4, 3), lay, out=torch.zeros(2, 2, 4, device=DEV), sample_format=SampleFormat.s16())),
    ]:
        with pytest.raises(RcbError, match=text):
            call()
    assert tuple(ops.signal_patch_pad(z(0, 3, 3), lay, sample_format=SampleFormat.s16()).shape) == (0, 2, 3)


def _raw_finish(y, t, n_rows, P, Cc, nd, pn, ps, size, mode, depth, q, whole, sse, n_bad, ws):
    return _lib.load().rcb_recon_finish_fmt(_p(y), _p(t), n_rows, P, Cc, nd, _arr(pn), _arr(ps), _arr(size), mode, depth, _p(q),
                                            _p(whole), _p(sse), _p(n_bad), _p(ws), 0 if ws is None else ws.numel(), _lib.stream_ptr())


def test_refusals_of_recon_finish_fmt():
    """an unknown mode, a depth outside 9 .. 16 for mode 2, a depth for any other mode, q_out with mode 1, and what the older entries
    refuse: RCB_ERR_* with a message before anything is launched (the outputs and their canary borders keep their fill); then the
    errors of ops.recon_finish(sample_format=)"""
    pn, ps, Cc, rows, P, size = (2, 3), (4, 5), 3, 12, 20, (7, 11)
    y, t = dev(fill((rows, P, Cc), "random", 1)), dev(fill((rows, P, Cc), "random", 2))
    shape = (2, *size, Cc)
    fills = (QFILL, -7.5, -7.5, -77)
    bufs = [_bordered(shape, torch.int16, QFILL), _bordered(shape, torch.float32, -7.5), _bordered((2,), torch.float64, -7.5),
            _bordered((2,), torch.int32, -77)]
    q, whole, sse, n_bad = (v for _, v in bufs)
    ws = torch.empty(1 << 16, device=DEV, dtype=torch.uint8)
    lib = _lib.load()
    base = dict(y=y, t=t, n_rows=rows, P=P, Cc=Cc, nd=2, pn=pn, ps=ps, size=size, mode=2, depth=12, q=q, whole=whole, sse=sse,
                n_bad=n_bad, ws=ws)
    assert _raw_finish(**base) == 0 and _raw_finish(**dict(base, mode=3, depth=0)) == 0      # (the valid calls, for contrast)
    torch.cuda.synchronize()
    assert float(sse[0]) != -7.5
    for (_, v), f in zip(bufs, fills):
        v.fill_(f)
    refused = {
        "mode 4": dict(mode=4, depth=0), "mode -1": dict(mode=-1, depth=0),
        "depth 8": dict(depth=8), "depth 17": dict(depth=17), "depth 0 for u16": dict(depth=0),
        "depth for mode 0": dict(mode=0, depth=8), "depth for mode 1": dict(mode=1, depth=12, q=None),
        "depth for mode 3": dict(mode=3, depth=16),
        "q_out with mode 1": dict(mode=1, depth=0),
        "size above the grid": dict(size=(9, 11)), "size 0": dict(size=(0, 11)),
        "nd = 0 with a size": dict(nd=0, pn=(), ps=(), size=()),
        "nd > 3": dict(nd=4, pn=(1, 1, 2, 3), ps=(1, 1, 4, 5), size=(1, 1, 7, 11)),
        "C = 0": dict(Cc=0), "C = 33": dict(Cc=33), "P != prod(patch_size)": dict(ps=(4, 4)),
        "rows no multiple of prod(patch_nums)": dict(n_rows=11), "sse without target": dict(t=None),
        "2^31 elements per stitched datapoint": dict(pn=(1 << 15, 1 << 14), ps=(4, 5), n_rows=1 << 29),
        "workspace too small": dict(ws=ws[:8]), "null y": dict(y=None), "null patch geometry": dict(pn=None),
    }
    for what, change in refused.items():
        rc = _raw_finish(**dict(base, **change))
        assert rc < 0, what
        assert len(lib.rcb_last_error_string()) > 10, what
    torch.cuda.synchronize()
    for (buf, _), f in zip(bufs, fills):
        assert bool((buf == f).all()), "something was launched"
    lay = ops.PeLayout(pn, ps)
    f12, s16 = SampleFormat.u16(12), SampleFormat.s16()
    calls = {
        "integers of the f32 format": lambda: ops.recon_finish(y, t, layout=lay, sample_format=SampleFormat.f32(), want_int=True),
        "uint8 output for s16": lambda: ops.recon_finish(y, t, layout=lay, sample_format=s16,
                                                         out=(torch.empty(2, 8, 15, 3, device=DEV, dtype=torch.uint8), None, None, None)),
        "int16 output for u16": lambda: ops.recon_finish(y, t, layout=lay, sample_format=f12,
                                                         out=(torch.empty(2, 8, 15, 3, device=DEV, dtype=torch.int16), None, None, None)),
        "size above the grid": lambda: ops.recon_finish(y, t, layout=lay, size=(9, 11), sample_format=f12),
        "size without a layout": lambda: ops.recon_finish(y, t, size=size, sample_format=s16),
        "rows no multiple": lambda: ops.recon_finish(y[:11], t[:11], layout=lay, size=size, sample_format=s16),
        "cpu tensor": lambda: ops.recon_finish(y.cpu(), None, layout=lay, sample_format=s16),
    }
    for what, call in calls.items():
        with pytest.raises(RcbError):
            call()
            pytest.fail(what)
    got = ops.recon_finish(y, t, layout=lay, size=size, sample_format=f12, want_int=True)
    assert got[0].dtype == torch.uint16 and tuple(got[0].shape) == shape and got[1] is None and got[2].shape == (2,)
    assert ops.RECON_U16 == 2 and ops.RECON_S16 == 3
