"""rcb_signal_patch_ragged / rcb_recon_finish_ragged (N4 413) against the per-signal evaluator (tests/ragged_emul.py) and against the
entries they generalise: every comparison of floating-point data is bit for bit, through an int32 view."""
import ctypes as C

import numpy as np
import pytest
import torch

import ragged_emul as R
import sample16_emul as Q
import signal_emul as S

pytestmark = pytest.mark.gpu

from recombiner_amd import _lib, ops  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

DEV = "cuda"
FMTS = {"u8": Q.U8, "f32": Q.F32FMT, "u16_12": Q.u16(12), "s16": Q.S16}
GEOS = {1: ((3,), (4,)), 2: ((2, 3), (4, 4)), 3: ((1, 2, 2), (2, 4, 4))}
SIZES = {1: [(12,), (9,), (8,), (1,)], 2: [(8, 12), (7, 11), (5, 4), (1, 1), (8, 1)], 3: [(2, 8, 8), (2, 7, 5), (1, 8, 8), (1, 1, 3)]}
# name -> (patch_nums, patch_size): one chunk; E = 9216 with C = 3, two chunks; E = 105, no multiple of 4 (the element path only)
MIX_GEOS = {"one_chunk": ((2, 3), (8, 8)), "two_chunks": ((3, 4), (16, 16)), "odd": ((1, 1), (5, 7))}
SENT = -7.25


def _rand(fmt, shape, rng):
    if fmt[0] == 1:
        a = rng.rand(*shape).astype(np.float32)
        a.reshape(-1)[::7] = np.float32(-0.0)                  # bits that only an integer move keeps
        return a
    lo, hi = (-32768, 32768) if fmt[0] == 3 else (0, 256 if fmt[0] == 0 else Q.m_of(fmt) + 1)
    return rng.randint(lo, hi, size=shape).astype(Q.np_dtype(fmt))


def _bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.int32)


def _guarded(shape, pad=32):
    """a contiguous fp32 tensor of `shape` inside a larger buffer of sentinels -> (tensor, check())"""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * pad,), SENT, device=DEV)

    def check():
        assert bool((big[:pad] == SENT).all().item()) and bool((big[pad + n:] == SENT).all().item())
    return big[pad:pad + n].view(shape), check


# ---- targets --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("kind", list(FMTS))
@pytest.mark.parametrize("nd", [1, 2, 3])
def test_targets_of_mixed_sizes(nd, kind, Cc):
    fmt, (pn, ps) = FMTS[kind], GEOS[nd]
    rng = np.random.RandomState(nd * 10 + Cc)
    sigs = [_rand(fmt, (*s, Cc), rng) for s in SIZES[nd]]
    per, P = int(np.prod(pn)), int(np.prod(ps))
    out, check = _guarded((len(sigs) * per, P, Cc))
    y = ops.signal_patch_ragged([torch.from_numpy(a).to(DEV) for a in sigs], ops.PeLayout(pn, ps), out=out, sample_format=SampleFormat(*fmt))
    assert y is out and np.array_equal(_bits(y), _bits(R.targets(sigs, pn, ps, fmt)))
    check()


@pytest.mark.parametrize("kind", ["u8", "f32", "s16"])
@pytest.mark.parametrize("geo", list(MIX_GEOS))
def test_targets_of_mixed_layouts_in_one_call(geo, kind):
    """a signal that fills the grid, one with a single position on an axis, a transposed, a channel-first and an expanded-channel
    one, one on the vector path and one misaligned by one element -- in one call, each the existing entry's rows bit for bit"""
    fmt, (pn, ps), Cc = FMTS[kind], MIX_GEOS[geo], 3
    f = SampleFormat(*fmt)
    G = tuple(a * b for a, b in zip(pn, ps))
    rng = np.random.RandomState(11)
    t = lambda a: torch.from_numpy(a).to(DEV)                  # noqa: E731
    full = t(_rand(fmt, (*G, Cc), rng))
    thin = t(_rand(fmt, (1, max(G[1] - 3, 1), Cc), rng))
    transposed = t(_rand(fmt, (G[1] - 1, G[0] - 2, Cc), rng)).transpose(0, 1)
    chan_first = t(_rand(fmt, (Cc, G[0] - 1, G[1]), rng)).movedim(0, -1)
    expanded = t(_rand(fmt, (G[0], G[1] - 2, 1), rng)).expand(G[0], G[1] - 2, Cc)
    vec = t(_rand(fmt, (G[0] - 1, 4 * max(G[1] // 4 - 1, 1), Cc), rng))
    flat = t(_rand(fmt, (1 + (G[0] - 1) * G[1] * Cc,), rng))
    off_by_one = flat[1:].view(G[0] - 1, G[1], Cc)
    sigs = [full, thin, transposed, chan_first, expanded, vec, off_by_one]
    per, P = int(np.prod(pn)), int(np.prod(ps))
    out, check = _guarded((len(sigs) * per, P, Cc))
    y = ops.signal_patch_ragged(sigs, ops.PeLayout(pn, ps), out=out, sample_format=f)
    check()
    assert np.array_equal(_bits(y), _bits(R.targets([s.cpu().numpy() for s in sigs], pn, ps, fmt)))
    for k, s in enumerate(sigs):                               # against the existing entry, signal by signal
        one = ops.signal_patch_pad(s[None], ops.PeLayout(pn, ps), sample_format=f)
        assert torch.equal(y[k * per:(k + 1) * per].view(torch.int32), one.view(torch.int32)), k


def test_a_batch_of_equal_sizes_is_the_batched_entry():
    pn, ps, Cc = (2, 3), (8, 8), 3
    batch = torch.from_numpy(_rand(Q.U8, (4, 13, 21, Cc), np.random.RandomState(2))).to(DEV)
    y = ops.signal_patch_ragged(list(batch), ops.PeLayout(pn, ps))
    assert torch.equal(y.view(torch.int32), ops.signal_patch_pad(batch, ops.PeLayout(pn, ps)).view(torch.int32))


def test_a_signal_past_2_to_the_31_elements():
    pn, ps, Cc = (2, 3), (8, 8), 3
    buf = torch.empty(2 ** 31 + 4096, device=DEV, dtype=torch.uint8)
    rng = np.random.RandomState(5)
    a, b = _rand(Q.U8, (16, 20, Cc), rng), _rand(Q.U8, (15, 24, Cc), rng)
    lo, hi = buf[64:64 + a.size].view(a.shape), buf[2 ** 31 + 5:2 ** 31 + 5 + b.size].view(b.shape)
    lo.copy_(torch.from_numpy(a))
    hi.copy_(torch.from_numpy(b))
    y = ops.signal_patch_ragged([hi, lo], ops.PeLayout(pn, ps))
    assert np.array_equal(_bits(y), _bits(R.targets([b, a], pn, ps, Q.U8)))


# ---- reconstructions ------------------------------------------------------------------------------------------------------------
def _recon_case(geo, fmt, seed=6):
    (pn, ps), Cc = MIX_GEOS[geo], 3
    G = tuple(a * b for a, b in zip(pn, ps))
    sizes = [G, (1, max(G[1] - 3, 1)), (G[0] - 1, 4 * max(G[1] // 4 - 1, 1)), (max(G[0] - 2, 1), G[1] - 1), (G[0], 1)]
    swaps = [False, False, False, True, True]
    rng = np.random.RandomState(seed)
    per, P = int(np.prod(pn)), int(np.prod(ps))
    y = (rng.rand(len(sizes) * per, P, Cc) * 1.2 - 0.1).astype(np.float32)
    t = rng.rand(len(sizes) * per, P, Cc).astype(np.float32)
    return pn, ps, Cc, sizes, swaps, y, t


@pytest.mark.parametrize("geo,kind", [("one_chunk", "u8"), ("one_chunk", "f32"), ("one_chunk", "u16_12"), ("one_chunk", "s16"),
                                      ("two_chunks", "u8"), ("two_chunks", "s16"), ("odd", "u8"), ("odd", "u16_12")])
def test_finish_of_mixed_sizes(geo, kind):
    fmt = FMTS[kind]
    f = SampleFormat(*fmt)
    pn, ps, Cc, sizes, swaps, y, t = _recon_case(geo, fmt)
    lay, per = ops.PeLayout(pn, ps), int(np.prod(pn))
    want = R.finish(y, t, pn, ps, fmt, sizes, swaps)
    yd, td = torch.from_numpy(y).to(DEV), torch.from_numpy(t).to(DEV)
    q, whole, sse, n_bad = ops.recon_finish_ragged(yd, td, layout=lay, sizes=sizes, swap=swaps, sample_format=f,
                                                   want_int=f.is_integer, want_whole=True)
    for k in range(len(sizes)):
        assert whole[k].is_contiguous() and tuple(whole[k].shape) == want["whole"][k].shape
        assert np.array_equal(_bits(whole[k]), _bits(want["whole"][k])), k
        if f.is_integer:
            assert q[k].dtype == f.dtype and np.array_equal(q[k].cpu().numpy(), want["q"][k]), k
    assert q is not None or not f.is_integer
    assert not n_bad.any().item()
    # sse[k]: bitwise the existing entry's for that signal alone; the evaluator's correctly rounded sum within the order of additions
    alone = torch.stack([ops.recon_finish(yd[k * per:(k + 1) * per], td[k * per:(k + 1) * per], layout=lay, size=sizes[k],
                                          sample_format=f)[2][0] for k in range(len(sizes))])
    assert torch.equal(sse.view(torch.int64), alone.view(torch.int64))
    E_pad = per * int(np.prod(ps)) * Cc
    assert np.all(np.abs(sse.cpu().numpy() - want["sse"]) <= E_pad * 2.0 ** -53 * np.maximum(want["sse"], 1e-300) * 1.01)
    # ... and in any batch order
    perm = [3, 0, 4, 2, 1]
    rows = torch.cat([torch.arange(k * per, (k + 1) * per) for k in perm]).to(DEV)
    _, _, sse_p, _ = ops.recon_finish_ragged(yd[rows].contiguous(), td[rows].contiguous(), layout=lay, sizes=[sizes[k] for k in perm],
                                             swap=[swaps[k] for k in perm], sample_format=f)
    assert torch.equal(sse_p.view(torch.int64), sse[perm].view(torch.int64))


@pytest.mark.parametrize("kind", ["u8", "s16"])
def test_finish_leaves_everything_outside_the_spans_untouched(kind):
    fmt = FMTS[kind]
    f = SampleFormat(*fmt)
    pn, ps, Cc, sizes, swaps, y, t = _recon_case("one_chunk", fmt)
    spans, shapes, _ = ops._ragged_spans(sizes, swaps, Cc)
    gaps = [8, 3, 4, 1, 6]                                    # between and before the spans: aligned and misaligned starts
    shift, total = 0, 0
    for sp, shp, g in zip(spans, shapes, gaps):
        shift += g
        sp[0] += shift
        total = sp[0] + int(np.prod(shp)) + 5
    wbuf = torch.full((total,), SENT, device=DEV)
    qbuf = torch.full((total,), 77, device=DEV, dtype=f.dtype)
    ops.recon_finish_ragged_into(torch.from_numpy(y).to(DEV), torch.from_numpy(t).to(DEV), ops.PeLayout(pn, ps), sizes, spans, total,
                                 mode=f.kind, depth=f.depth, q_buf=qbuf, whole_buf=wbuf)
    want = R.finish(y, t, pn, ps, fmt, sizes, swaps)
    wref, qref = np.full(total, SENT, dtype=np.float32), np.full(total, 77, dtype=Q.np_dtype(fmt))
    for sp, k in zip(spans, range(len(sizes))):
        n = want["whole"][k].size
        wref[sp[0]:sp[0] + n] = want["whole"][k].reshape(-1)
        qref[sp[0]:sp[0] + n] = want["q"][k].reshape(-1)
    assert np.array_equal(_bits(wbuf), _bits(wref)) and np.array_equal(qbuf.cpu().numpy(), qref)


def test_a_nan_counts_only_inside_its_signals_extent():
    fmt = Q.U8
    pn, ps, Cc, sizes, swaps, y, t = _recon_case("one_chunk", fmt)
    lay, per = ops.PeLayout(pn, ps), int(np.prod(pn))
    yd, td = torch.from_numpy(y).to(DEV), torch.from_numpy(t).to(DEV)
    _, _, sse, _ = ops.recon_finish_ragged(yd, td, layout=lay, sizes=sizes, swap=swaps)
    import recon_emul as E
    whole = E.stitch(y.copy(), pn, ps)
    s2 = sizes[2]                                              # signal 2 is smaller than the grid on both axes
    whole[2, s2[0], 0, 1] = np.nan                             # padding: the row below the extent
    whole[2, 0, s2[1], 0] = np.inf                             # padding: the column right of it
    _, _, sse_pad, bad_pad = ops.recon_finish_ragged(torch.from_numpy(S.patch(whole, pn, ps)).to(DEV), td, layout=lay, sizes=sizes, swap=swaps)
    assert torch.equal(sse_pad.view(torch.int64), sse.view(torch.int64)) and not bad_pad.any().item()
    whole[2, s2[0] - 1, s2[1] - 1, 2] = np.nan                 # the last real sample
    _, _, sse_in, bad_in = ops.recon_finish_ragged(torch.from_numpy(S.patch(whole, pn, ps)).to(DEV), td, layout=lay, sizes=sizes, swap=swaps)
    keep = [0, 1, 3, 4]
    assert torch.isnan(sse_in[2]).item() and bad_in.cpu().tolist() == [0, 0, 1, 0, 0]
    assert torch.equal(sse_in[keep].view(torch.int64), sse[keep].view(torch.int64))


@pytest.mark.parametrize("fmt", [Q.U8, Q.u16(9), Q.u16(16), Q.S16])
def test_round_trip_gives_the_integers_back_in_their_orientation(fmt):
    f = SampleFormat(*fmt)
    pn, ps, Cc = (2, 3), (8, 8), 3
    rng = np.random.RandomState(9)
    mem = [_rand(fmt, s, rng) for s in ((16, 24, Cc), (13, 21, Cc), (20, 9, Cc), (1, 1, Cc), (24, 16, Cc))]       # two portraits
    swaps = [a.shape[0] > a.shape[1] for a in mem]
    assert swaps == [False, False, True, False, True]
    dev = [torch.from_numpy(a).to(DEV) for a in mem]
    cut = [d.transpose(0, 1) if sw else d for d, sw in zip(dev, swaps)]
    lay = ops.PeLayout(pn, ps)
    y = ops.signal_patch_ragged(cut, lay, sample_format=f)
    q, _, sse, n_bad = ops.recon_finish_ragged(y, y, layout=lay, sizes=[tuple(c.shape[:-1]) for c in cut], swap=swaps, sample_format=f,
                                               want_int=True)
    for a, got in zip(mem, q):
        assert got.is_contiguous() and tuple(got.shape) == a.shape and np.array_equal(got.cpu().numpy(), a)
    assert not sse.any().item() and not n_bad.any().item()


# ---- refusals: on the host, nothing launched ------------------------------------------------------------------------------------
def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def _tables(sizes, spans):
    sz, sp = np.zeros((len(sizes), 3), np.int32), np.zeros((len(sizes), 4), np.int64)
    for k, (s, p) in enumerate(zip(sizes, spans)):
        sz[k, :len(s)] = s
        sp[k, :len(p)] = p
    return sz, sp


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


GOOD_SIZES, GOOD_SRC_SPANS = [(16, 24), (13, 21)], [(0, 72, 3), (1152, 63, 3)]


def _patch_call(sizes=GOOD_SIZES, spans=GOOD_SRC_SPANS, src_elems=1152 + 13 * 63, null=(), table_bytes=None, kind=0, depth=0, n=2):
    lib = _lib.load()
    src = torch.zeros(4096, device=DEV, dtype=torch.uint8)
    y, check = _guarded((n * 6, 64, 3))
    before = y.clone()
    table = torch.full((256,), 0x5A, device=DEV, dtype=torch.uint8)
    sz, sp = _tables(sizes, spans)
    need = lib.rcb_ragged_table_bytes(n)
    rc = lib.rcb_signal_patch_ragged(_ptr(src), src_elems, kind, depth, n, 2, _i32(2, 3, 0), _i32(8, 8, 0),
                                     None if "sizes" in null else _ptr(sz), None if "spans" in null else _ptr(sp), 3, 1, _ptr(y),
                                     None if "table" in null else _ptr(table), need if table_bytes is None else table_bytes,
                                     ops.stream_ptr())
    torch.cuda.synchronize()
    untouched = torch.equal(y.view(torch.int32), before.view(torch.int32)) and bool((table == 0x5A).all().item())
    check()
    return rc, untouched


def test_patch_refusals():
    lib = _lib.load()
    assert lib.rcb_ragged_table_bytes(0) == 0 and lib.rcb_ragged_table_bytes(-1) == -1 and lib.rcb_ragged_table_bytes(3) % 8 == 0
    rc, untouched = _patch_call()
    assert rc == 0 and not untouched                           # the call the refusals below are one step away from
    bad = [dict(sizes=[(17, 24), (13, 21)]), dict(sizes=[(16, 24), (0, 21)]), dict(sizes=[(16, 25), (13, 21)]),
           dict(spans=[(0, 72, 3), (1152, -63, 3)]), dict(spans=[(-1, 72, 3), (1152, 63, 3)]),
           dict(src_elems=1152 + 13 * 63 - 1), dict(src_elems=0), dict(spans=[(0, 72, 3), (1152, 2 ** 61, 3)]),
           dict(null=("sizes",)), dict(null=("spans",)), dict(null=("table",)),
           dict(table_bytes=lib.rcb_ragged_table_bytes(2) - 1), dict(table_bytes=0),
           dict(kind=4), dict(kind=2, depth=8), dict(kind=0, depth=9)]
    for kw in bad:
        rc, untouched = _patch_call(**kw)
        assert rc < 0 and untouched, kw
        assert lib.rcb_last_error_string()
    rc, untouched = _patch_call(n=0, null=("sizes", "spans", "table"), sizes=[], spans=[])
    assert rc == 0 and untouched                               # no signals: succeeds, launches nothing


GOOD_OUT_SPANS = [(0, 72, 3), (1152, 63, 3)]                  # dense [16, 24, 3] and [13, 21, 3]


def _finish_call(sizes=GOOD_SIZES, spans=GOOD_OUT_SPANS, out_elems=1152 + 13 * 63, null=(), table_bytes=None, mode=0, depth=0,
                 n_rows=12):
    lib = _lib.load()
    y = torch.rand(max(n_rows, 1), 64, 3, device=DEV)
    n = n_rows // 6
    whole, check = _guarded((2048,))
    before = whole.clone()
    q = torch.full((2048,), 77, device=DEV, dtype=torch.uint8)
    sse = torch.full((2,), SENT, device=DEV, dtype=torch.float64)
    n_bad = torch.full((2,), -5, device=DEV, dtype=torch.int32)
    table = torch.full((256,), 0x5A, device=DEV, dtype=torch.uint8)
    n_ws = max(int(lib.rcb_recon_workspace_bytes(max(n, 1), 6 * 64 * 3)), 8)
    ws = torch.zeros(n_ws, device=DEV, dtype=torch.uint8)
    sz, sp = _tables(sizes, spans)
    need = lib.rcb_ragged_table_bytes(n)
    rc = lib.rcb_recon_finish_ragged(_ptr(y), _ptr(y), n_rows, 64, 3, 2, _i32(2, 3, 0), _i32(8, 8, 0),
                                     None if "sizes" in null else _ptr(sz), None if "spans" in null else _ptr(sp), out_elems, mode,
                                     depth, None if mode == 1 else _ptr(q), _ptr(whole), _ptr(sse), _ptr(n_bad), _ptr(ws), n_ws,
                                     None if "table" in null else _ptr(table), need if table_bytes is None else table_bytes,
                                     ops.stream_ptr())
    torch.cuda.synchronize()
    untouched = (torch.equal(whole.view(torch.int32), before.view(torch.int32)) and bool((q == 77).all().item())
                 and bool((table == 0x5A).all().item()) and bool((sse == SENT).all().item()) and bool((n_bad == -5).all().item()))
    check()
    return rc, untouched


def test_finish_refusals():
    lib = _lib.load()
    rc, untouched = _finish_call()
    assert rc == 0 and not untouched
    rc, _ = _finish_call(spans=[(0, 3, 48), (1152, 63, 3)])    # a transposed dense signal is accepted
    assert rc == 0
    bad = [dict(sizes=[(17, 24), (13, 21)]), dict(sizes=[(16, 24), (13, 0)]),
           dict(spans=[(0, 72, 3), (1152, -63, 3)]), dict(spans=[(-4, 72, 3), (1152, 63, 3)]),
           dict(spans=[(0, 72, 3), (1151, 63, 3)]),            # overlapping spans
           dict(spans=[(0, 72, 3), (0, 63, 3)]),
           dict(spans=[(0, 75, 3), (1152, 63, 3)]),            # rows with a gap: not dense
           dict(spans=[(0, 72, 4), (1152, 63, 3)]), dict(spans=[(0, 72, 1), (1152, 63, 3)]), dict(spans=[(0, 3, 3), (1152, 63, 3)]),
           dict(out_elems=1152 + 13 * 63 - 1),                 # a span past the output
           dict(spans=[(0, 72, 3), (2 ** 40, 63, 3)]), dict(out_elems=-1),
           dict(null=("sizes",)), dict(null=("spans",)), dict(null=("table",)),
           dict(table_bytes=lib.rcb_ragged_table_bytes(2) - 1),
           dict(mode=4), dict(mode=2, depth=17), dict(mode=0, depth=12), dict(n_rows=13)]
    for kw in bad:
        rc, untouched = _finish_call(**kw)
        assert rc < 0 and untouched, kw
    rc, untouched = _finish_call(n_rows=0, sizes=[], spans=[], null=("sizes", "spans", "table"))
    assert rc == 0 and untouched
