"""rcb_recon_regions (N4 417: the squared error per region -- per frame, per patch, per tile -- on the device) against the numpy
evaluator tests/region_emul.py, whose premises tests/test_region_emul_cpu.py checks: bit for bit on dyadic inputs, within the
a-priori reordering bound in the rounding modes, the defining identity against ops.recon_finish device against device, bit identity
alone / in a batch / run to run / on either memory path, the locality of bad elements and of padding, guard words, refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import extent_emul as X
import recon_emul as E
import region_emul as R
import sample16_emul as K

pytestmark = pytest.mark.gpu

from recombiner_amd import _lib, ops, utils  # noqa: E402

DEV = "cuda"
F32 = np.float32
NAMES = list(R.CASES)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def geo(name):
    pn, ps, Cc, sizes, regions = R.CASES[name]
    return pn, ps, Cc, sizes, regions, ops.PeLayout(pn, ps)


def fmt_of(fmt):
    return utils.SampleFormat(*fmt)


def fill(shape, kind, seed, fmt):
    """uniform values a little beyond [0, 1]; "special": with the format's ties, their neighbours and the ends of the range (+-inf
    among them: bad elements) scattered over them"""
    rng = np.random.RandomState(seed)
    a = rng.uniform(-0.2, 1.2, size=shape).astype(F32)
    if kind == "special":
        if fmt[0] >= 2:
            sp = K.special_values(fmt)
        else:
            x, _ = E.tie_inputs()
            sp = np.concatenate([x, np.nextafter(x, F32(0)), np.nextafter(x, F32(1)), np.array([-0.0, 0.0, 1.0, np.inf, -np.inf], dtype=F32)])
        flat = a.reshape(-1)
        m = min(flat.size // 2, len(sp))
        flat[rng.permutation(flat.size)[:m]] = sp[rng.permutation(len(sp))[:m]]
    return a


def check_against_evaluator(got_sse, got_bad, want, what):
    """n_bad_r exactly; sse_r NaN exactly where the evaluator's is; elsewhere |sse_r - fsum| <= n_r * 2^-53 * sum(terms)"""
    got_sse, got_bad = got_sse.cpu().numpy(), got_bad.cpu().numpy()
    assert got_sse.shape == want["sse_r"].shape and got_sse.dtype == np.float64 and got_bad.dtype == np.int32
    assert np.array_equal(got_bad, want["n_bad_r"]), what
    assert np.array_equal(np.isnan(got_sse), want["n_bad_r"] > 0), what
    worst = 0.0
    for key, tm in want["terms"].items():
        if want["n_bad_r"][key] == 0:
            bound = tm.size * 2.0 ** -53 * float(tm.sum())
            err = abs(got_sse[key] - want["sse_r"][key])
            assert err <= bound, (what, key, err, bound)
            worst = max(worst, err / bound if bound else 0.0)
    return worst


# ---- bit for bit on dyadic inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_dyadic_sums_are_exact(name):
    pn, ps, Cc, sizes, regions, layout = geo(name)
    y, t = R.inputs(pn, ps, Cc, 3, kind="dyadic")
    yd, td = dev(y), dev(t)
    for size in sizes:
        for region in regions:
            want = R.finish_regions(y, t, pn, ps, region, fmt=K.F32FMT, size=size)
            sse_r, n_bad_r = ops.recon_regions(yd, td, layout, region, mode=ops.RECON_RAW, size=size)
            assert tuple(sse_r.shape) == want["sse_r"].shape, (size, region)
            assert torch.equal(sse_r.cpu(), torch.from_numpy(want["sse_r"])), (size, region)
            assert int(n_bad_r.abs().sum()) == 0


def test_dyadic_many_chunks_and_the_datapoints_own_sum():
    """one region covering an unpatched signal of 257 chunks (the `t, t + 256` leg of the reduce): exact, and -- the one case where
    the two orders coincide -- the bits of ops.recon_finish's sse for the datapoint"""
    pn, ps, Cc, size, region = R.MANY
    layout = ops.PeLayout(pn, ps)
    y, t = R.inputs(pn, ps, Cc, 5, n_data=2, kind="dyadic")
    want = R.finish_regions(y, t, pn, ps, region, fmt=K.F32FMT, size=size)
    yd, td = dev(y), dev(t)
    sse_r, n_bad_r = ops.recon_regions(yd, td, layout, region, mode=ops.RECON_RAW)
    assert tuple(sse_r.shape) == (2, 1, 1) and torch.equal(sse_r.cpu(), torch.from_numpy(want["sse_r"]))
    rng = np.random.RandomState(6)
    yr, tr = dev(rng.uniform(-0.2, 1.2, size=y.shape).astype(F32)), dev(rng.rand(*y.shape).astype(F32))
    for mode in (ops.RECON_8BIT, ops.RECON_RAW):
        sse_r, _ = ops.recon_regions(yr, tr, layout, region, mode=mode)
        _, _, sse, _ = ops.recon_finish(yr, tr, layout=layout, mode=mode)
        assert torch.equal(sse_r.reshape(-1), sse)
        _, _, flat, _ = ops.recon_finish(yr, tr, layout=None, mode=mode)
        assert torch.equal(sse_r.reshape(-1), flat)


# ---- the rounding modes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "special"])
@pytest.mark.parametrize("fmt", [K.U8, K.u16(9), K.u16(16), K.S16], ids=str)
@pytest.mark.parametrize("name", NAMES)
def test_modes_0_2_3_within_the_reordering_bound(name, fmt, kind):
    pn, ps, Cc, sizes, regions, layout = geo(name)
    shape = (R.N_DATA * int(np.prod(pn)), int(np.prod(ps)), Cc)
    y, t = fill(shape, kind, 1, fmt), np.random.RandomState(2).rand(*shape).astype(F32)
    yd, td = dev(y), dev(t)
    worst = 0.0
    for size in sizes:
        for region in regions:
            want = R.finish_regions(y, t, pn, ps, region, fmt=fmt, size=size)
            sse_r, n_bad_r = ops.recon_regions(yd, td, layout, region, size=size, sample_format=fmt_of(fmt))
            worst = max(worst, check_against_evaluator(sse_r, n_bad_r, want, (size, region)))
    print(f"{name} {fmt} {kind}: worst sse error / bound = {worst:.3g}")


def test_n_bad_without_a_target():
    pn, ps, Cc, sizes, regions, layout = geo("2d")
    y = fill((R.N_DATA * 6, 20, Cc), "special", 4, K.U8)
    want = R.finish_regions(y, None, pn, ps, (3, 4), size=(7, 13))
    sse_r, n_bad_r = ops.recon_regions(dev(y), None, layout, (3, 4), size=(7, 13))
    assert sse_r is None and want["n_bad_r"].sum() > 0 and np.array_equal(n_bad_r.cpu().numpy(), want["n_bad_r"])


# ---- the defining identity, device against device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [K.U8, K.F32FMT, K.u16(9)], ids=str)
@pytest.mark.parametrize("name", ["2d", "3d", "two_chunks"])
def test_a_region_is_recon_finish_on_its_box_gathered_contiguous(name, fmt):
    """sse_r[d][r] == ops.recon_finish(layout=None)'s sse, bit for bit, on the box cut out of the whole signal by torch indexing and
    made contiguous (boxes of one shape go as the datapoints of one call: a datapoint's sse does not depend on its batch)"""
    pn, ps, Cc, sizes, regions, layout = geo(name)
    shape = (R.N_DATA * int(np.prod(pn)), int(np.prod(ps)), Cc)
    y, t = fill(shape, "random", 7, fmt), np.random.RandomState(8).rand(*shape).astype(F32)
    yd, td = dev(y), dev(t)
    wy, wt = dev(E.stitch(y, pn, ps)), dev(E.stitch(t, pn, ps))                  # whole signals [n, *G, C] on the device
    for size in sizes:
        extent = size if size is not None else X.grid_of(pn, ps)
        for region in regions:
            sse_r, _ = ops.recon_regions(yd, td, layout, region, size=size, sample_format=fmt_of(fmt))
            by_shape = {}
            for idx, sl in R.boxes(extent, region):
                by_shape.setdefault(tuple(s.stop - s.start for s in sl), []).append((idx, sl))
            for box, members in by_shape.items():
                gy = torch.stack([wy[(d,) + sl] for idx, sl in members for d in range(R.N_DATA)]).reshape(-1, int(np.prod(box)), Cc)
                gt = torch.stack([wt[(d,) + sl] for idx, sl in members for d in range(R.N_DATA)]).reshape(-1, int(np.prod(box)), Cc)
                _, _, sse, _ = ops.recon_finish(gy.contiguous(), gt.contiguous(), layout=None, sample_format=fmt_of(fmt))
                got = torch.stack([sse_r[(d,) + idx] for idx, sl in members for d in range(R.N_DATA)])
                assert torch.equal(got, sse), (size, region, box)


# ---- batch, run and memory path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bits_do_not_depend_on_the_batch_its_order_or_the_run(name):
    pn, ps, Cc, sizes, regions, layout = geo(name)
    per = int(np.prod(pn))
    shape = (R.N_DATA * per, int(np.prod(ps)), Cc)
    rng = np.random.RandomState(9)
    yd, td = dev(rng.uniform(-0.2, 1.2, size=shape).astype(F32)), dev(rng.rand(*shape).astype(F32))
    order = [2, 0, 1]
    rows = torch.cat([torch.arange(d * per, (d + 1) * per) for d in order]).to(DEV)
    ys, ts = yd[rows].contiguous(), td[rows].contiguous()
    for size in sizes:
        for region in regions:
            sse_r, n_bad_r = ops.recon_regions(yd, td, layout, region, size=size)
            again, _ = ops.recon_regions(yd, td, layout, region, size=size)
            assert torch.equal(sse_r, again)
            shuffled, _ = ops.recon_regions(ys, ts, layout, region, size=size)
            assert torch.equal(shuffled, sse_r[order])
            for d in range(R.N_DATA):
                alone, _ = ops.recon_regions(yd[d * per:(d + 1) * per], td[d * per:(d + 1) * per], layout, region, size=size)
                assert torch.equal(alone, sse_r[d:d + 1])


def _offset_by_one_float(a):
    buf = torch.empty(a.numel() + 8, device=DEV, dtype=torch.float32)
    view = buf[1:1 + a.numel()].view(a.shape)
    view.copy_(a)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("fmt", [K.U8, K.F32FMT, K.S16], ids=str)
def test_the_element_path_gives_the_bits_of_the_16_byte_path(fmt):
    """the 2-D vector case (runs, box rows and origins all on 4-element boundaries) from 16-byte aligned tensors, and the same
    tensors at a storage offset of one float, which only the element-wise path can read"""
    pn, ps, Cc, sizes, regions, layout = geo("2d_vec")
    shape = (R.N_DATA * int(np.prod(pn)), int(np.prod(ps)), Cc)
    y, t = fill(shape, "special", 10, fmt), np.random.RandomState(11).rand(*shape).astype(F32)
    yd, td = dev(y), dev(t)
    assert yd.data_ptr() % 16 == 0 and td.data_ptr() % 16 == 0
    yo, to = _offset_by_one_float(yd), _offset_by_one_float(td)
    for size in sizes:
        for region in regions:
            a_sse, a_bad = ops.recon_regions(yd, td, layout, region, size=size, sample_format=fmt_of(fmt))
            for yy, tt in ((yo, to), (yo, td), (yd, to)):
                o_sse, o_bad = ops.recon_regions(yy, tt, layout, region, size=size, sample_format=fmt_of(fmt))
                assert torch.equal(a_bad, o_bad) and torch.equal(a_sse.view(torch.int64), o_sse.view(torch.int64)), (size, region)


# ---- bad elements and padding --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size,region", [("2d", (7, 13), (3, 4)), ("3d", None, (1, 4, 8)), ("2d_vec", (5, 7), (2, 2)), ("1d", (33,), (10,))])
def test_a_bad_element_stays_in_its_region_and_padding_in_none(name, size, region):
    pn, ps, Cc, _, _, layout = geo(name)
    shape = (R.N_DATA * int(np.prod(pn)), int(np.prod(ps)), Cc)
    rng = np.random.RandomState(12)
    y, t = rng.uniform(-0.2, 1.2, size=shape).astype(F32), rng.rand(*shape).astype(F32)
    extent = size if size is not None else X.grid_of(pn, ps)
    clean_sse, clean_bad = ops.recon_regions(dev(y), dev(t), layout, region, size=size)
    assert int(clean_bad.abs().sum()) == 0 and bool(torch.isfinite(clean_sse).all())
    # the source index of a whole-signal position: a NaN at the first position of datapoint 1, an inf at the last of its extent
    pos = E.stitch(np.arange(y.size).reshape(shape), pn, ps)
    first, last = (1,) + (0,) * len(extent) + (0,), (1,) + tuple(s - 1 for s in extent) + (Cc - 1,)
    yb, tb = y.copy(), t.copy()
    yb.reshape(-1)[pos[first]] = np.nan
    tb.reshape(-1)[pos[last]] = np.inf
    sse_r, n_bad_r = ops.recon_regions(dev(yb), dev(tb), layout, region, size=size)
    nr = utils.region_grid(extent, region)
    r_first, r_last = (1,) + (0,) * len(nr), (1,) + tuple(n - 1 for n in nr)
    assert r_first != r_last
    want_bad = np.zeros((R.N_DATA, *nr), dtype=np.int32)
    want_bad[r_first] = want_bad[r_last] = 1
    assert np.array_equal(n_bad_r.cpu().numpy(), want_bad)
    hit = torch.from_numpy(want_bad > 0).to(DEV)
    assert bool(torch.isnan(sse_r[hit]).all()) and torch.equal(sse_r[~hit], clean_sse[~hit])
    want = R.finish_regions(yb, tb, pn, ps, region, size=size)
    assert np.array_equal(want["n_bad_r"], want_bad)
    # a NaN in every padded position of both operands: no output bit changes
    pad = E.cut(~X.inside(R.N_DATA, pn, ps, Cc, extent), pn, ps)
    if size is not None:
        assert pad.any()
    yn, tn = np.where(pad, F32(np.nan), y), np.where(pad, F32(np.nan), t)
    p_sse, p_bad = ops.recon_regions(dev(yn), dev(tn), layout, region, size=size)
    assert torch.equal(p_sse, clean_sse) and torch.equal(p_bad, clean_bad)


def test_offsets_past_2_to_31():
    """more than 2^31 elements in the batch (each datapoint 2^20, two regions): the first and the last datapoint against the evaluator"""
    pn, ps, Cc, region = (1, 1), (512, 512), 4, (256, 512)
    n = (1 << 11) + 1
    g = torch.Generator(device=DEV).manual_seed(0)
    y = torch.empty(n, 512 * 512, Cc, device=DEV)
    for part in y.split(256):
        part.uniform_(-0.2, 1.2, generator=g)
    assert y.numel() > 2 ** 31
    sse_r, n_bad_r = ops.recon_regions(y, y, ops.PeLayout(pn, ps), region)                 # target = y itself: the rounding error
    assert tuple(sse_r.shape) == (n, 2, 1) and int(n_bad_r.abs().sum()) == 0 and bool(torch.isfinite(sse_r).all())
    for d in (0, n - 1):
        yd = y[d:d + 1].cpu().numpy()
        want = R.finish_regions(yd, yd, pn, ps, region)
        check_against_evaluator(sse_r[d:d + 1], n_bad_r[d:d + 1], want, d)


def test_the_entry_can_be_graph_captured():
    """no stream synchronisation and no table upload: a captured call replays on new inputs with the bits of an eager call"""
    pn, ps, Cc, _, _, layout = geo("2d")
    shape = (R.N_DATA * 6, 20, Cc)
    rng = np.random.RandomState(13)
    yd, td = dev(rng.rand(*shape).astype(F32)), dev(rng.rand(*shape).astype(F32))
    out = (torch.zeros(R.N_DATA, 3, 4, device=DEV, dtype=torch.float64), torch.zeros(R.N_DATA, 3, 4, device=DEV, dtype=torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.recon_regions(yd, td, layout, (3, 4), size=(7, 13), out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.recon_regions(yd, td, layout, (3, 4), size=(7, 13), out=out)
    yd.copy_(dev(rng.rand(*shape).astype(F32)))
    out[0].zero_()
    graph.replay()
    eager, _ = ops.recon_regions(yd, td, layout, (3, 4), size=(7, 13))
    assert torch.equal(out[0], eager)


# ---- guard words and refusals ---------------------------------------------------------------------------------------------------------
PAD = 64
FILL = {torch.uint8: 0xA5, torch.float64: -7.5, torch.int32: -77}


def _bordered(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), FILL[dtype], device=DEV, dtype=dtype)
    return buf, buf[PAD:PAD + n].view(shape)


def _border_intact(buf, n):
    f = FILL[buf.dtype]
    return bool((buf[:PAD] == f).all()) and bool((buf[PAD + n:] == f).all())


def _raw(y, t, N, P, Cc, nd, pn, ps, size, region, mode, depth, sse_r, n_bad_r, ws, ws_bytes=None):
    lib = _lib.load()
    arr = lambda v: None if v is None else (C.c_int32 * 4)(*(list(v) + [0] * (4 - len(v))))      # noqa: E731
    p = lambda v: C.c_void_p(0 if v is None else v.data_ptr())                                 # noqa: E731
    if ws_bytes is None:
        ws_bytes = 0 if ws is None else ws.numel()
    return lib.rcb_recon_regions(p(y), p(t), N, P, Cc, nd, arr(pn), arr(ps), arr(size), arr(region), mode, depth, p(sse_r), p(n_bad_r),
                                 p(ws), ws_bytes, _lib.stream_ptr())


@pytest.mark.parametrize("name", NAMES)
def test_nothing_is_written_outside_the_outputs_and_the_workspace(name):
    pn, ps, Cc, sizes, regions, layout = geo(name)
    N, P = R.N_DATA * int(np.prod(pn)), int(np.prod(ps))
    rng = np.random.RandomState(14)
    y, t = rng.uniform(-0.2, 1.2, size=(N, P, Cc)).astype(F32), rng.rand(N, P, Cc).astype(F32)
    yd, td = dev(y), dev(t)
    lib = _lib.load()
    for size in sizes:
        extent = size if size is not None else X.grid_of(pn, ps)
        for region in regions:
            nr = utils.region_grid(extent, region)
            need = lib.rcb_recon_regions_workspace_bytes(R.N_DATA, int(np.prod(nr)), int(np.prod([min(a, b) for a, b in zip(extent, region)])) * Cc)
            assert need > 0
            bufs = [_bordered((R.N_DATA, *nr), torch.float64), _bordered((R.N_DATA, *nr), torch.int32), _bordered((need,), torch.uint8)]
            (_, sse_r), (_, n_bad_r), (_, ws) = bufs
            assert _raw(yd, td, N, P, Cc, len(pn), pn, ps, size, region, 0, 0, sse_r, n_bad_r, ws) == 0
            torch.cuda.synchronize()
            for buf, v in bufs:
                assert _border_intact(buf, v.numel()), (size, region)
            ref_sse, ref_bad = ops.recon_regions(yd, td, layout, region, size=size)
            assert torch.equal(sse_r, ref_sse) and torch.equal(n_bad_r, ref_bad)


def test_refusals():
    """every refusal of the header: the library returns RCB_ERR_* with its message before it launches anything (the outputs keep
    their fill), and ops.recon_regions raises RcbError"""
    pn, ps, Cc, N, P = (2, 3), (4, 5), 3, 12, 20
    rng = np.random.RandomState(15)
    y, t = dev(rng.rand(N, P, Cc).astype(F32)), dev(rng.rand(N, P, Cc).astype(F32))
    bufs = [_bordered((2, 3, 4), torch.float64), _bordered((2, 3, 4), torch.int32)]
    sse_r, n_bad_r = (v for _, v in bufs)
    ws = torch.empty(1 << 16, device=DEV, dtype=torch.uint8)
    lib = _lib.load()
    base = dict(y=y, t=t, N=N, P=P, Cc=Cc, nd=2, pn=pn, ps=ps, size=(7, 13), region=(3, 4), mode=0, depth=0, sse_r=sse_r,
                n_bad_r=n_bad_r, ws=ws)
    assert _raw(**base) == 0                                                         # (the valid call, for contrast)
    torch.cuda.synchronize()
    for _, v in bufs:
        v.fill_(FILL[v.dtype])
    refused = {
        "null y": (dict(y=None), "null y or workspace"),
        "null workspace": (dict(ws=None), "null y or workspace"),
        "both outputs null": (dict(sse_r=None, n_bad_r=None), "nothing to write"),
        "mode 4": (dict(mode=4), "mode 4"),
        "mode -1": (dict(mode=-1), "mode -1"),
        "u16 at depth 8": (dict(mode=2, depth=8), "depth 8 for mode 2"),
        "a depth for the 8-bit mode": (dict(depth=9), "depth 9 for mode 0"),
        "nd = 0": (dict(nd=0), "0 grid dimensions"),
        "nd = 4": (dict(nd=4, pn=(1, 1, 2, 3), ps=(1, 1, 4, 5)), "4 grid dimensions"),
        "null patch_nums": (dict(pn=None), "null patch geometry or region"),
        "null region": (dict(region=None), "null patch geometry or region"),
        "C = 0": (dict(Cc=0), "0 channels"),
        "C = 33": (dict(Cc=33), "33 channels"),
        "no rows": (dict(N=0), "0 rows"),
        "sse_r without target": (dict(t=None), "sse_r needs a target"),
        "region 0": (dict(region=(3, 0)), "axis 1 of a region has 0 positions"),
        "region < 0": (dict(region=(-3, 4)), "axis 0 of a region has -3 positions"),
        "a patch count of 0": (dict(pn=(2, 0)), "axis 1 has 0 patches"),
        "size 0": (dict(size=(0, 13)), "axis 0 of the signal has 0 positions"),
        "size beyond the grid": (dict(size=(7, 16)), "axis 1 of the signal has 16 positions"),
        "P != prod(patch_size)": (dict(ps=(4, 4), size=(7, 12)), "the patch has 16 pixels, the rows 20"),
        "N no multiple of prod(patch_nums)": (dict(N=11), "no whole number of datapoints"),
        "2^31 elements per datapoint": (dict(pn=(1 << 15, 1 << 14), N=1 << 29, size=None), "per datapoint"),
        "2^31 workgroups": (dict(pn=(1, 1), ps=(64, 64), Cc=1, N=1 << 20, P=4096, size=None, region=(1, 1)), "more than 2^31 - 1 workgroups"),
        "workspace too small": (dict(ws=ws[:64]), "workspace of 64 bytes"),
        "workspace misaligned": (dict(ws=ws[4:]), "8-byte aligned"),
    }
    for what, (change, message) in refused.items():
        kw = dict(base)
        kw.update(change)
        rc = _raw(**kw)
        assert rc < 0, what
        assert message in lib.rcb_last_error_string().decode(), (what, lib.rcb_last_error_string())
    torch.cuda.synchronize()
    for buf, _ in bufs:
        assert bool((buf == FILL[buf.dtype]).all())                                   # nothing was launched
    # the wrapper
    lay = ops.PeLayout(pn, ps)
    calls = {
        "no layout": lambda: ops.recon_regions(y, t, None, (3, 4)),
        "region of one entry": lambda: ops.recon_regions(y, t, lay, (3,)),
        "region 0": lambda: ops.recon_regions(y, t, lay, (3, 0)),
        "size of one entry": lambda: ops.recon_regions(y, t, lay, (3, 4), size=(7,)),
        "size beyond the grid": lambda: ops.recon_regions(y, t, lay, (3, 4), size=(9, 13)),
        "P != prod(patch_size)": lambda: ops.recon_regions(y, t, ops.PeLayout(pn, (4, 4)), (3, 4)),
        "N no multiple": lambda: ops.recon_regions(y[:11], t[:11], lay, (3, 4)),
        "cpu tensor": lambda: ops.recon_regions(y.cpu(), None, lay, (3, 4)),
        "fp64": lambda: ops.recon_regions(y.double(), None, lay, (3, 4)),
        "strided": lambda: ops.recon_regions(y.transpose(0, 1), None, lay, (3, 4)),
        "target shape": lambda: ops.recon_regions(y, t[:6], lay, (3, 4)),
        "target on the host": lambda: ops.recon_regions(y, t.cpu(), lay, (3, 4)),
        "output shape": lambda: ops.recon_regions(y, t, lay, (3, 4), out=(torch.empty(2, 4, 3, device=DEV, dtype=torch.float64), None)),
        "output dtype": lambda: ops.recon_regions(y, t, lay, (3, 4), out=(None, torch.empty(2, 3, 4, device=DEV, dtype=torch.int64))),
        "empty": lambda: ops.recon_regions(y[:0], None, lay, (3, 4)),
        "mode 2 without a depth": lambda: ops.recon_regions(y, t, lay, (3, 4), mode=ops.RECON_U16),
    }
    for what, call in calls.items():
        with pytest.raises(ops.RcbError):
            call()
            pytest.fail(what)


# ---- utils.metric_regions_device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset,name,size,by", [("kodak", "2d", None, "patch"), ("kodak", "2d", (7, 13), (3, 4)),
                                                  ("video", "3d", None, "frame"), ("video", "3d", (2, 3, 7), "frame"),
                                                  ("audio", "1d", (33,), (10,)), ("protein", "1d", None, "patch")])
def test_metric_regions_device_is_the_figure_of_each_box(dataset, name, size, by):
    from test_recon_emul_cpu import psnr_bound_db, rmsd_bound_abs
    pn, ps, Cc, _, _, layout = geo(name)
    shape = (R.N_DATA * int(np.prod(pn)), int(np.prod(ps)), Cc)
    rng = np.random.RandomState(16)
    t = rng.rand(*shape).astype(F32)
    y = (t + 0.05 * rng.randn(*shape)).astype(F32)
    region = utils.region_of(layout, by)
    got = utils.metric_regions_device(dev(t), dev(y), dataset, layout, region, size=size)
    wy, wt = R.whole_cropped(y, pn, ps, size), R.whole_cropped(t, pn, ps, size)
    extent = wy.shape[1:-1]
    assert got.shape == (R.N_DATA, *utils.region_grid(extent, region)) and got.dtype == np.float64
    counts = utils.region_counts(extent, region, Cc)
    for idx, sl in R.boxes(extent, region):
        for d in range(R.N_DATA):
            o, c = wt[(d,) + sl], wy[(d,) + sl]
            if dataset == "protein":
                want = float(utils.batch_RMSD(o[None], c[None], 25)[0])
                assert abs(got[(d,) + idx] - want) <= rmsd_bound_abs(int(counts[idx]), 1.3, got[(d,) + idx])
            else:
                want = utils.PSNR(o, c, round=utils.METRIC_ROUNDS[dataset])
                assert want < 60.0 and abs(got[(d,) + idx] - want) <= psnr_bound_db(int(counts[idx]))
