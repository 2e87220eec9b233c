"""rcb_recon_finish (N4: 8-bit whole signals and exact per-datapoint squared errors on the device) against the numpy evaluator
tests/recon_emul.py, whose premises tests/test_recon_emul_cpu.py checks: u8 / whole bit for bit, sse bit for bit on dyadic inputs
and within the a-priori reordering bound elsewhere, bit identity alone / in a batch / run to run, NaN locality, refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import recon_emul as E
from test_recon_emul_cpu import psnr_bound_db, rmsd_bound_abs

pytestmark = pytest.mark.gpu

from recombiner_amd import _lib, ops, utils  # noqa: E402

DEV = "cuda"
F32 = np.float32

# name -> (patch_nums, patch_size, C, rows N).  The smallest shapes that reach every index path: rows = datapoints with an odd
# run (scalar path: 99 and 33 elements, a tail quad), 1-D / 2-D / 3-D patches with runs of 7 / 15 floats (scalar) and 12 / 60
# floats (16-byte path; C = 20: five quads per pixel, runs that end inside a 64-byte line), two chunks (one workgroup per 8192
# elements of a datapoint) on either path, and more chunks than the reducing workgroup has threads.
CASES = {
    "a3": (None, None, 3, 3, 33),
    "a1": (None, None, 1, 3, 33),
    "b": ((5,), (7,), 1, 10, None),
    "c": ((2, 3), (4, 5), 3, 12, None),
    "d": ((1, 2, 2), (3, 2, 4), 3, 8, None),
    "e": ((2, 2), (3, 3), 20, 8, None),
    "two_chunks_vec": ((3, 2), (24, 24), 3, 12, None),
    "two_chunks_scalar": (None, None, 3, 2, 3001),
    "many_chunks": (None, None, 4, 2, 526337),
}
SMALL = ["a3", "a1", "b", "c", "d", "e"]


def geo(name):
    pn, ps, Cc, N, P = CASES[name]
    if pn is not None:
        P = int(np.prod(ps))
    return pn, ps, Cc, N, P, (ops.PeLayout(pn, ps) if pn is not None else None)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(y, t, layout, mode, u8=False, whole=False, out=None):
    return ops.recon_finish(dev(y), None if t is None else dev(t), layout=layout, mode=mode, want_u8=u8, want_whole=whole, out=out)


def special_values():
    """the tie set, values one ulp below / above every tie, -0.0, 0, 1, +-inf (no NaN)"""
    x, _ = E.tie_inputs()
    return np.concatenate([x, np.nextafter(x, F32(0)), np.nextafter(x, F32(1)),
                           np.array([-0.0, 0.0, 1.0, np.inf, -np.inf, np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2))], dtype=F32)])


def fill(shape, kind, seed):
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    if kind == "random":
        return rng.uniform(-0.2, 1.2, size=shape).astype(F32)
    sp = special_values()
    a = rng.uniform(-0.2, 1.2, size=n).astype(F32)
    m = min(n, len(sp))
    a[rng.permutation(n)[:m]] = sp[rng.permutation(len(sp))[:m]]         # (a small case takes a random part of the set)
    return a.reshape(shape)


def sse_bound(terms):
    """a-priori bound on the difference between two summation orders of n exact fp64 terms, one of them correctly rounded (the
    evaluator's fsum): n * 2^-53 * sum(terms), per datapoint"""
    return terms.shape[1] * 2.0 ** -53 * terms.sum(1)


@pytest.mark.parametrize("kind", ["random", "special"])
@pytest.mark.parametrize("name", SMALL + ["two_chunks_vec", "two_chunks_scalar"])
def test_mode0_u8_whole_and_sse_match_the_evaluator(name, kind):
    pn, ps, Cc, N, P, layout = geo(name)
    if kind == "special" and name == "a3":
        # every special value at least once, whatever part of the set the other cases draw: as many datapoints as it takes
        sp = special_values()
        y = np.resize(sp, (-(-len(sp) // (P * Cc)), P, Cc)).astype(F32)
        N = y.shape[0]
    else:
        y = fill((N, P, Cc), kind, 1)
    t = np.random.RandomState(2).rand(N, P, Cc).astype(F32)
    want = E.finish(y, t, pn, ps, mode=0)
    u8, whole, sse, n_bad = run(y, t, layout, 0, u8=True, whole=True)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == want["u8"].shape == ops.recon_whole_shape((N, P, Cc), layout)
    assert torch.equal(u8.cpu(), torch.from_numpy(want["u8"]))
    assert torch.equal(whole.cpu(), torch.from_numpy(np.ascontiguousarray(want["whole"])))
    assert np.array_equal(n_bad.cpu().numpy(), want["n_bad"])
    got = sse.cpu().numpy()
    fin = want["n_bad"] == 0
    assert np.isnan(got[~fin]).all() and np.isnan(want["sse"][~fin]).all()
    err, bound = np.abs(got - want["sse"])[fin], sse_bound(want["terms"])[fin]
    if fin.any():
        print(f"{name} {kind}: worst sse error / bound = {(err / bound).max():.3g}")
        assert (err <= bound).all()


@pytest.mark.parametrize("name", SMALL + ["two_chunks_vec", "two_chunks_scalar", "many_chunks"])
def test_mode1_sse_is_exact_on_dyadic_inputs_and_whole_is_a_copy(name):
    pn, ps, Cc, N, P, layout = geo(name)
    y, t = E.dyadic((N, P, Cc), 3), E.dyadic((N, P, Cc), 4)
    want = E.finish(y, t, pn, ps, mode=1)
    u8, whole, sse, n_bad = run(y, t, layout, 1, whole=True)
    assert u8 is None and torch.equal(whole.cpu(), torch.from_numpy(np.ascontiguousarray(want["whole"])))
    assert torch.equal(sse.cpu(), torch.from_numpy(want["sse"])) and int(n_bad.abs().sum()) == 0


@pytest.mark.parametrize("name", SMALL + ["many_chunks"])
def test_mode1_sse_on_random_inputs_within_the_reordering_bound(name):
    pn, ps, Cc, N, P, layout = geo(name)
    rng = np.random.RandomState(5)
    y, t = rng.randn(N, P, Cc).astype(F32), rng.randn(N, P, Cc).astype(F32)
    want = E.finish(y, t, pn, ps, mode=1)
    _, _, sse, _ = run(y, t, layout, 1)
    err, bound = np.abs(sse.cpu().numpy() - want["sse"]), sse_bound(want["terms"])
    print(f"{name} mode 1: worst sse error / bound = {(err / bound).max():.3g}")
    assert (err <= bound).all()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", SMALL + ["two_chunks_vec", "two_chunks_scalar", "many_chunks"])
def test_sse_bits_do_not_depend_on_the_batch_or_the_run(name, mode):
    """each datapoint alone (its rows as a batch of one -- for an odd datapoint size also from a pointer that is not 16-byte
    aligned) against itself inside the batch, and a second run of the same call"""
    pn, ps, Cc, N, P, layout = geo(name)
    rng = np.random.RandomState(6)
    y, t = rng.uniform(-0.2, 1.2, size=(N, P, Cc)).astype(F32), rng.rand(N, P, Cc).astype(F32)
    yd, td = dev(y), dev(t)
    _, _, sse, _ = ops.recon_finish(yd, td, layout=layout, mode=mode)
    _, _, again, _ = ops.recon_finish(yd, td, layout=layout, mode=mode)
    assert torch.equal(sse, again)
    per = N // sse.numel()
    for d in range(sse.numel()):
        _, _, alone, _ = ops.recon_finish(yd[d * per:(d + 1) * per], td[d * per:(d + 1) * per], layout=layout, mode=mode)
        assert torch.equal(alone, sse[d:d + 1])


@pytest.mark.parametrize("name", ["c", "d", "a3"])
def test_a_bad_element_stays_in_its_datapoint(name):
    pn, ps, Cc, N, P, layout = geo(name)
    rng = np.random.RandomState(7)
    y, t = rng.uniform(-0.2, 1.2, size=(N, P, Cc)).astype(F32), rng.rand(N, P, Cc).astype(F32)
    clean = run(y, t, layout, 0, u8=True, whole=True)
    yb, tb = y.copy(), t.copy()
    yb[0, 3, 0] = np.nan
    tb[0, 5, Cc - 1] = np.inf
    u8, whole, sse, n_bad = run(yb, tb, layout, 0, u8=True, whole=True)
    assert n_bad.cpu().tolist() == [2] + [0] * (sse.numel() - 1)
    assert bool(torch.isnan(sse[0])) and torch.equal(sse[1:], clean[2][1:])
    assert torch.equal(u8[1:], clean[0][1:]) and torch.equal(whole[1:], clean[1][1:])
    # inside datapoint 0 only the NaN element changed: it is 0 in u8 (and in whole)
    pos = E.stitch(np.arange(N * P * Cc).reshape(N, P, Cc), pn, ps)
    at = tuple(int(v[0]) for v in np.nonzero(pos == (0 * P + 3) * Cc + 0))
    assert int(u8[at]) == 0 and float(whole[at]) == 0.0
    same = torch.ones_like(u8, dtype=torch.bool)
    same[at] = False
    assert torch.equal(u8[same], clean[0][same]) and torch.equal(whole[same], clean[1][same])
    want = E.finish(yb, tb, pn, ps, mode=0)
    assert torch.equal(u8.cpu(), torch.from_numpy(want["u8"])) and np.array_equal(n_bad.cpu().numpy(), want["n_bad"])


def test_offsets_past_2_to_31():
    """more than 2^31 elements in the batch (each datapoint 2^20): the first and the last datapoint against the evaluator"""
    Ed, n = 1 << 20, (1 << 11) + 1
    g = torch.Generator(device=DEV).manual_seed(0)
    y = torch.empty(n, Ed // 4, 4, device=DEV)
    for part in y.split(256):
        part.uniform_(-0.2, 1.2, generator=g)
    assert y.numel() > 2 ** 31
    u8, _, sse, n_bad = ops.recon_finish(y, y, mode=0, want_u8=True)           # target = y itself: sse = the rounding error
    for d in (0, n - 1):
        yd = y[d:d + 1].cpu().numpy()
        want = E.finish(yd, yd, mode=0)
        assert torch.equal(u8[d:d + 1].cpu(), torch.from_numpy(want["u8"]))
        err, bound = abs(float(sse[d]) - want["sse"][0]), sse_bound(want["terms"])[0]
        assert err <= bound
    assert int(n_bad.abs().sum()) == 0 and bool(torch.isfinite(sse).all())


# ---- refusals, with a canary border around every output -------------------------------------------------------------------------
PAD = 64


def _bordered(shape, dtype, fill, shift=0):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), fill, device=DEV, dtype=dtype)
    return buf, buf[PAD + shift:PAD + shift + n].view(shape)


def _border_intact(buf, n, fill, shift=0):
    return bool((buf[:PAD + shift] == fill).all()) and bool((buf[PAD + shift + n:] == fill).all())


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name", SMALL + ["two_chunks_vec", "two_chunks_scalar"])
def test_nothing_is_written_outside_the_outputs(name, shift):
    """a canary border around u8 / whole / sse / n_bad stays intact; shift = 1 moves every output off its 16-byte alignment (the
    element-wise path of the same launch), with the same results"""
    pn, ps, Cc, N, P, layout = geo(name)
    y, t = fill((N, P, Cc), "random", 8), np.random.RandomState(9).rand(N, P, Cc).astype(F32)
    shape = ops.recon_whole_shape((N, P, Cc), layout)
    n_data = shape[0]
    bufs = [_bordered(shape, torch.uint8, 0xA5, shift), _bordered(shape, torch.float32, -7.5, shift),
            _bordered((n_data,), torch.float64, -7.5, shift), _bordered((n_data,), torch.int32, -77, shift)]
    u8, whole, sse, n_bad = run(y, t, layout, 0, u8=True, whole=True, out=tuple(v for _, v in bufs))
    torch.cuda.synchronize()
    for (buf, v), f in zip(bufs, (0xA5, -7.5, -7.5, -77)):
        assert _border_intact(buf, v.numel(), f, shift)
    want = E.finish(y, t, pn, ps, mode=0)
    assert torch.equal(u8.cpu(), torch.from_numpy(want["u8"])) and torch.equal(whole.cpu(), torch.from_numpy(np.ascontiguousarray(want["whole"])))
    ref = run(y, t, layout, 0)[2]
    assert torch.equal(sse, ref)                                   # the same bits on either path


def _raw(y, t, N, P, Cc, nd, pn, ps, mode, u8, whole, sse, n_bad, ws):
    lib = _lib.load()
    arr = lambda v: (C.c_int32 * 4)(*(list(v) + [0] * (4 - len(v))))      # noqa: E731
    p = lambda v: C.c_void_p(0 if v is None else v.data_ptr())          # noqa: E731
    return lib.rcb_recon_finish(p(y), p(t), N, P, Cc, nd, arr(pn), arr(ps), mode, p(u8), p(whole), p(sse), p(n_bad), p(ws),
                                0 if ws is None else ws.numel(), _lib.stream_ptr())


def test_refusals():
    """every refusal of the header: the library returns RCB_ERR_* with a message before it launches anything (the outputs and
    their canary borders keep their fill), and ops.recon_finish raises RcbError"""
    pn, ps, Cc, N, P = (2, 3), (4, 5), 3, 12, 20
    y, t = dev(fill((N, P, Cc), "random", 1)), dev(fill((N, P, Cc), "random", 2))
    shape = (2, 8, 15, 3)
    bufs = [_bordered(shape, torch.uint8, 0xA5), _bordered(shape, torch.float32, -7.5), _bordered((2,), torch.float64, -7.5),
            _bordered((2,), torch.int32, -77)]
    u8, whole, sse, n_bad = (v for _, v in bufs)
    ws = torch.empty(1 << 16, device=DEV, dtype=torch.uint8)
    lib = _lib.load()
    assert _raw(y, t, N, P, Cc, 2, pn, ps, 0, u8, whole, sse, n_bad, ws) == 0          # (the valid call, for contrast)
    for _, v in bufs:
        v.fill_({torch.uint8: 0xA5, torch.float32: -7.5, torch.float64: -7.5, torch.int32: -77}[v.dtype])
    refused = {
        "nd > 3": dict(nd=4, pn=(1, 1, 2, 3), ps=(1, 1, 4, 5)),
        "C = 0": dict(Cc=0),
        "C = 33": dict(Cc=33),
        "P != prod(patch_size)": dict(ps=(4, 4)),
        "N no multiple of prod(patch_nums)": dict(N=11),
        "u8 with mode 1": dict(mode=1),
        "sse without target": dict(t=None),
        "2^31 elements per datapoint": dict(nd=0, N=1, P=1 << 30, Cc=2),
        "2^31 elements per stitched datapoint": dict(pn=(1 << 15, 1 << 14), ps=(4, 5), N=1 << 29),
        "workspace too small": dict(ws=ws[:8]),
        "null y": dict(y=None),
    }
    for what, change in refused.items():
        kw = dict(y=y, t=t, N=N, P=P, Cc=Cc, nd=2, pn=pn, ps=ps, mode=0, u8=u8, whole=whole, sse=sse, n_bad=n_bad, ws=ws)
        kw.update(change)
        rc = _raw(**kw)
        assert rc < 0, what
        assert len(lib.rcb_last_error_string()) > 10, what
    assert lib.rcb_recon_workspace_bytes(1, 1 << 31) == -1 and lib.rcb_recon_workspace_bytes(0, 5) == -1
    torch.cuda.synchronize()
    for (buf, v), f in zip(bufs, (0xA5, -7.5, -7.5, -77)):
        assert bool((buf == f).all())                                  # nothing was launched
    # the wrapper
    lay = ops.PeLayout(pn, ps)
    bad4 = ops.PeLayout((2, 3), (4, 5))
    bad4.patch_nums, bad4.patch_size = [1, 1, 2, 3], [1, 1, 4, 5]
    calls = {
        "nd > 3": lambda: ops.recon_finish(y, t, layout=bad4),
        "C = 33": lambda: ops.recon_finish(torch.zeros(2, 4, 33, device=DEV), None),
        "P != prod(patch_size)": lambda: ops.recon_finish(y, t, layout=ops.PeLayout(pn, (4, 4))),
        "N no multiple": lambda: ops.recon_finish(y[:11], t[:11], layout=lay),
        "u8 with mode 1": lambda: ops.recon_finish(y, t, layout=lay, mode=1, want_u8=True),
        "cpu tensor": lambda: ops.recon_finish(y.cpu(), None),
        "fp64": lambda: ops.recon_finish(y.double(), None),
        "strided": lambda: ops.recon_finish(y.transpose(0, 1), None),
        "2-D": lambda: ops.recon_finish(y[0], None),
        "target shape": lambda: ops.recon_finish(y, t[:6], layout=lay),
        "target dtype": lambda: ops.recon_finish(y, t.double(), layout=lay),
        "target on the host": lambda: ops.recon_finish(y, t.cpu(), layout=lay),
        "output shape": lambda: ops.recon_finish(y, t, layout=lay, out=(None, None, torch.empty(3, device=DEV, dtype=torch.float64), None)),
        "empty": lambda: ops.recon_finish(y[:0], None),
    }
    for what, call in calls.items():
        with pytest.raises(ops.RcbError):
            call()
            pytest.fail(what)


# ---- utils.metric_device -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset,name", [("cifar", "a3"), ("kodak", "c"), ("kodak", "e"), ("video", "d"), ("audio", "b"), ("protein", "a3")])
def test_metric_device_agrees_with_utils_metric(dataset, name):
    pn, ps, Cc, N, P, layout = geo(name)
    rng = np.random.RandomState(11)
    y = rng.rand(N, P, Cc).astype(F32)
    pred = (y + 0.05 * rng.randn(N, P, Cc)).astype(F32)
    got = utils.metric_device(dev(y), dev(pred), dataset, layout)
    want = utils.metric(y, pred, dataset)
    assert np.shape(got) == np.shape(want) and isinstance(got, float) == isinstance(want, float)
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    if dataset == "protein":
        bound = np.array([rmsd_bound_abs(P * Cc, 1.3, g) for g in got])
    else:
        bound = psnr_bound_db(P * Cc if dataset == "cifar" else y.size)
        assert np.all(np.asarray(got) < 60.0)
    print(f"{dataset} / {name}: {got}, worst |diff| / bound = {np.max(err / bound):.3g}")
    assert np.all(err <= bound)
    # the batch-wide figures do not depend on how the rows are grouped into datapoints
    if dataset in ("kodak", "video", "audio"):
        flat = utils.metric_device(dev(y), dev(pred), dataset, None)
        assert abs(flat - got) <= 1e-12 * abs(got)
