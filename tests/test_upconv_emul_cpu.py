"""CPU tests of the fp64 evaluator of the upsampling net's conv kernels (tests/upconv_emul.py): without any rounding it is the
reference's stage (F.interpolate + F.conv{1,2,3}d and autograd), its effective weights reproduce the stage in phase form, the
lattice condition holds for every case that test_hip_upconv_exact.py runs on the GPU, summation order does not matter there, and
every deliberately wrong evaluator of upconv_emul.DISCRIMINATION changes its case's output.  Nothing here needs the kernels or
their library."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import upconv_emul as ue

F64 = torch.float64
GEOS = [ue.Geo(f, k, pad, nd) for (f, k, pad) in ((2, 3, 1), (4, 5, 2)) for nd in (1, 2, 3)]
GRIDS = {1: (7,), 2: (3, 5), 3: (2, 3, 4)}                                # odd sizes, no multiple of anything
LATTICE_CASES = (ue.PHASECONV_CASES + ue.STAGE1_CASES + ue.UPCONV2_CASES + ue.UPCONV2_SLOPE_CASES + ue.UPCONV3_CASES
                 + [ue.HALF_WG_CASE])
FWD_ONLY = ue.UPCONV2_FWD_ONLY


def _ids(cases):
    return [c.id for c in cases]


def _stage_ref(x, W, b, geo):
    conv = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}[geo.nd]
    return conv(F.interpolate(x.movedim(-1, 1), scale_factor=geo.f, mode="nearest"), W, b, padding=geo.pad).movedim(1, -1)


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: "f%d-k%d-%dd" % (g.f, g.k, g.nd))
def test_unrounded_evaluator_is_the_reference_stage(geo):
    """forward, and the autograd gradients of input, weight and bias, to 1e-12; the data gradient with its LeakyReLU' factor; the
    effective weights in phase form, as the 2^d-tap weights and as Wbig over 3-pixel windows"""
    torch.manual_seed(geo.f * 10 + geo.nd)
    B, g, Ci, Co = 2, GRIDS[geo.nd], 5, 3
    pre = torch.randn(B, *g, Ci, dtype=F64, requires_grad=True)           # stored stage input = LeakyReLU(pre): same sign
    W = torch.randn(Co, Ci, *([geo.k] * geo.nd), dtype=F64, requires_grad=True)
    b = torch.randn(Co, dtype=F64, requires_grad=True)
    x = F.leaky_relu(pre, 0.01)
    lin = _stage_ref(x, W, b, geo)
    dy = torch.randn_like(lin)
    gpre, gx, gW, gb = torch.autograd.grad(lin, [pre, x, W, b], dy)
    xd, Wd, bd = x.detach(), W.detach(), b.detach()
    Wt = ue.tap_weights(Wd, geo)
    y = ue.forward_acc(xd, Wt, bd, geo)
    assert _rel(y, lin.detach()) < 1e-12
    assert _rel(ue.lrelu(y, False), F.leaky_relu(lin.detach(), 0.01)) < 1e-12
    dx = ue.dgrad_acc(dy, Wt, geo)
    assert _rel(dx, gx) < 1e-12 and _rel(ue.dlrelu(dx, xd, False), gpre) < 1e-12
    dWp, db = ue.wgrad_acc(xd, dy, geo)
    assert _rel(ue.conv_layout(dWp), gW) < 1e-12 and _rel(db, gb) < 1e-12
    # pre-summed taps (exact sums) in the tap loop are the same stage, forward and backward
    Ws = ue.tap_weights(Wd, geo, "f64")
    assert _rel(ue.forward_acc(xd, Ws, bd, geo), lin.detach()) < 1e-12 and _rel(ue.dgrad_acc(dy, Ws, geo), gx) < 1e-12
    # the 2^d-tap weights, used in phase form, are the stage; their gradient layout is the adjoint of their build
    Weff = ue.eff_layout(Ws, geo)
    assert _rel(ue.phase_forward(xd, Weff, bd, geo), lin.detach()) < 1e-12
    dWeff = ue.eff_layout(dWp, geo)
    Weff_r = Weff.clone().requires_grad_(True)
    (gWeff,) = torch.autograd.grad(ue.phase_forward(xd, Weff_r, bd, geo), [Weff_r], dy)
    assert _rel(dWeff, gWeff) < 1e-12
    assert _rel(ue.eff_grad_to_conv(dWeff, geo), gW) < 1e-12              # every tap collects the gradient of its group
    # Wbig: one GEMM over the 3^d-pixel windows, all phases at once, then the pixel shuffle
    big = ue.big_layout(Ws, geo)
    xp = F.pad(xd, [0, 0] + [1, 1] * geo.nd)
    cols = torch.cat([xp[(slice(None),) + tuple(slice(o[d], o[d] + g[d]) for d in range(geo.nd))]
                      for o in itertools.product(range(3), repeat=geo.nd)], dim=-1)
    yb = (cols.reshape(-1, cols.shape[-1]) @ big).view([B] + list(g) + [geo.f] * geo.nd + [Co]) + bd
    perm = [0] + [v for d in range(geo.nd) for v in (1 + d, 1 + geo.nd + d)] + [1 + 2 * geo.nd]
    assert _rel(yb.permute(perm).reshape(lin.shape), lin.detach()) < 1e-12
    dbig = ue.big_layout(dWp, geo)
    big_r = big.clone().requires_grad_(True)
    yb2 = (cols.reshape(-1, cols.shape[-1]) @ big_r).view([B] + list(g) + [geo.f] * geo.nd + [Co]).permute(perm).reshape(lin.shape)
    (gbig,) = torch.autograd.grad(yb2, [big_r], dy)
    assert _rel(dbig, gbig * (big != 0)) < 1e-12 and bool((dbig[big == 0] == 0).all())      # zero where no phase reads


def test_dense_map_is_stage_one_on_the_2x2_latent_grid():
    geo = ue.Geo(4, 5, 2, 2)
    torch.manual_seed(3)
    W = torch.randn(4, 6, 5, 5, dtype=F64, requires_grad=True)
    x = torch.randn(3, 2, 2, 6, dtype=F64)
    M = ue.dense_map(W.detach(), (2, 2), geo)
    lin = _stage_ref(x, W, None, geo)
    assert _rel((x.reshape(3, -1) @ M).view(lin.shape), lin.detach()) < 1e-12
    dy = torch.randn_like(lin)
    (gW,) = torch.autograd.grad(lin, [W], dy)
    dM = x.reshape(3, -1).t() @ dy.reshape(3, -1)
    assert _rel(ue.dense_map_grad(dM, tuple(W.shape), (2, 2), geo), gW) < 1e-12


def test_bf16_rounding_is_torchs():
    torch.manual_seed(0)
    v = torch.cat([torch.randn(4096) * 10.0 ** torch.randint(-6, 6, (4096,)), torch.tensor([0.0, 1.0, 257.0, 255.5, 1e-40, -3.0])])
    assert torch.equal(ue.bf16(v.double()), v.to(torch.bfloat16).double())
    assert ue.SLOPE32 == float(torch.tensor(0.01, dtype=torch.float32)) and ue.SLOPE32 != 0.01


# ---- the lattice condition: the generator's own assertion, for every case of the GPU tests --------------------------------------
_LATTICE = {}


def _lattice(case, want=("fwd", "dgrad", "wgrad")):
    key = (case, want)
    if key not in _LATTICE:
        _LATTICE.clear()                                    # (one at a time: the largest hold a few hundred MB)
        _LATTICE[key] = ue.lattice(case, want=want)
    return _LATTICE[key]


@pytest.mark.parametrize("case", LATTICE_CASES, ids=_ids(LATTICE_CASES))
def test_lattice_condition_holds_and_order_does_not_matter(case):
    """sum |product| / lsb < 2^24 for every element of every output (asserted inside upconv_emul.lattice), and on a seeded sample
    of output elements (all of them where there are few) the fp32 sum of the products taken in ascending order and in a seeded
    permutation has the bits of the fp64 result"""
    want = ("fwd",) if case is ue.HALF_WG_CASE else ("fwd", "dgrad", "wgrad")
    inp, ref = _lattice(case, want)
    assert all(q < ue.EXACT for q in ref.q.values())
    print(case.id, " ".join("%s %.0f" % kv for kv in ref.q.items()))
    _orders(case, inp, want)


@pytest.mark.parametrize("case", FWD_ONLY, ids=_ids(FWD_ONLY))
def test_lattice_condition_of_the_second_trip_forward(case):
    inp, ref = _lattice(case, ("fwd",))
    assert ref.q["y"] < ue.EXACT
    _orders(case, inp, ("fwd",))


@pytest.mark.parametrize("cc", ue.CIFAR_CHAINS + ue.STITCHED_CHAINS, ids=lambda c: c.id)
def test_lattice_condition_of_the_chains(cc):
    """both stages' sums (asserted inside chain23), and the intermediate images are real bf16 roundings, not small integers; the
    stitched backward folds bf16 tile sums of dz2, which is exact only while they are bf16 integers"""
    r = ue.chain23(cc, ue.chain_inputs(cc))
    assert float(r.h2.max()) > 256 and bool((ue.bf16(r.h2) == r.h2).all())
    assert float(r.S_dz2.max()) <= 256


def _terms(case, inp, what, n_samples, gen):
    """the products behind sampled output elements, enumerated from the definition element by element (gathers, not the tap
    loop of the evaluator): -> (terms [samples, n], the evaluator's values at those elements before the epilogue)"""
    geo, R = case.geo, case.rounding
    f, k, pad, nd = geo.f, geo.k, geo.pad, geo.nd
    Wt = ue.tap_weights(inp.W, geo, "bf16")
    xop = ue.operand(case, inp.x, R)
    dyop = ue.bf16(inp.dy) if R.dy else inp.dy
    xp = ue.up_pad(xop, geo)
    B, g = case.shape[0], list(case.shape[1:])
    rnd = lambda hi, n: torch.randint(0, hi, (n,), generator=gen)       # noqa: E731
    if what == "y":
        n = min(n_samples, B * math.prod(g) * f ** nd * case.cout)
        bs, co = rnd(B, n), rnd(case.cout, n)
        p = [rnd(f * g[d], n) for d in range(nd)]
        cols = [inp.b[co].unsqueeze(1)]
        for kk in geo.taps():
            w = Wt[tuple(pp % f for pp in p) + tuple(torch.full((n,), v) for v in kk) + (co,)]          # [n, Ci]
            cols.append(xp[(bs,) + tuple(p[d] + kk[d] for d in range(nd))] * w)
        return torch.cat(cols, 1), ue.forward_acc(xop, Wt, inp.b, geo)[(bs,) + tuple(p) + (co,)]
    if what == "dx":
        n = min(n_samples, B * math.prod(g) * case.cin)
        bs, ci = rnd(B, n), rnd(case.cin, n)
        i = [rnd(g[d], n) for d in range(nd)]
        cols = []
        for kk in geo.taps():
            for r in itertools.product(range(f), repeat=nd):            # the f^d up-sampled copies of the source pixel
                p = [f * i[d] + r[d] - kk[d] + pad for d in range(nd)]
                ok = torch.ones(n, dtype=torch.bool)
                for d in range(nd):
                    ok &= (p[d] >= 0) & (p[d] < f * g[d])
                pc = [p[d].clamp(0, f * g[d] - 1) for d in range(nd)]
                w = Wt[tuple(pp % f for pp in pc) + tuple(torch.full((n,), v) for v in kk)][torch.arange(n), :, ci]       # [n, Co]
                cols.append(dyop[(bs,) + tuple(pc)] * w * ok.unsqueeze(1))
        return torch.cat(cols, 1), ue.dgrad_acc(dyop, Wt, geo)[(bs,) + tuple(i) + (ci,)]
    n = min(n_samples, 256)
    a = [rnd(f, n) for _ in range(nd)]
    kk = [rnd(k, n) for _ in range(nd)]
    co, ci = rnd(case.cout, n), rnd(case.cin, n)
    rows = []
    for s in range(n):                                                   # per-phase tap gradient: over the batch and the positions
        sl_in = (slice(None),) + tuple(slice(int(a[d][s] + kk[d][s]), int(a[d][s] + kk[d][s]) + f * (g[d] - 1) + 1, f) for d in range(nd))
        sl_out = (slice(None),) + tuple(slice(int(a[d][s]), None, f) for d in range(nd))
        rows.append((xp[sl_in][..., int(ci[s])] * dyop[sl_out][..., int(co[s])]).reshape(-1))
    dWp = ue.wgrad_acc(xop, dyop, geo)[0]
    return torch.stack(rows), dWp[tuple(a) + tuple(kk) + (co, ci)]


def _orders(case, inp, want):
    gen = torch.Generator().manual_seed(77 + case.seed)
    for what, need in (("y", "fwd"), ("dx", "dgrad"), ("dW", "wgrad")):
        if need not in want:
            continue
        terms, val = _terms(case, inp, what, 2048, gen)
        assert torch.equal(terms.sum(1), val), (case.id, what, "the terms are not the evaluator's sum")
        perm = torch.randperm(terms.shape[1], generator=gen)
        for order in (torch.arange(terms.shape[1]), perm):
            t32 = terms[:, order].to(torch.float32)
            assert torch.equal(t32.double(), terms[:, order]), "a product is not an fp32 value"
            acc = torch.zeros(terms.shape[0], dtype=torch.float32)
            for j in range(t32.shape[1]):
                acc = acc + t32[:, j]
            assert torch.equal(acc.double(), val), (case.id, what, "fp32 accumulation order matters")


# ---- the faults ------------------------------------------------------------------------------------------------------------------
def _old_rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize("entry", ue.DISCRIMINATION, ids=[e[0].replace(" ", "_") for e in ue.DISCRIMINATION])
def test_each_fault_changes_its_case(entry):
    """lattice faults: at least one output element differs from the right evaluator (so bit equality with a right kernel fails).
    gridded faults: at least one element is more than TWICE the a-priori bound away from the right evaluator -- a kernel within
    the bound of the right evaluator is then outside the bound of the wrong one.  Printed, not asserted: whether the whole-tensor
    limit of the matching test of test_hip_upsample.py would still pass (the recorded gap)."""
    name, case, kw, out, old_limit, kind = entry
    want = {"y": ("fwd",), "dx": ("dgrad",), "dW": ("wgrad",)}[out]
    if kind == "lattice":
        inp, ref = _lattice(case, want)
        bad = ue.evaluate(case, inp, faults=ue.Faults(**kw), want=want)
        r, w = getattr(ref, out), getattr(bad, out)
        n_diff = int((r != w).sum())
        assert n_diff > 0, name
        print("%-75s lattice: %d of %d elements differ; old limit %.0e would %s (%.1e)"
              % (name, n_diff, r.numel(), old_limit, "PASS" if _old_rel(w, r) < old_limit else "fail", _old_rel(w, r)))
    else:
        inp, ref = ue.gridded(case, want=want)
        _, bad = ue.gridded(case, faults=ue.Faults(**kw), want=want)
        r, w = getattr(ref, out), getattr(bad, out)
        S, n = getattr(ref, "S_" + out), getattr(ref, "n_" + out)
        res_type = {"y": case.out, "dx": case.dx, "dW": "f32"}[out]
        ratio = ((w - r).abs() / ue.bound(r, S, n, res_type)).max()
        assert float(ratio) > 2, (name, float(ratio))
        print("%-75s gridded: worst error / bound %.1f; old limit %.0e would %s (%.1e)"
              % (name, float(ratio), old_limit, "PASS" if _old_rel(w, r) < old_limit else "fail", _old_rel(w, r)))
