"""The A-transform kernels (atrans.hip: atrans_kernel<terms, planes> with its 26 run_segment instances, atrans_slab_sum_kernel,
atrans_pack_kernel, wgrad_narrow_kernel + wgrad_narrow_sum_kernel) and the glue of ops.ATransform against the fp64 evaluator of
tests/atrans_emul.py.

  lattice    x and A from s (256 a + b): every product of every term form is a multiple of 256 and every fp32 partial sum is exact
             in any order (test_atrans_emul_cpu.py asserts sum |p| / 256 < 2^24 for each case), so the kernel must return the
             evaluator's value BIT FOR BIT -- torch.equal, no element exempt.  A failure names the first differing element.
  packed     the four planes of rcb_atrans_pack against their definition, zero padding included.
  locality   a NaN in one (row, layer) of x changes that (row, layer) of the output and nothing else, bit for bit.
  real       x = 0.03 randn, A = randn / sqrt(n): every element within n 2^-23 sum |p| of the fp64 product of the split operands,
             n = products accumulated + K slices: the any-order, any-rounding-mode cap of n fp32 additions.  Derived, not measured.
  wgrad      the narrow kernel on lattice x small-integer operands (exact), the batched bf16 GEMM and the fp32 GEMM paths of
             ATransform.wgrad on operands where they are exact too, and on real inputs the narrow kernel against the fp32 fma
             chain in row order that atrans.hip claims it is (atrans_emul.wgrad_narrow_chain).

Every test pins tr.n_cu to a CU count whose plan test_atrans_emul_cpu.py analysed (atrans_emul.LATTICE_CASES / REAL_CASES): the
plan, and so the kernel instances that run, do not depend on the device.

Worst |got - ref| / bound on real inputs, first MI355X run (for information; no limit is derived from it): see RATIOS."""
import pytest
import torch

import atrans_emul as ae

from recombiner_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16

RATIOS = """
worst over the elements, both directions, fp32 rows and planes (bit-identical), per case and number of terms:
[224, 40, 8, 33]  257 rows, 256 CUs    1 term 0.031   2 terms 0.031   3 terms 0.034
[224, 40, 8, 33]   33 rows, 256 CUs    1 term 0.024   2 terms 0.017   3 terms 0.021     (K-split, S = 8)
[1056, 99]        300 rows,   1 CU     1 term 0.008   2 terms 0.005   3 terms 0.005
[528, 272, 51]      1 row,  256 CUs    1 term 0.005   2 terms 0.003   3 terms 0.004     (K-split)
narrow weight gradient, 70 rows, L = 33: 0 of 1089 elements differ from the fma chain; against fp64, error / bound 0.007
"""


def g(t):
    return t.to(DEV)


def _first_diff(got, ref, slices):
    bad = (got != ref) | (got.isnan() != ref.isnan())
    r, c = (int(v) for v in bad.nonzero()[0])
    l = next(i for i, (a, b) in enumerate(slices) if a <= c < b)
    return "%d elements differ; first: row %d, layer %d, column %d of it: got %r, expected %r" % (
        int(bad.sum()), r, l, c - slices[l][0], float(got[r, c]), float(ref[r, c]))


def _assert_equal(got, ref, slices, what):
    ref = ref.to(got.device)
    assert torch.equal(got, ref), "%s: %s" % (what, _first_diff(got, ref, slices))


def _transform(case, terms, dgrad_terms=None):
    tr = ops.ATransform(ae.slices_of(case.sizes), DEV, terms=terms, dgrad_terms=dgrad_terms)
    tr.n_cu = case.n_cu                                   # before the first call: plans are made (and kept) per row count
    return tr


# ---- lattice: bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ae.LATTICE_CASES, ids=ae.case_id)
def test_lattice_forward_and_data_gradient_equal_the_evaluator(case):
    x, A = ae.case_inputs(case)
    sl = ae.slices_of(case.sizes)
    rows, D = case.rows, sum(case.sizes)
    xg, Ag = g(x), [g(a) for a in A]
    planes = ops.Planes.from_float(xg)
    assert torch.equal(planes.float(), xg)
    ref = {(t, tr): ae.apply(x, A, sl, t, tr)[0].to(F32) for t in (1, 2, 3) for tr in (0, 1)}
    for terms in (1, 2, 3):
        tr = _transform(case, terms)
        tr.prepare(Ag)
        for form, src in (("rows", xg), ("planes", planes)):
            out = torch.full((rows, D), float("nan"), device=DEV)
            _assert_equal(tr.forward(src, out), ref[terms, 0], sl, "forward, terms %d, %s" % (terms, form))
            out = torch.full((rows, D), float("nan"), device=DEV)
            _assert_equal(tr.dgrad(src, out), ref[terms, 1], sl, "dgrad, terms %d, %s" % (terms, form))
        for dt in range(1, terms):                       # fewer terms in the data gradient than in the forward: same images
            tr2 = _transform(case, terms, dgrad_terms=dt)
            tr2.prepare(Ag)
            for form, src in (("rows", xg), ("planes", planes)):
                out = torch.full((rows, D), float("nan"), device=DEV)
                _assert_equal(tr2.dgrad(src, out), ref[dt, 1], sl, "dgrad, terms %d of %d, %s" % (dt, terms, form))
                out = torch.full((rows, D), float("nan"), device=DEV)
                _assert_equal(tr2.forward(src, out), ref[terms, 0], sl, "forward, terms %d (dgrad %d), %s" % (terms, dt, form))


@pytest.mark.parametrize("case", [ae.Case((224, 40, 8, 33), 257, 256), ae.Case((528, 272, 51), 33, 256), ae.Case((1056, 99), 300, 1)],
                         ids=ae.case_id)
def test_lattice_strided_views_and_untouched_border(case):
    """x as a view at a row offset, a column offset of 2 and a row stride that is no multiple of 4 floats; the output as the inner
    view of a buffer filled with a sentinel: the result is the evaluator's, the border keeps its bits"""
    x, A = ae.case_inputs(case)
    sl = ae.slices_of(case.sizes)
    rows, D = case.rows, sum(case.sizes)
    big = torch.full((rows + 3, D + 5 + ((D + 5) % 4 == 0)), float("nan"))
    big[1:rows + 1, 2:D + 2] = x
    assert big.stride(0) % 4 != 0
    xv = g(big)[1:rows + 1, 2:D + 2]
    sentinel = -12345.678
    for terms in (1, 2, 3):
        tr = _transform(case, terms)
        tr.prepare([g(a) for a in A])
        for direction in (0, 1):
            buf = torch.full((rows + 2, D + 3), sentinel, device=DEV)
            inner = buf[1:rows + 1, 1:D + 1]
            inner.fill_(float("nan"))
            (tr.dgrad if direction else tr.forward)(xv, inner)
            _assert_equal(inner, ae.apply(x, A, sl, terms, direction)[0].to(F32), sl, "terms %d, direction %d" % (terms, direction))
            border = torch.ones_like(buf, dtype=torch.bool)
            border[1:rows + 1, 1:D + 1] = False
            assert torch.equal(buf[border], torch.full((int(border.sum()),), sentinel, device=DEV))


def test_planes_on_a_layer_off_a_multiple_of_8_columns_are_refused():
    tr = ops.ATransform(ae.slices_of((33, 64)), DEV, terms=2)
    tr.n_cu = 8
    gen = torch.Generator().manual_seed(4)
    x, A = g(ae.lattice((40, 97), gen)), [g(ae.lattice((n, n), gen)) for n in (33, 64)]
    tr.prepare(A)
    out = torch.zeros(40, 97, device=DEV)
    with pytest.raises(ops.RcbError, match="multiple of 8"):
        tr.forward(ops.Planes.from_float(x), out)
    assert not bool(out.any())
    ref = ae.apply(x.cpu(), [a.cpu() for a in A], tr.slices, 2, 0)[0].to(F32)     # fp32 rows have no such condition
    _assert_equal(tr.forward(x, out), ref, tr.slices, "fp32 rows")


# ---- packed images --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(224, 40, 8, 33), (99,), (7,), (30, 64, 51), (528, 272, 51)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["lattice", "real"])
def test_packed_images_are_their_definition(sizes, kind):
    """sizes with L % 4 != 0 (the scalar load path), L % 32 != 0 (padding) and L < 32"""
    gen = torch.Generator().manual_seed(sum(sizes))
    A = [ae.lattice((n, n), gen) if kind == "lattice" else torch.randn(n, n, generator=gen) / n ** 0.5 for n in sizes]
    plane = sum(ae.pad32(n) ** 2 for n in sizes)
    for want_lo in (0, 1):
        tr = ops.ATransform(ae.slices_of(sizes), DEV, terms=3 if want_lo else 2)
        assert tr.packed.numel() == 4 * plane
        pattern = (torch.arange(4 * plane, device=DEV) % 251 + 1).to(BF)
        tr.packed.copy_(pattern)
        tr.prepare([g(a) for a in A])
        want = ae.packed_images(A, want_lo)
        for i, name in enumerate(("forward hi", "data-gradient hi", "forward lo", "data-gradient lo")):
            got = tr.packed[i * plane:(i + 1) * plane]
            exp = g(want[i]) if want[i] is not None else pattern[i * plane:(i + 1) * plane]        # want_lo = 0: untouched
            same = got.view(torch.int16) == exp.view(torch.int16)
            assert bool(same.all()), "%s, want_lo %d: %d elements differ, first at %d" % (name, want_lo, int((~same).sum()),
                                                                                         int((~same).nonzero()[0]))


# ---- row and layer locality -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cu", [256, 1])
def test_a_nan_stays_in_its_row_and_layer(n_cu):
    case = ae.Case((224, 40, 8, 33), 257, n_cu)
    x, A = ae.case_inputs(case, real=True)
    sl = ae.slices_of(case.sizes)
    for terms in (2, 3):
        tr = _transform(case, terms)
        tr.prepare([g(a) for a in A])
        for as_planes in (False, True):
            give = (lambda t: ops.Planes.from_float(g(t))) if as_planes else g
            clean = [tr.forward(give(x), torch.empty(257, 305, device=DEV)).clone(), tr.dgrad(give(x), torch.empty(257, 305, device=DEV)).clone()]
            for r, l in ((0, 0), (255, 1), (256, 2), (256, 3), (0, 3), (255, 0)):
                a, b = sl[l]
                xn = x.clone()
                xn[r, a:b] = float("nan")
                for direction in (0, 1):
                    out = (tr.dgrad if direction else tr.forward)(give(xn), torch.empty(257, 305, device=DEV))
                    keep = torch.ones(257, 305, dtype=torch.bool, device=DEV)
                    keep[r, a:b] = False
                    assert bool(out[r, a:b].isnan().all()), (terms, as_planes, r, l, direction)
                    assert torch.equal(out[keep].view(torch.int32), clean[direction][keep].view(torch.int32)), (terms, as_planes, r, l, direction)


# ---- real inputs, element by element --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ae.REAL_CASES, ids=ae.case_id)
def test_real_inputs_within_the_any_order_cap(case):
    x, A = ae.case_inputs(case, real=True)
    sl = ae.slices_of(case.sizes)
    rows, D = case.rows, sum(case.sizes)
    S = ae.read_plan(case.rows, case.sizes, case.n_cu).S
    xg, Ag = g(x), [g(a) for a in A]
    worst = {}
    for terms in (1, 2, 3):
        tr = _transform(case, terms)
        tr.prepare(Ag)
        for direction in (0, 1):
            ref, sabs = ae.apply(x, A, sl, terms, direction)
            n = torch.cat([torch.full((b - a,), float(ae.n_products(b - a, terms) + S), dtype=F64) for a, b in sl])
            bound = n * ae.EPS32 * sabs
            for src in (xg, ops.Planes.from_float(xg)):
                got = (tr.dgrad if direction else tr.forward)(src, torch.full((rows, D), float("nan"), device=DEV)).cpu().double()
                ratio = ((got - ref).abs() / bound)
                worst[terms] = max(worst.get(terms, 0.0), float(ratio.max()))
                print("%s terms %d direction %d: worst |got - ref| / bound = %.4g" % (ae.case_id(case), terms, direction, float(ratio.max())))
                assert bool(torch.isfinite(got).all()) and bool((ratio <= 1).all()), (terms, direction, float(ratio.max()))


# ---- weight gradient ------------------------------------------------------------------------------------------------------------------
def _narrow(h, dw, forms):
    """dA of a single narrow layer through ATransform.wgrad; forms: (h as planes, dw as planes).  L = 256 alone would be the
    widest layer and go to the batched bf16 GEMM: a 264-wide layer of zeros in front keeps it on the narrow kernel"""
    rows, L = h.shape
    front = 264 if L >= 256 else 0
    tr = ops.ATransform(ae.slices_of((front, L)) if front else [(0, L)], DEV, terms=2)
    hg, dg = (g(torch.cat([torch.zeros(rows, front), t], 1)) for t in (h, dw))
    gA = tr.wgrad(ops.Planes.from_float(hg) if forms[0] else hg, ops.Planes.from_float(dg) if forms[1] else dg)
    assert len(gA) == 1 + bool(front) and not (front and bool(gA[0].any()))
    return gA[-1]


@pytest.mark.parametrize("L,rows", ae.WGRAD_CASES)
def test_narrow_weight_gradient_is_exact_on_the_lattice(L, rows):
    gen = torch.Generator().manual_seed(L * 10007 + rows)                   # the inputs test_atrans_emul_cpu.py budgeted
    for lat_first in (True, False):
        h = ae.lattice((rows, L), gen) if lat_first else ae.small_ints((rows, L), gen)
        dw = ae.small_ints((rows, L), gen) if lat_first else ae.lattice((rows, L), gen)
        ref = g(ae.wgrad(h, dw)[0].to(F32))
        for forms in ((False, False), (True, False), (False, True), (True, True)):
            got = _narrow(h, dw, forms)
            assert torch.equal(got, ref), (lat_first, forms, int((got != ref).sum()), (got != ref).nonzero()[0].tolist())


def test_narrow_weight_gradient_inside_a_wider_row():
    """the layer as columns 40..139 of wider rows (strides and layer offsets of both operand forms), other layers next to it"""
    gen = torch.Generator().manual_seed(9)
    sizes, rows = (40, 99, 31), 129
    h, dw = ae.lattice((rows, 170), gen), ae.small_ints((rows, 170), gen)
    tr = ops.ATransform(ae.slices_of(sizes), DEV, terms=2)
    for forms in ((False, False), (True, True), (True, False)):
        got = tr.wgrad(ops.Planes.from_float(g(h)) if forms[0] else g(h), ops.Planes.from_float(g(dw)) if forms[1] else g(dw))
        for (a, b), gl in zip(tr.slices, got):
            assert torch.equal(gl, g(ae.wgrad(h[:, a:b], dw[:, a:b])[0].to(F32))), (forms, a, b)


def test_wide_and_fp32_gemm_paths_are_exact_on_the_lattice():
    """[256, 256, 40]: the two widest layers take one batched bf16 GEMM through as_strided views -- with the bf16 copies handed
    over, cast on the spot, and as the hi planes; lattice hi x small integers is exact there.  [272, 264, 33]: 264 is above
    256 and not the widest: the fp32 GEMM path"""
    gen = torch.Generator().manual_seed(10)
    rows = 70
    for sizes in ((256, 256, 40), (272, 264, 33)):
        D = sum(sizes)
        h, dw = ae.lattice((rows, D), gen), ae.small_ints((rows, D), gen)
        hi = ae.split(h)[0].float()
        tr = ops.ATransform(ae.slices_of(sizes), DEV, terms=2)
        hg, dg = g(h), g(dw)
        ld = (D + 7) // 8 * 8
        h16 = torch.zeros(rows, ld, device=DEV, dtype=BF)[:, :D]
        h16.copy_(hg)
        d16 = torch.zeros(rows, ld + 8, device=DEV, dtype=BF)[:, :D]
        d16.copy_(dg)
        runs = {"cast inside": tr.wgrad(hg, dg), "h16 given": tr.wgrad(hg, dg, h16, None), "both given": tr.wgrad(hg, dg, h16, d16),
                "planes": tr.wgrad(ops.Planes.from_float(hg), ops.Planes.from_float(dg)),
                "fp32": tr.wgrad(hg, dg, bf16_hi=False), "planes, fp32": tr.wgrad(ops.Planes.from_float(hg), dg, bf16_hi=False)}
        big = max(sizes)
        for name, got in runs.items():
            for (a, b), gl in zip(tr.slices, got):
                hh = hi if (b - a == big and "fp32" not in name) else h               # the wide path keeps the hi part of h alone
                ref, sabs = ae.wgrad(hh[:, a:b], dw[:, a:b])
                assert float(sabs.max()) < ae.EXACT
                assert torch.equal(gl, g(ref.to(F32))), (sizes, name, a, b)


def test_narrow_weight_gradient_is_the_fma_chain_in_row_order():
    """atrans.hip: `bit for bit a chain of fmaf in row order` -- v_mfma_f32_32x32x2_f32 as two single-rounding fmas per
    instruction, k = 0 first.  Real inputs, 70 rows, L = 33: two slabs (40 + 30 rows), four tiles, ragged in both directions"""
    h, dw = ae.chain_inputs()
    want = ae.wgrad_narrow_chain(h, dw, 70, 33, ae.narrow_slabs(70))
    ref, sabs = ae.wgrad(h, dw)
    for forms in ((False, False), (True, True)):
        hh = ops.Planes.from_float(h).float() if forms[0] else h            # planes: the operand IS hi + lo
        dd = ops.Planes.from_float(dw).float() if forms[1] else dw
        if forms[0]:
            want_f, (ref_f, sabs_f) = ae.wgrad_narrow_chain(hh, dd, 70, 33, 2), ae.wgrad(hh, dd)
        else:
            want_f, ref_f, sabs_f = want, ref, sabs
        got = _narrow(h, dw, forms).cpu()
        err = (got.double() - ref_f).abs() / ((70 + 4 + 2) * ae.EPS32 * sabs_f)
        print("narrow wgrad, planes %s: %d of %d elements differ from the fma chain; worst |got - ref64| / bound = %.4g"
              % (forms[0], int((got != want_f).sum()), got.numel(), float(err.max())))
        assert bool((err <= 1).all())
        assert torch.equal(got, want_f), "%d of %d elements differ from the chain" % (int((got != want_f).sum()), got.numel())
