"""CPU tests of the fp64 evaluator of the A-transform kernels (tests/atrans_emul.py) and of the host planner rcb_atrans_plan.

  evaluator   its split is ops.Planes.from_float bit for bit; its fma is the correctly rounded fp32 fma (fractions.Fraction);
              without a fault it is the plain fp64 product of the split operands.
  lattice     for every case test_hip_atrans_exact.py runs on the GPU: sum |p| / lsb < 2^24, the split identity, and the fp32
              result equal to the fp64 one under two summation orders -- the premises of its torch.equal.
  planner     rcb_atrans_plan over rows x CU counts x layer lists: the head, the segment table, exact coverage of every (row tile,
              layer, column block) by K slices that partition the contraction, the workspace size, the refusals.
  instances   from the plans of the GPU cases: which run_segment instances they execute (atrans_emul.instances).
  faults      every switch of atrans_emul.FAULTS / WGRAD_FAULTS changes at least one element on every case where it applies, and
              which of them the per-slice limit rel_err < 2e-5 of test_hip_kernels.py would have let through.

The planner is host code inside the kernels' library: the library must be built, a GPU is not needed."""
import ctypes
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

import atrans_emul as ae

from recombiner_amd import ops

F64, F32 = torch.float64, torch.float32

PLAN_ROWS = (1, 37, 255, 256, 257, 300, 4096, 61440)
PLAN_CUS = (1, 8, 64, 104, 256, 304)
PLAN_SIZES = ((1056, 1056, 1056, 99), (1584, 2352, 2352, 147), (528, 272, 51), (2112, 4160, 4160, 195), (224, 40, 8, 33), (33,), (7,),
              (32,), (64, 8, 40), (96, 33, 128, 8, 7, 264, 64, 51))


# ---- the evaluator ----------------------------------------------------------------------------------------------------------------
def test_split_is_planes_from_float():
    gen = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(40, 67, generator=gen) * 0.03, ae.lattice((9, 67), gen), torch.randn(3, 67, generator=gen) * 1e-30,
                   torch.zeros(1, 67)])
    hi, lo = ae.split(x)
    p = ops.Planes.from_float(x)
    assert torch.equal(hi.view(torch.int16), p.hi.contiguous().view(torch.int16))
    assert torch.equal(lo.view(torch.int16), p.lo.contiguous().view(torch.int16))
    assert bool((p.buf[:, :, 67:] == 0).all())
    assert torch.equal(p.float(), hi.float() + lo.float())


def _round_f32(q):
    """Fraction -> nearest fp32 (ties to even, gradual underflow) as a Fraction"""
    if q == 0:
        return q
    e = 0
    a = abs(q)
    while a >= 2:
        a /= 2
        e += 1
    while a < 1:
        a *= 2
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    return round(q / quantum) * quantum              # round(Fraction): half to even


def _fma_triples():
    gen = torch.Generator().manual_seed(2)
    n = 1600
    man = lambda: (torch.randint(1 << 23, 1 << 24, (n,), generator=gen).double() * 2.0 ** -23) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
    ex = lambda lo, hi: torch.pow(2.0, torch.randint(lo, hi, (n,), generator=gen).double())
    a, b = man() * ex(-20, 20), man() * ex(-20, 20)
    c = man() * ex(-20, 20) * (a * b).abs() * ex(-30, 30).to(F32).double()         # c from far below to far above the product
    c = c.to(F32).double()
    tri = [(a, b, c)]
    # constructed ties: (1 + i 2^-12)(1 + j 2^-12) = 1 + (i + j) 2^-12 + i j 2^-24 with i j odd sits half way between two fp32
    # values; c = k 2^-23 keeps it there, c = +-2^-60 (lost in the fp64 sum: the round-to-odd step must remember it) breaks the tie
    ij = [(i, j) for i in range(1, 40, 2) for j in range(1, 40, 2)]
    ti = torch.tensor([1 + i * 2.0 ** -12 for i, _ in ij], dtype=F64)
    tj = torch.tensor([1 + j * 2.0 ** -12 for _, j in ij], dtype=F64)
    for cv in (0.0, 2.0 ** -23, -3 * 2.0 ** -23, 2.0 ** -60, -2.0 ** -60, 2.0 ** -100):
        tri.append((ti, tj, torch.full_like(ti, cv)))
        tri.append((-ti, tj, torch.full_like(ti, -cv)))
    return [torch.cat([t[i] for t in tri]) for i in range(3)]


def test_fma32_is_the_correctly_rounded_fma():
    a, b, c = _fma_triples()
    assert a.numel() >= 2000
    assert torch.equal(a, a.to(F32).double()) and torch.equal(b, b.to(F32).double()) and torch.equal(c, c.to(F32).double())
    got = ae.fma32(a, b, c)
    ties = 0
    for av, bv, cv, gv in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(av) * Fraction(bv) + Fraction(cv)
        want = _round_f32(exact)
        assert Fraction(gv) == want, (av, bv, cv, gv, float(want))
        ties += (exact != want and abs(exact - want) * 2 == Fraction(2) ** -23 and 1 <= abs(exact) < 2)
    assert ties >= 400                                           # the constructed half-way cases are in there
    # the plain fp64 route (round the fp64 sum to fp32) is wrong on some of them: the detour through round-to-odd is needed
    naive = (a * b + c).to(F32).double()
    assert not torch.equal(naive, got)


def test_evaluator_without_faults_is_the_product_of_the_split_operands():
    case = ae.Case((64, 8, 40, 33), 37, 1)
    x, A = ae.case_inputs(case, real=True)
    sl = ae.slices_of(case.sizes)
    for tr in (0, 1):
        o1, _ = ae.apply(x, A, sl, 1, tr)
        o2, _ = ae.apply(x, A, sl, 2, tr)
        o3, s3 = ae.apply(x, A, sl, 3, tr)
        for (a, b), m in zip(sl, A):
            md = (m.t() if tr else m)
            xs = x[:, a:b]
            mh = md.bfloat16().double()
            ml = (md - md.bfloat16().float()).bfloat16().double()
            xh = xs.bfloat16().double()
            xl = (xs - xs.bfloat16().float()).bfloat16().double()
            assert torch.equal(o1[:, a:b], xh @ mh)
            assert float((o2[:, a:b] - (xh + xl) @ mh).abs().max()) < 1e-15
            assert float((o3[:, a:b] - ((xh + xl) @ mh + xh @ ml)).abs().max()) < 1e-15
            # three terms: within 2^-15 relative of the full product (the dropped lo x lo term and the third split)
            full = xs.double() @ md.double()
            assert float((o3[:, a:b] - full).abs().max()) <= 2.0 ** -14 * float(s3[:, a:b].max())
            assert float((o1[:, a:b] - full).abs().max()) > 50 * float((o3[:, a:b] - full).abs().max())


# ---- the lattice premises, for every GPU case ---------------------------------------------------------------------------------------
def test_lattice_split_identity_and_worst_case_budget():
    gen = torch.Generator().manual_seed(3)
    x = ae.lattice((64, 4160), gen)
    hi, lo = ae.split(x)
    a = (x.abs() / 256).floor()
    assert torch.equal(hi.float(), torch.sign(x) * 256 * a) and torch.equal(lo.float(), x - hi.float())
    assert set(lo.float().abs().unique().tolist()) == {0.0, 1.0} and 0.4 < float((lo != 0).float().mean()) < 0.6
    assert set(a.unique().tolist()) == {1.0, 2.0, 3.0}
    # worst case of the three-term form at the longest contraction any preset has: every |x| = |A| = 769
    assert 4160 * (9 * 256 + 3 + 3) < ae.EXACT and abs(4160 * 2310 / ae.EXACT - 0.573) < 1e-3
    A = ae.lattice((4160, 4160), gen)
    b = ae.budget(x, [A], [(0, 4160)])
    assert 0.2 * ae.EXACT < b < 0.35 * ae.EXACT


@pytest.mark.parametrize("case", ae.LATTICE_CASES, ids=ae.case_id)
def test_lattice_case_is_exact_in_fp32_in_any_order(case):
    x, A = ae.case_inputs(case)
    sl = ae.slices_of(case.sizes)
    hi, lo = ae.split(x)
    assert torch.equal(hi.float() + lo.float(), x) and bool((hi.float().abs() % 256 == 0).all()) and bool((lo.float().abs() <= 1).all())
    for m in A:
        mh, ml = ae.split(m)
        assert torch.equal(mh.float() + ml.float(), m) and bool((mh.float().abs() % 256 == 0).all())
    assert ae.budget(x, A, sl) < ae.EXACT
    for tr in (0, 1):
        for terms in (1, 2, 3):
            ref, sabs = ae.apply(x, A, sl, terms, tr)
            assert float(sabs.max()) / 256 < ae.EXACT and bool((ref % 256 == 0).all())
            assert torch.equal(ref.float().double(), ref)
            # fp32 accumulation, ascending and descending contraction index
            for flip in (False, True):
                got = torch.zeros_like(ref, dtype=F32)
                for (a, b), m in zip(sl, A):
                    xh, xl = (t.float() for t in ae.split(x[:, a:b]))
                    mh, ml = (t.float().t() if tr else t.float() for t in ae.split(m))
                    parts = [(xh, mh)] + ([(xl, mh)] if terms >= 2 else []) + ([(xh, ml)] if terms == 3 else [])
                    acc = torch.zeros(case.rows, b - a, dtype=F32)
                    for xp, mp in (parts[::-1] if flip else parts):
                        acc = acc + (xp.flip(1) @ mp.flip(0) if flip else xp @ mp)
                    got[:, a:b] = acc
                assert torch.equal(got.double(), ref), (tr, terms, flip)


@pytest.mark.parametrize("L,rows", ae.WGRAD_CASES)
def test_wgrad_lattice_case_is_exact_in_fp32(L, rows):
    gen = torch.Generator().manual_seed(L * 10007 + rows)
    for lat_first in (True, False):
        h = ae.lattice((rows, L), gen) if lat_first else ae.small_ints((rows, L), gen)
        dw = ae.small_ints((rows, L), gen) if lat_first else ae.lattice((rows, L), gen)
        ref, sabs = ae.wgrad(h, dw)
        assert float(sabs.max()) < ae.EXACT and rows * 769 * 4 < ae.EXACT
        assert torch.equal(h.t() @ dw, ref.float()) and torch.equal((h.flip(0).t() @ dw.flip(0)).double(), ref)
        if rows <= 129:                                           # the fma chain in the kernel's order lands on the same value
            assert torch.equal(ae.wgrad_narrow_chain(h, dw, rows, L, ae.narrow_slabs(rows)).double(), ref)


# ---- the planner --------------------------------------------------------------------------------------------------------------------
def _check_plan(rows, sizes, n_cu):
    pl = ae.read_plan(rows, sizes, n_cu)
    raw, segs, S, n = pl.raw, pl.segs, pl.S, len(sizes)
    where = (rows, sizes, n_cu)
    assert pl.need == pl.written == pl.head + 8 * pl.n_segs, where          # the size query is what the fill writes
    assert pl.n_wg >= 1 and pl.n_segs >= pl.n_wg and 1 <= S <= 8 and raw[3] == 0, where
    nblk = [ae.pad32(L) // 32 for L in sizes]
    for l in range(ae.MAX_LAYERS):
        want = 0 if (S == 1 or l >= n) else min(S, nblk[l])
        assert pl.slabs[l] == want, where
    sb = pl.seg_begin
    assert sb[0] == 0 and sb[-1] == pl.n_segs and bool((np.diff(sb) >= 0).all()), where
    assert bool((raw[ae.PLAN_HEAD + pl.n_wg + 1:pl.head] == 0).all()) and pl.head % 4 == 0, where
    if S > 1:
        assert bool((np.diff(sb) == 1).all()), where                          # one (segment, slice) per workgroup
    lay, row0, cb0, w, c0, c1, slab, z = (segs[:, i].astype(np.int64) for i in range(8))
    L = np.array(sizes)[np.clip(lay, 0, n - 1)]
    nc = np.array(nblk)[np.clip(lay, 0, n - 1)]
    assert bool(((lay >= 0) & (lay < n)).all()) and bool((z == 0).all()), where
    assert bool((row0 % ae.BM == 0).all()) and bool(((row0 >= 0) & (row0 < rows)).all()), where
    assert bool(((w >= 1) & (w <= ae.MAXSEG)).all()) and bool((w[L % 8 != 0] <= 2).all()), where
    assert bool((cb0 >= 0).all()) and bool((cb0 + w <= nc).all()), where
    assert bool(((0 <= c0) & (c0 < c1) & (c1 <= nc)).all()), where
    assert bool(((slab == -1) == (S == 1)).all()) and bool((slab < np.maximum(pl.slabs[lay], 1)).all()), where
    # coverage: one row per (segment, column block of it), sorted by (row tile, layer, column block, slab)
    rep = np.repeat(np.arange(len(w)), w)
    blk = cb0[rep] + (np.arange(len(rep)) - np.repeat(np.cumsum(w) - w, w))
    key = np.stack([row0[rep] // ae.BM, lay[rep], blk, np.maximum(slab[rep], 0), c0[rep], c1[rep], nc[rep]], 1)
    key = key[np.lexsort((key[:, 3], key[:, 2], key[:, 1], key[:, 0]))]
    grp = np.r_[True, (np.diff(key[:, :3], axis=0) != 0).any(1)]
    m_tiles = (rows + ae.BM - 1) // ae.BM
    assert int(grp.sum()) == m_tiles * sum(nblk), where                       # every (row tile, layer, block) is there
    first = np.flatnonzero(grp)
    last = np.r_[first[1:], len(key)] - 1
    idx_in = np.arange(len(key)) - np.repeat(first, np.diff(np.r_[first, len(key)]))
    assert bool((key[:, 3] == idx_in).all()), where                           # slabs 0, 1, .. once each
    want_n = np.ones(len(first), dtype=np.int64) if S == 1 else pl.slabs[key[first, 1]]
    assert bool((last - first + 1 == want_n).all()), where
    assert bool((key[first, 4] == 0).all()) and bool((key[last, 5] == key[last, 6]).all()), where
    inner = ~grp[1:]
    assert bool((key[1:, 4][inner] == key[:-1, 5][inner]).all()), where       # each slice begins where the one before it ends
    D4 = (sum(sizes) + 3) // 4 * 4
    assert pl.ws_floats == (S * rows * D4 if S > 1 else 0), where
    return pl


@pytest.mark.parametrize("sizes", PLAN_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_planner_over_rows_and_cu_counts(sizes):
    seen_S = set()
    for rows, n_cu in itertools.product(PLAN_ROWS, PLAN_CUS):
        seen_S.add(_check_plan(rows, sizes, n_cu).S)
    assert 1 in seen_S and max(seen_S) > 1                                    # both regimes occur for every layer list


@pytest.mark.parametrize("case", ae.LATTICE_CASES + ae.REAL_CASES, ids=ae.case_id)
def test_planner_on_the_gpu_cases(case):
    _check_plan(case.rows, case.sizes, case.n_cu)


def test_planner_refusals():
    lib = ae._planner()
    i32 = ctypes.c_int32
    sizes = (i32 * 3)(224, 40, 33)
    need = lib.rcb_atrans_plan(300, 3, sizes, 8, None, 0)
    assert need > 0
    buf = (i32 * (need + 1))(*([-7] * (need + 1)))
    assert lib.rcb_atrans_plan(300, 3, sizes, 8, buf, need - 1) == -2        # one int short: RCB_ERR_SHAPE, nothing written
    msg = lib.rcb_last_error_string().decode()
    assert "atrans_plan" in msg and str(need) in msg and str(need - 1) in msg
    assert all(v == -7 for v in buf)
    assert lib.rcb_atrans_plan(300, 3, sizes, 8, buf, need) == need and buf[need] == -7 and buf[0] >= 1
    assert lib.rcb_atrans_plan(300, 3, sizes, 8, buf, need + 1) == need
    bad = [(300, 3, None, 8), (300, 0, sizes, 8), (300, 9, (i32 * 9)(*([32] * 9)), 8), (300, 3, (i32 * 3)(224, 0, 33), 8),
           (0, 3, sizes, 8), (300, 3, sizes, 0), (-5, 3, sizes, 8), (300, 3, sizes, -1)]
    for rows, n, sz, cu in bad:
        assert lib.rcb_atrans_plan(rows, n, sz, cu, None, 0) == -1, (rows, n, cu)
        assert "atrans_plan" in lib.rcb_last_error_string().decode()
        assert lib.rcb_atrans_plan(rows, n, sz, cu, buf, need) == -1
    assert lib.rcb_atrans_plan(300, 3, sizes, 8, None, need) == -1           # no buffer, but a size
    with pytest.raises(ae.PlanError):
        ae.read_plan(0, (32,), 8)
    head = (i32 * 12)(1, 1, 4)
    assert lib.rcb_atrans_workspace_floats(300, 3, None, head) == -1 and lib.rcb_atrans_workspace_floats(0, 3, sizes, head) == -1
    assert lib.rcb_atrans_workspace_floats(300, 3, sizes, None) == -1 and lib.rcb_atrans_workspace_floats(300, 9, sizes, head) == -1


# ---- which kernel instances the GPU cases run ------------------------------------------------------------------------------------------
def test_gpu_cases_cover_every_kernel_instance():
    inst = set()
    short_layer = False
    for case in ae.LATTICE_CASES:
        pl = ae.read_plan(case.rows, case.sizes, case.n_cu)
        short_layer |= pl.S > 1 and any(0 < pl.slabs[l] < pl.S for l in range(len(case.sizes)))
        for terms in (1, 2, 3):
            inst |= ae.instances(pl, case.sizes, terms)
    for terms in (1, 2):
        assert {k[0] for k in inst if k[2] == terms and not k[1]} == set(range(1, 8)), terms
    t3 = [k for k in inst if k[2] == 3 and not k[1]]
    assert {k[0] for k in t3 if k[5] is None} == {1, 2, 3, 4}
    assert {k[5] for k in t3 if k[5] is not None} == {(w, h) for w in (5, 6, 7) for h in (0, 1)}
    assert {(k[0], k[5]) for k in t3 if k[5] is not None} == {(3, (5, 0)), (2, (5, 1)), (3, (6, 0)), (3, (6, 1)), (4, (7, 0)), (3, (7, 1))}
    for terms in (1, 2, 3):
        assert {k[0] for k in inst if k[2] == terms and k[1]} == {1, 2}, terms          # ragged
        # every nk class: terms 1 and 2 walk the three-stage ring, terms 3 the two-stage path
        assert {k[3] for k in inst if k[2] == terms and not k[1]} == {1, 2, 3, 4}, terms
        assert {k[3] for k in inst if k[2] == terms and k[1]} >= {1, 2, 4}, terms
        assert {k[4] for k in inst if k[2] == terms and not k[1]} == {False, True}, terms
        assert {k[4] for k in inst if k[2] == terms and k[1]} == {False, True}, terms
    assert short_layer


# ---- the faults -----------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


OLD_LIMIT = 2e-5          # test_hip_kernels.py: max |a - b| / max |b| per layer slice (1e-5 with one term)


@pytest.mark.parametrize("case", ae.LATTICE_CASES, ids=ae.case_id)
def test_every_fault_shows_on_every_lattice_case_it_applies_to(case):
    x, A = ae.case_inputs(case)
    sl = ae.slices_of(case.sizes)
    pl = ae.read_plan(case.rows, case.sizes, case.n_cu)
    applied = set()
    for tr, terms in itertools.product((0, 1), (1, 2, 3)):
        ref, _ = ae.apply(x, A, sl, terms, tr)
        for fault in ae.FAULTS:
            if not ae.fault_applies(fault, case, terms, pl):
                continue
            bad, _ = ae.apply(x, A, sl, terms, tr, fault=fault, plan=pl)
            assert not torch.equal(bad, ref), (fault, terms, tr)
            applied.add(fault)
    assert "rho_swap" in applied or case.rows < 5


def test_every_fault_applies_somewhere_and_what_the_old_limit_saw():
    """every switch applies to at least one GPU case.  For the record (printed, -s): on REAL inputs at the old tests' scales, the
    smallest per-slice rel_err = max |a - b| / max |b| each fault produces over the cases it applies to -- a fault whose figure is
    below 2e-5 (1e-5 with one term) would have passed test_atrans_kernels_forward_and_data_gradient on that case"""
    applied, least = set(), {}
    for case in ae.LATTICE_CASES:
        pl = ae.read_plan(case.rows, case.sizes, case.n_cu)
        sl = ae.slices_of(case.sizes)
        small = sum(case.sizes) <= 700
        if small:
            xr, Ar = ae.case_inputs(case, real=True)
        for terms in (1, 2, 3):
            ref = None
            for fault in ae.FAULTS:
                if not ae.fault_applies(fault, case, terms, pl):
                    continue
                applied.add(fault)
                if small:
                    ref = ae.apply(xr, Ar, sl, terms, 0)[0] if ref is None else ref
                    bad = ae.apply(xr, Ar, sl, terms, 0, fault=fault, plan=pl)[0]
                    worst = max(_rel(bad[:, a:b], ref[:, a:b]) for a, b in sl) / (OLD_LIMIT if terms >= 2 else 1e-5)
                    least[fault] = min(least.get(fault, float("inf")), worst)
    assert applied == set(ae.FAULTS)
    print("smallest rel_err / old limit per fault on real inputs:", {k: "%.3g" % v for k, v in sorted(least.items())})


def test_wgrad_faults_show():
    gen = torch.Generator().manual_seed(5)
    for L, rows in ae.WGRAD_CASES:
        if L > 32:
            h, dw = ae.lattice((rows, L), gen), ae.small_ints((rows, L), gen)
            assert not torch.equal(ae.wgrad(h, dw, fault="kn_swapped")[0], ae.wgrad(h, dw)[0]), (L, rows)
    # a slab boundary that is not rounded to 8 changes no exact sum, only the order: it shows where the order does, on the
    # real-valued chain case of test_hip_atrans_exact.py (70 rows, L = 33: two slabs of 40 and 30 rows, not 35 and 35)
    h, dw = ae.chain_inputs()
    good = ae.wgrad_narrow_chain(h, dw, 70, 33, ae.narrow_slabs(70))
    assert ae.narrow_slabs(70) == 2
    assert not torch.equal(ae.wgrad_narrow_chain(h, dw, 70, 33, 2, fault="slab_not_rounded8"), good)
    # and the chain is a rounding of the product, nothing else
    ref, sabs = ae.wgrad(h, dw)
    assert bool(((good.double() - ref).abs() <= (70 + 4 + 2) * ae.EPS32 * sabs).all())
    assert not torch.equal(good, ref.float())                    # the order matters on these inputs: the bit check says something
