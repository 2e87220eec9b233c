"""The posterior-path kernels (posterior.hip, posterior_bodies.h, the helpers of rcb_common.h) against the evaluator of
tests/posterior_emul.py, whose premises test_posterior_emul_cpu.py checks on the CPU.

The approximated pieces are observed alone through the C ABI ("taps"), bounded once against fp64, and their device values are fed
into the evaluator, so that everything built from them with exactly rounded fp32 glue compares BIT FOR BIT:

  taps       st_f32 (rcb_softplus_scale), dst_f32 (the generic rcb_posterior_bwd with d_out = eps = 1, S = 1, no KL, no Adam:
             g_log_scale = 1 * dst), kl_elem_f32 (rcb_gauss_kl with one-element segments), Adam (rcb_adam_flat), the noise
             (rcb_philox_normal): swept against fp64 within the bounds DERIVED in posterior_emul's docstring.
  bit exact  the sampler on every layout case (real inputs, sigma tap); the gradient gather on lattice inputs, as gradients and through
             the Adam moments from zero state; Adam's m and v; kl_group as the ascending fp64 sum of the tapped elements; the
             fixed-point column moments as Python integers; beta_update; which noise the fused samplers draw.
  bounded    gradients with the KL part, the updated parameters, the KL log, kl_row, the KL column sums: element by element inside
             the derived bounds.
Every layout case runs under the default dispatch and under rcb_debug_generic_kernels_only(1), and BOTH are compared with the evaluator,
not with each other.  A failure names the first differing element.

PINNED: NaN in gives NaN out of st_f32 and dst_f32 (dst_f32 clamped its argument with fminf, which drops a NaN: dst_f32(NaN) was the
finite value of -80 until this suite found it).  st_f32(+-inf) is NaN (softplus gives inf and 0): exp_fast forms inf - inf.
dst_f32(+inf) is 1/6 and dst_f32(-inf) is 0, the reference's values; a finite x < -80, outside the swept range, gives dst_f32(-80).  A uniform u1 that rounds to exactly 1 gives a normal of exactly 0
(posterior_emul.philox_normal_ref).

PHILOX_LIMIT: the absolute error of v_sin / v_cos / v_log / v_sqrt is not documented; worst |noise - fp64 Box-Muller| over 2^22 draws on
the first MI355X run was PHILOX_MEASURED = 7.86e-7 (at |eps| = 4.43); the asserted limit is 4x that (one seed undersamples the tail), and never above 1e-5: a
wrong stream differs by O(1).

Worst |got - ref| / bound of every bounded check on the first MI355X run (for information; no limit is derived from it): see RATIOS."""
import contextlib

import numpy as np
import pytest
import torch

import posterior_emul as pe
from golden_util import O

from recombiner_amd import _lib, ops
from recombiner_amd.ops import LevelSpec

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = np.float32, np.float64
PHILOX_MEASURED = 7.86e-7
PHILOX_LIMIT = min(4 * PHILOX_MEASURED, 1e-5)

RATIOS = """
st_f32 / (6 ulp)                    0.642   (3.9 ulp)        dst_f32 / (5 ulp)                  0.581   (2.9 ulp)
kl_elem_f32 / bound, grid           0.565                    kl_elem_f32 / bound, case data     0.524
g_loc / bound                       0.539                    g_log_scale / bound                0.395
m_loc / bound (kernels without      0.520                    m_ls / bound (the same)            0.415
  gradient outputs)
updated parameter / bound           0.999   (the 1/2 ulp of the closing addition is reached)
Adam alone, p / bound               1.000   (the same)
KL log / bound                      0.108                    kl_colsum / bound                  0.087
kl_row / bound, segments            0.002                    kl_row / bound, no segments      < 0.001
share of gradient elements bit-equal to the rounded fp64 value: 0.43 - 0.67 per case, 0.51 typical
"""

UPDATE_LEVELS = [(c, li) for c in pe.CASES if c.update for li in range(len(c.levels))]
lid = lambda p: "%s-L%d" % (p[0].name, p[1])          # noqa: E731
SEEN = {}


def note(key, ratio):
    """keep and print the worst ratio of a bounded check (the RATIOS block is filled from this output)"""
    if float(ratio) > SEEN.get(key, -1.0):
        SEEN[key] = float(ratio)
        print("RATIO %-44s %.3f" % (key, SEEN[key]))


def g(a, dtype=None):
    if a is None:
        return None
    t_ = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t_ if dtype is None else t_.to(dtype)).to(DEV).contiguous()


def cpu(t_):
    return t_.detach().cpu().numpy()


@contextlib.contextmanager
def dispatch(generic):
    lib = _lib.load()
    old = lib.rcb_debug_generic_kernels_only(int(generic))
    try:
        yield
    finally:
        lib.rcb_debug_generic_kernels_only(old)


def st_tap(x):
    return cpu(ops.softplus_scale(g(pe.f32(x))))


def dst_tap(x):
    """dst_f32 of every element of x through the generic update kernel: S = 1, d_out = eps = 1, kl_scalar = 0, gradients out"""
    x = pe.f32(x)
    flat = x.reshape(-1)
    out = np.empty_like(flat)
    chunk = 4 << 18
    with dispatch(True):
        for a in range(0, flat.size, chunk):
            part = flat[a:a + chunk]
            cols = min(part.size, 1 << 18)
            rows = pe.cdiv(part.size, cols)
            buf = np.zeros(rows * cols, F32)
            buf[:part.size] = part
            ls = g(buf.reshape(rows, cols))
            one = torch.ones(rows, 1, cols, device=DEV)
            lv = LevelSpec(torch.zeros_like(ls), ls, cols, rows)
            _, gls = ops.posterior_bwd(lv, torch.zeros(cols, device=DEV), torch.ones(cols, device=DEV), False, 0.0, one, one, 1,
                                       want_grads=True)
            out[a:a + chunk] = cpu(gls).reshape(-1)[:part.size]
    return out.reshape(x.shape)


def kl_tap(loc, ls, p_loc, p_scale, p_is_log=False):
    """kl_elem_f32 of every element: one-element segments, kl_group[r, g] is the element as a double"""
    cols = loc.shape[1]
    s = torch.arange(cols, device=DEV, dtype=torch.int32)
    _, grp = ops.gauss_kl(g(loc), g(ls), g(p_loc), g(p_scale), p_is_log, seg_start=s, seg_end=s + 1, want_rows=False, want_groups=True)
    return cpu(grp)


def floats_between(lo, hi):
    a, b = (int(v) for v in np.array([lo, hi], F32).view(np.int32))
    return np.arange(min(a, b), max(a, b) + 1, dtype=np.int32).view(F32)


def floats_around(x, n):
    i = int(np.array([x], F32).view(np.int32)[0])
    return np.arange(i - n, i + n + 1, dtype=np.int32).view(F32)


_sweep = {}


def sweep_points():
    if not _sweep:
        r = np.random.RandomState(1)
        _sweep["x"] = np.concatenate([floats_around(20.0, 1 << 10), floats_between(-4.17, -4.15),
                                      pe.f32(r.uniform(-80, 80, 1 << 22)), pe.f32([88.5, 88.8, 89.0, 100.0, 1e4, 3e38])])
    return _sweep["x"]


def first_diff(got, ref, names):
    bad = (got != ref) | (np.isnan(got) != np.isnan(ref))
    idx = tuple(int(v[0]) for v in np.nonzero(bad))
    return "%d of %d elements differ; first at (%s) = %r: got %r, expected %r" % (int(bad.sum()), bad.size, names, idx, got[idx], ref[idx])


def assert_equal(got, ref, what, names):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    assert np.array_equal(got, ref, equal_nan=True), "%s: %s" % (what, first_diff(got, ref, names))


def assert_within(got, ref, bound, what, key=None):
    err = np.abs(got.astype(F64) - ref)
    ok = err <= bound
    if key is not None:
        note(key, np.max(err / np.maximum(bound, 1e-300)))
    if not ok.all():
        idx = tuple(int(v[0]) for v in np.nonzero(~ok))
        raise AssertionError("%s: %d of %d elements outside the bound; first %r: got %r, ref %r, |diff| %.3e, bound %.3e" % (
            what, int((~ok).sum()), ok.size, idx, got[idx], ref[idx], err[idx], np.broadcast_to(bound, err.shape)[idx]))


# ---- 1. function sweeps ----------------------------------------------------------------------------------------------------------------
def test_softplus_scale_sweep():
    x = sweep_points()
    got = st_tap(x)
    ref = pe.st_ref(x)
    assert_within(got, ref, pe.ST_ULPS * pe.ulp(ref), "st_f32", "st_f32 / (ST_ULPS ulp)")
    sw = floats_between(-4.17, -4.15)
    assert sw.size > 30000 and (np.exp(sw.astype(F64)) < 2.0 ** -6).any() and (np.exp(sw.astype(F64)) > 2.0 ** -6).any()
    edge = st_tap(pe.f32([np.nan, np.inf, -np.inf]))
    assert np.isnan(edge).all()                       # pinned: NaN in, NaN out; +-inf -> NaN (rcb_common.h), never another finite number


def test_softplus_derivative_sweep():
    x = sweep_points()
    got = dst_tap(x)
    ref = pe.dst_ref(x)
    assert_within(got, ref, pe.DST_ULPS * pe.ulp(ref), "dst_f32", "dst_f32 / (DST_ULPS ulp)")
    edge = dst_tap(pe.f32([np.nan, np.inf, -np.inf, -80.0, -1000.0]))
    assert np.isnan(edge[0]) and edge[1] == F32(1.0 / 6.0)
    assert edge[2] == 0 and not np.signbit(edge[2])                                 # -inf: the reference's 0
    assert edge[3] == edge[4] and 0 < edge[3] < 4e-36                               # pinned: finite arguments are clamped at -80


# ---- 2. KL element ---------------------------------------------------------------------------------------------------------------------
def kl_grid():
    r = np.random.RandomState(2)
    ls_c = np.repeat(np.linspace(-6, -2, 8), 33)
    ratio = np.tile(np.r_[2.0 ** np.arange(-8, 9), 1.37 * 2.0 ** np.arange(-8, 8)], 8)
    sig = st_tap(pe.f32(ls_c))
    p_scale = pe.f32(sig / pe.f32(ratio))
    p_loc = pe.f32(0.01 * r.randn(ls_c.size))
    tv = np.r_[0.0, 2.0 ** np.arange(-10, 9), -2.0 ** np.arange(-10, 9), r.uniform(-256, 256, 25)]
    loc = pe.f32(p_loc[None, :] + pe.f32(tv)[:, None] * p_scale[None, :])
    loc[0] = p_loc                                                            # q = p exactly where ratio = 1
    ls = np.broadcast_to(pe.f32(ls_c)[None, :], loc.shape).copy()
    return loc, ls, np.broadcast_to(sig[None, :], loc.shape), p_loc, p_scale


def test_kl_element_on_a_grid():
    loc, ls, sig, p_loc, p_scale = kl_grid()
    got = kl_tap(loc, ls, p_loc, p_scale)
    ref, _ = pe.kl_ref(loc, sig, p_loc[None, :], p_scale[None, :])
    r = (sig / p_scale[None, :]).astype(F64)
    assert r.min() <= 2.0 ** -8 * 1.001 and r.max() >= 2.0 ** 8 * 0.999 and np.abs((loc - p_loc) / p_scale).max() > 255
    same = (sig == p_scale[None, :]) & (loc == p_loc[None, :])
    assert same.sum() >= 8 and np.all(got[same] == 0)
    assert_within(got, ref, pe.kl_bound(loc, sig, p_loc[None, :], p_scale[None, :]), "kl_elem_f32", "kl_elem_f32 / bound")


# ---- the layout cases ------------------------------------------------------------------------------------------------------------------
_levels = {}


def level(case, li, lattice=False):
    key = (case.name, li, lattice)
    if key not in _levels:
        L = pe.level_data(case, li, lattice, O.column_row_perms)
        L.sig, L.dst, L.sp = st_tap(L.ls), dst_tap(L.ls), st_tap(L.p_ls)
        assert_within(L.sig, pe.st_ref(L.ls), pe.ST_ULPS * pe.ulp(pe.st_ref(L.ls)), "sigma tap")
        _levels[key] = L
    return _levels[key]


def spec(L):
    return LevelSpec(g(L.loc.copy()), g(L.ls.copy()), L.cols_out, L.n, row_map=L.row_map, row_perm=L.row_perm, col_map=L.col_map,
                     enc_sample=g(L.z), enc_mask=g(L.mask), scale_is_sigma=L.scale_is_sigma)


# ---- 3. sampler ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pe.CASES, ids=pe.case_id)
def test_sampler_equals_the_fp32_chain(case):
    levels = [level(case, li) for li in range(len(case.levels))]
    ref = pe.sample(levels)
    for generic in (False, True):
        with dispatch(generic):
            out = ops.reparam_fwd([spec(L) for L in levels], [g(L.eps) for L in levels], case.S)
        assert_equal(cpu(out), ref, "%s, %s" % (case.name, pe.fwd_reached(case, generic)), "n, s, d")


# ---- 4. gradient gather on the lattice ---------------------------------------------------------------------------------------------------
def update_args(L, case):
    kw = {}
    if case.beta:
        kw = dict(beta=g(L.beta), group_idx=g(L.group_idx.astype(np.int32)), n_groups=len(L.seg_start))
    return kw


def zero_state(lv):
    return {k: torch.zeros_like(lv.loc) for k in ("m_loc", "v_loc", "m_ls", "v_ls")}


@pytest.mark.parametrize("case,li", UPDATE_LEVELS, ids=map(lid, UPDATE_LEVELS))
def test_lattice_gather_is_exact(case, li):
    L = level(case, li, lattice=True)
    g_mu, g_sig = pe.gather32(L)
    g_ls = pe.f32(g_sig * L.dst)
    s = pe.adam_scalars(2e-4, 1)
    moments = lambda gr: (pe.f32(s.w1 * gr), pe.f32(pe.f32(s.w2 * gr) * gr))           # noqa: E731
    for generic in (False, True):
        with dispatch(generic):
            lv = spec(L)
            gl, gs = ops.posterior_bwd(lv, g(L.p_loc), g(L.p_ls), True, 0.0, g(L.d_out), g(L.eps), L.S, want_grads=True, **update_args(L, case))
            what = "%s level %d, %s" % (case.name, li, pe.bwd_reached(case, li, False, True, generic))
            assert_equal(cpu(gl), g_mu, what + ": g_loc", "r, j")
            assert_equal(cpu(gs), g_ls, what + ": g_log_scale", "r, j")
            assert_equal(cpu(lv.loc), L.loc, what + ": loc untouched", "r, j")
            lv = spec(L)
            st = zero_state(lv)
            ops.posterior_bwd(lv, g(L.p_loc), g(L.p_ls), True, 0.0, g(L.d_out), g(L.eps), L.S, adam=ops.adam_cfg(2e-4, 1), state=st,
                              **update_args(L, case))
            what = "%s level %d, %s" % (case.name, li, pe.bwd_reached(case, li, True, False, generic))
            for name, gr in (("loc", g_mu), ("ls", g_ls)):
                m, v = moments(gr)
                assert_equal(cpu(st["m_" + name]), m, what + ": m_" + name, "r, j")
                assert_equal(cpu(st["v_" + name]), v, what + ": v_" + name, "r, j")
            # a zero gradient (masked elements, columns not produced, empty rows) keeps the parameter bit for bit
            loc2, ls2 = cpu(lv.loc), cpu(lv.log_scale)
            assert np.array_equal(loc2[g_mu == 0], L.loc[g_mu == 0]) and np.array_equal(ls2[g_ls == 0], L.ls[g_ls == 0]), what
            assert (loc2 != L.loc).any()
            if L.mask is not None:
                enc = (L.mask == 1) & (L.group_idx == 2)[None, :]
                assert enc.any() and not g_mu[enc].any() and np.array_equal(loc2[enc], L.loc[enc]) and np.array_equal(ls2[enc], L.ls[enc])


# ---- 5. gradient with KL on real inputs, one update ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,li", UPDATE_LEVELS, ids=map(lid, UPDATE_LEVELS))
def test_gradient_with_kl_and_one_update_within_the_bounds(case, li):
    L = level(case, li)
    v = case.levels[li]
    ksd = 0.5
    w = pe.kl_weight(L, 0.37, ksd, use_beta=case.beta)
    g_mu, g_sig, b_mu, b_sig = pe.grads64(L, w, L.sig, L.sp)
    g_ls = g_sig * L.dst.astype(F64)
    b_ls = L.dst.astype(F64) * b_sig + pe.U * np.abs(g_ls)
    s = pe.adam_scalars(2e-4, 1)
    kl64, _ = pe.kl_ref(L.loc, L.sig, L.p_loc[None, :], L.sp[None, :])
    kl_b = pe.kl_bound(L.loc, L.sig, L.p_loc[None, :], L.sp[None, :])
    runs = [(True, True), (True, False)]                         # (adam, want_grads); the second only where it reaches another kernel
    for generic in (False, True):
        for adam, want in runs:
            kern = pe.bwd_reached(case, li, adam, want, generic)
            if not want and kern == pe.bwd_reached(case, li, True, True, generic):
                continue
            what = "%s level %d, %s" % (case.name, li, kern)
            with dispatch(generic):
                lv = spec(L)
                st = zero_state(lv)
                slots = torch.zeros(1024, device=DEV, dtype=torch.int64)
                out = ops.posterior_bwd(lv, g(L.p_loc), g(L.p_ls), True, 0.37, g(L.d_out), g(L.eps), L.S, adam=ops.adam_cfg(2e-4, 1),
                                        state=st, want_grads=want, kl_accum=slots, kl_scalar_dev=torch.tensor([ksd], device=DEV),
                                        **update_args(L, case))
            for name, gr64, bnd, p0 in (("loc", g_mu, b_mu, L.loc), ("ls", g_ls, b_ls, L.ls)):
                m, vv = cpu(st["m_" + name]), cpu(st["v_" + name])
                if want:
                    gd = cpu(out[0 if name == "loc" else 1])
                    assert_within(gd, gr64, bnd, what + ": g_" + name, "g_%s / bound" % name)
                    print("BITEQUAL %s g_%s: %.4f" % (what, name, float(np.mean(gd == pe.f32(gr64)))))
                    assert_equal(m, pe.f32(s.w1 * gd), what + ": m_" + name, "r, j")
                    assert_equal(vv, pe.f32(pe.f32(s.w2 * gd) * gd), what + ": v_" + name, "r, j")
                else:
                    w1, w2 = float(s.w1), float(s.w2)
                    assert_within(m, w1 * gr64, w1 * bnd + pe.U * np.abs(m), what + ": m_" + name, "m_%s / bound (no g out)" % name)
                    assert_within(vv, w2 * gr64 ** 2, w2 * (2 * np.abs(gr64) * bnd + bnd ** 2) + 2 * pe.U * np.abs(vv), what + ": v_" + name)
                # the parameter: the fp64 step from the kernel's own m and v (checked above), as pe.adam forms it
                denom = np.sqrt(vv.astype(F64)) / float(s.bc2_sqrt) + float(s.eps)
                stepv = float(s.step_size) * m.astype(F64) / denom
                p64 = p0.astype(F64) - stepv
                bound = 0.5 * pe.ulp(np.abs(p64) + pe.ADAM_C * 2.0 ** -23 * np.abs(stepv)) + pe.ADAM_C * 2.0 ** -23 * np.abs(stepv)
                got = cpu(lv.loc if name == "loc" else lv.log_scale)
                assert_within(got, p64, bound, what + ": updated " + name, "updated parameter / bound")
                keep = (m == 0) & (vv == 0)
                assert np.array_equal(got[keep], p0[keep])
            if L.mask is not None and case.beta:                    # masked elements of the zero-beta group keep their bits
                enc = (L.mask == 1) & (L.group_idx == 2)[None, :]
                assert enc.any() and np.array_equal(cpu(lv.loc)[enc], L.loc[enc]) and np.array_equal(cpu(lv.log_scale)[enc], L.ls[enc])
            # 7c. the KL log: the KL BEFORE the update, one partial sum rounded to 2^-24 nats per workgroup
            sl = cpu(slots)
            assert sl[-1] == 0
            kl_got = float(sl[:-1].sum()) / ops.KL_FX
            lim = kl_b.sum() + pe.kl_workgroups(kern, v) * 2.0 ** -25 + kl64.size * 2.0 ** -53 * np.abs(kl64).sum()    # (pe: "KL log")
            assert abs(kl_got - kl64.sum()) <= lim, (what, kl_got, kl64.sum(), lim)
            note("KL log / bound", abs(kl_got - kl64.sum()) / lim)


# ---- 6. Adam alone -----------------------------------------------------------------------------------------------------------------------
def _adam_inputs(n, seed):
    r = np.random.RandomState(seed)
    gs = []
    for _ in range(3):
        gr = pe.f32(10.0 ** r.uniform(-15, 2, n) * r.choice([-1.0, 1.0], n))
        gr[np.abs(gr) < 1e-15] = F32(1e-15)
        gr[r.rand(n) < 0.1] = 0
        gr[:16] = 0                                         # never a gradient: p, m, v stay as they are
        gs.append(gr)
    return pe.f32(r.randn(n)), gs


@pytest.mark.parametrize("entry", ["flat", "multi"])
def test_adam_moments_bit_for_bit_and_the_step_within_the_bound(entry):
    sizes = [5000] if entry == "flat" else [1023, 1024, 1025, 1, 1927, 0, 300]
    data = [_adam_inputs(n, 7 + i) for i, n in enumerate(sizes)]
    p = [g(d[0].copy()) for d in data]
    m, v = [torch.zeros_like(t_) for t_ in p], [torch.zeros_like(t_) for t_ in p]
    ref = [(d[0], np.zeros_like(d[0]), np.zeros_like(d[0])) for d in data]
    for step in (1, 2, 3):
        cfg = ops.adam_cfg(2e-4, step)
        grads = [g(d[1][step - 1]) for d in data]
        if entry == "flat":
            ops.adam_flat(p[0], grads[0], m[0], v[0], cfg)
        else:
            ops.adam_multi(p, grads, m, v, cfg)
        s = pe.adam_scalars(2e-4, step)
        for i, d in enumerate(data):
            if not sizes[i]:
                continue
            m2, v2, p64, bound = pe.adam(ref[i][0], d[1][step - 1], ref[i][1], ref[i][2], s)
            what = "adam_%s, tensor %d, step %d" % (entry, i, step)
            assert_equal(cpu(m[i]), m2, what + ": m", "i")
            assert_equal(cpu(v[i]), v2, what + ": v", "i")
            assert_within(cpu(p[i]), p64, bound, what + ": p", "adam p / bound")
            ref[i] = (cpu(p[i]).copy(), m2, v2)
    for i, d in enumerate(data):
        if sizes[i]:
            k = min(16, sizes[i])
            assert np.array_equal(cpu(p[i])[:k], d[0][:k]) and not cpu(m[i])[:k].any() and not cpu(v[i])[:k].any()


# ---- 7. KL sums --------------------------------------------------------------------------------------------------------------------------
def test_kl_group_and_row_sums():
    case = pe.CASE["testtime_l1"]
    L = level(case, 0)
    k = kl_tap(L.loc, L.ls, L.p_loc, L.p_ls, True)                                   # the tapped elements, doubles of floats
    k32 = k.astype(F32)
    assert np.array_equal(k32.astype(F64), k)
    kref, _ = pe.kl_ref(L.loc, L.sig, L.p_loc[None, :], L.sp[None, :])
    kb = pe.kl_bound(L.loc, L.sig, L.p_loc[None, :], L.sp[None, :])
    assert_within(k, kref, kb, "tapped KL elements", "kl_elem_f32 / bound (case data)")
    seg = (L.seg_start, L.seg_end)
    ss, se = g(L.seg_start.astype(np.int32)), g(L.seg_end.astype(np.int32))
    gi = g(L.group_idx.astype(np.int32))
    n = L.cols
    for beta in (None, L.beta):
        rows_ref, groups_ref = pe.kl_rows(k32, beta, L.group_idx, seg)
        rows, groups = ops.gauss_kl(g(L.loc), g(L.ls), g(L.p_loc), g(L.p_ls), True, beta=g(beta), group_idx=gi if beta is not None else None,
                                    seg_start=ss, seg_end=se, want_groups=True)
        assert_equal(cpu(groups), groups_ref, "kl_group", "r, g")
        wts = np.ones_like(groups_ref) if beta is None else beta.astype(F64)
        assert_within(cpu(rows), rows_ref, n * 2.0 ** -53 * (wts * np.abs(groups_ref)).sum(1), "kl_row with segments", "kl_row (segments) / bound")
        # without segments: every fl32(k beta) of the tapped elements, summed in fp64 in the kernel's own order
        rows2_ref, _ = pe.kl_rows(k32, beta, L.group_idx, None)
        terms = np.abs(k32 if beta is None else pe.f32(k32 * beta[:, L.group_idx])).astype(F64)
        rows2, _ = ops.gauss_kl(g(L.loc), g(L.ls), g(L.p_loc), g(L.p_ls), True, beta=g(beta), group_idx=gi if beta is not None else None)
        assert_within(cpu(rows2), rows2_ref, n * 2.0 ** -53 * terms.sum(1), "kl_row without segments", "kl_row (no segments) / bound")


# ---- 8. fixed-point sums -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(300, 517), (1, 7)])
def test_fixed_point_column_sums(rows, cols):
    r = np.random.RandomState(rows)
    loc = pe.f32(0.3 * r.randn(rows, cols))
    ls = pe.f32(-4 + r.randn(rows, cols))
    assert (loc < 0).any()
    sig = st_tap(ls)
    fx = cpu(ops.col_moments_fx(g(loc), g(ls)))
    ref = pe.col_moments_fx(loc, sig)
    assert fx.shape == (6 * cols + 1,) and [int(x) for x in fx] == ref, "col_moments: first differing word %d" % next(
        i for i, (a, b) in enumerate(zip(fx, ref)) if int(a) != b)
    assert ref[-1] == 0
    p_loc, p_ls = pe.f32(0.3 + 0.01 * r.randn(cols)), pe.f32(-3 + 0.2 * r.randn(cols))
    sp = st_tap(p_ls)
    loc = pe.f32(0.3 + 0.02 * r.randn(rows, cols))                   # (near the prior: every KL far below the 2^12 nats that count as bad)
    kfx = cpu(ops.gauss_kl_colsum_fx(g(loc), g(ls), g(p_loc), g(sp), q_is_log=True))
    kref, _ = pe.kl_ref(loc, sig, p_loc[None, :], sp[None, :])
    kb = pe.kl_bound(loc, sig, p_loc[None, :], sp[None, :])
    assert np.abs(kref).max() < 2048
    want = pe.kl_colsum_fx(kref)
    assert kfx[-1] == want[-1] == 0
    assert_within(kfx[:-1].astype(F64), np.array(want[:-1], F64), (2.0 ** 30 * kb + 1).sum(0), "kl_colsum", "kl_colsum / bound")
    # poison: the counts are exactly the number of poisoned terms
    bad_loc, bad_ls = loc.copy(), ls.copy()
    spots = [(0, 1, np.nan), (0, 3, np.inf), (0, 5, 100.0)] if rows == 1 else [(5, 7, np.nan), (200, 3, np.inf), (299, 516, 100.0), (17, 0, -np.inf)]
    for r_, c_, val in spots:
        bad_loc[r_, c_] = val
    bad_ls[0, 2] = np.nan
    fxb = cpu(ops.col_moments_fx(g(bad_loc), g(bad_ls)))
    refb = pe.col_moments_fx(bad_loc, st_tap(bad_ls))
    assert [int(x) for x in fxb] == refb and refb[-1] == 2 * (len(spots) - 1) + 1 + 1
    kb_fx = cpu(ops.gauss_kl_colsum_fx(g(bad_loc), g(ls), g(p_loc), g(sp), q_is_log=True))
    assert int(kb_fx[-1]) == len(spots)                             # (100 - 0.3)^2 / sp^2 / 2 is far beyond 2^12 nats as well
    clean = np.ones(cols, bool)
    clean[[c_ for _, c_, _ in spots]] = False
    assert np.array_equal(kb_fx[:-1][clean], kfx[:-1][clean])


# ---- 9. beta_update ------------------------------------------------------------------------------------------------------------------------
def test_beta_update_equals_the_restatement():
    r = np.random.RandomState(9)
    ln2 = 0.6931471805599453
    kl = r.uniform(5, 16, (64, 37)) * ln2
    for i, thr in enumerate((16.0, 15.6)):
        base = thr * ln2
        kl[3 * i, :3] = [np.nextafter(base, 0), base, np.nextafter(base, 100)]
        kl[3 * i + 1, :3] = [np.nextafter(np.nextafter(base, 0), 0), base, np.nextafter(np.nextafter(base, 100), 100)]
    beta = pe.f32(r.rand(64, 37) * 10)
    beta[:, 5], beta[:, 6], beta[:, 7], beta[:, 8] = 0, 9999.9, 10000.0, 9700.0
    kl[::2, 5:9] = 20 * ln2                           # above: beta *= 1.05 -> clamped at 1e4
    kl[1::2, 5:9] = 3 * ln2                           # below: beta /= 1.05
    done = (r.rand(64, 37) < 0.2).astype(np.uint8)
    b = g(beta.copy())
    ops.beta_update(g(kl), b, g(done))
    ref = pe.beta_update(kl, beta, done)
    assert_equal(cpu(b), ref, "beta_update", "r, g")
    assert (ref == 10000).any() and (ref == 0).any() and (ref > beta).any() and (ref < beta).any() and (ref[done == 1] == beta[done == 1]).all()
    b2 = g(beta.copy())
    ops.beta_update(g(kl), b2, None)
    assert_equal(cpu(b2), pe.beta_update(kl, beta, np.zeros_like(done)), "beta_update without done", "r, g")


# ---- 10. Philox ----------------------------------------------------------------------------------------------------------------------------
def _philox_check(n, seed, stream, step, goff, what, dev_step=False):
    st = torch.tensor([step], device=DEV, dtype=torch.int64) if dev_step else step
    got = cpu(ops.philox_normal(n, seed, stream, st, group_offset=goff))
    ref, one = pe.philox_normal_ref(n, seed, stream, step, goff)
    err = np.abs(got.astype(F64) - ref)
    print("PHILOX %s: worst |got - ref| = %.3e at |ref| = %.3f" % (what, err.max(), abs(ref[err.argmax()])))
    assert got.shape == (n,) and np.all(got[one] == 0)
    assert err.max() <= PHILOX_LIMIT <= 1e-5, "%s: element %d: got %r, expected %r" % (what, err.argmax(), got[err.argmax()], ref[err.argmax()])
    return got


def test_noise_is_philox4x32_10_with_the_documented_counter():
    seed = 0x1234_5678_9ABC_DEF0
    _philox_check(1 << 22, 1234, 0, 7, 0, "2^22 draws")
    _philox_check(1003, seed, 3, 7, 0, "n = 1003, both seed halves")
    _philox_check(16, seed, 3, 7, 2 ** 32 - 2, "group offset 2^32 - 2")
    a = _philox_check(4099, seed, 3, 2 ** 32 + 7, 5, "step 2^32 + 7 from the host")
    b = _philox_check(4099, seed, 3, 2 ** 32 + 7, 5, "step 2^32 + 7 from the device", dev_step=True)
    assert np.array_equal(a, b)
    c = cpu(ops.philox_normal(4099, seed, 3, 7, group_offset=5))
    assert not np.array_equal(a, c)                                          # the high step word counts


def test_fused_samplers_draw_that_noise():
    seed, goff = 0x1234_5678_9ABC_DEF0, 2 ** 32 - 2
    step = torch.tensor([2 ** 32 + 7], device=DEV, dtype=torch.int64)
    case = pe.CASE["hier3"]
    L = [level(case, li) for li in range(3)]
    lv0 = LevelSpec(g(L[0].loc), g(L[0].ls), L[0].cols, L[0].rows)
    n = L[0].rows * L[0].cols
    out, eps = ops.reparam_rng(lv0, seed, 3, step, group_offset=goff)
    want = ops.philox_normal(n, seed, 3, step, group_offset=goff)
    assert torch.equal(eps.view(-1), want)
    L0 = pe.SimpleNamespace(**vars(L[0]))
    L0.eps = cpu(want).reshape(L[0].rows, 1, L[0].cols)
    assert_equal(cpu(out), pe.sample([L0]), "reparam_rng", "n, s, d")
    specs = [spec(v) for v in L]
    eps_out = [torch.empty(case.n, 1, pe.D, device=DEV) for _ in L]
    out3 = ops.reparam_hier_rng(specs, eps_out, seed, (0, 2, 3), step, group_offset=goff)
    Ls = []
    for v, e, stream in zip(L, eps_out, (0, 2, 3)):
        assert torch.equal(e.view(-1), ops.philox_normal(n, seed, stream, step, group_offset=goff))
        c = pe.SimpleNamespace(**vars(v))
        c.eps = cpu(e)
        Ls.append(c)
    assert_equal(cpu(out3), pe.sample(Ls), "reparam_hier_rng", "n, s, d")
