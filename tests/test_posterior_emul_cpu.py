"""CPU tests of the evaluator of the posterior path (tests/posterior_emul.py): the premises of test_hip_posterior_exact.py.

  philox      Philox4x32-10 known answers; the counter layout; u1 = 1 gives a normal of exactly 0.
  bounds      ST_ULPS / DST_ULPS cover st_ulp_bound / dst_ulp_bound over a dense grid and every float next to the series / log switch.
  definition  sampler and gradients against oracle.ref_cpu (sample_latent_weights, Level.effective) and torch.autograd in fp64 on
              every layout case of the GPU suite; Adam against torch.optim.Adam; KL against torch.distributions; group KLs and
              beta_update against the goldens of tests/golden/test_cifar.npz; the fixed-point sums against exact rationals.
  inverses    ops.LevelSpec's host-built member lists and inverse maps against the forward maps, on every case.
  lattice     for every lattice case: sum |term| / grid < 2^24, so every fp32 partial sum is exact and the chain equals fp64.
  mutants     eight deliberately wrong variants of the evaluator each differ from it on the committed cases: the cases can see these
              errors.  (Evaluator against evaluator, on the CPU: nothing here is injected into a kernel.)
  dispatch    the arithmetic of each case's dispatch condition, so that the cases reach the kernels they name."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import posterior_emul as pe
from golden_util import O, load, t

from recombiner_amd.ops import LevelSpec

F32, F64 = np.float32, np.float64
UPDATE_LEVELS = [(c, li) for c in pe.CASES if c.update for li in range(len(c.levels))]
lid = lambda p: "%s-L%d" % (p[0].name, p[1])          # noqa: E731


def _level(case, li, lattice=False):
    L = pe.level_data(case, li, lattice, O.column_row_perms)
    L.sig = pe.f32(pe.st_ref(L.ls))                   # stand-ins for the device taps: the correctly rounded values
    L.dst = pe.f32(pe.dst_ref(L.ls))
    L.sp = pe.f32(pe.st_ref(L.p_ls))
    return L


# ---- philox -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(ctr, key, out):
    got = pe.philox4x32_10(ctr, key)
    assert " ".join("%08x" % int(v[0]) for v in got) == out


def test_philox_counter_layout_and_normals():
    groups = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5], np.uint64)
    ctr, key = pe.philox_counter(groups, 0x1234_5678_9ABC_DEF0, 3, 2 ** 32 + 7)
    assert [int(v) for v in ctr[0]] == [0, 1, 2 ** 32 - 1, 0, 5] and [int(v) for v in ctr[1]] == [0, 0, 0, 1, 256]
    assert int(ctr[2][0]) == 3 ^ 0x85EBCA6B and int(ctr[3][0]) == 7 and key == [0x9ABCDEF0, 0x12345678]
    e, one = pe.philox_normal_ref(1 << 20, 1234, 0, 7)
    assert abs(e.mean()) < 5e-3 and abs(e.var() - 1) < 1e-2 and np.all(e[one] == 0)
    assert np.array_equal(pe.philox_normal_ref(1003, 1234, 0, 7)[0], e[:1003])
    assert np.array_equal(pe.philox_normal_ref(16, 1234, 0, 7, group_offset=5)[0], e[20:36])
    # u1 = 1: (float)(2^24 - 1) + 0.5f rounds to 2^24
    assert (F32(2 ** 24 - 1) + F32(0.5)) * F32(1 / 16777216.0) == 1.0 and np.sqrt(-2 * np.log(1.0)) == 0


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
def _floats_between(lo, hi):
    a, b = np.array([lo, hi], F32).view(np.int32)
    return np.arange(min(a, b), max(a, b) + 1, dtype=np.int32).view(F32)


def test_ulp_constants_cover_the_counted_bounds():
    x = np.concatenate([np.linspace(-80, 20, 400001), np.linspace(20, 88.7, 1001), _floats_between(-4.17, -4.15).astype(F64)])
    b = pe.st_ulp_bound(x)
    assert np.isfinite(b).all() and b.max() <= pe.ST_ULPS <= 8, (b.max(), x[b.argmax()])
    x = np.concatenate([np.linspace(-80, 80, 400001), _floats_between(-4.17, -4.15).astype(F64)])
    b = pe.dst_ulp_bound(x)
    assert np.isfinite(b).all() and b.max() <= pe.DST_ULPS <= 8, (b.max(), x[b.argmax()])
    assert abs(np.log(2.0 ** -6) - (-4.1589)) < 1e-4                        # the switch t = 2^-6 sits inside the swept interval


# ---- definition: sampler and gradients ------------------------------------------------------------------------------------------------
def _torch_level(L, dtype=torch.float64):
    """oracle.ref_cpu.Level of one case level (group-order storage: col_map is its group_to_param)"""
    tt = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)          # noqa: E731
    lv = O.Level(tt(L.loc).requires_grad_(True), tt(L.ls).requires_grad_(True), tt(L.p_loc), tt(L.p_ls), L.group_idx, L.seg_start,
                 L.seg_end, L.col_map if L.col_map is not None else np.arange(L.cols_out), len(L.seg_start), tt(L.beta),
                 row_perm_g2p=L.row_perm)
    if L.mask is not None:
        lv.mask, lv.sample = tt(L.mask), tt(L.z)
    return lv


def _torch_sample(levels, tls):
    out = 0
    for L, lv in zip(levels, tls):
        mu, sig = lv.effective()
        if L.scale_is_sigma:
            sig = lv.log_scale[:, :L.cols_out]
        rm = torch.from_numpy(L.row_map if L.row_map is not None else np.arange(L.n))
        v = mu[rm][:, None, :] + sig[rm][:, None, :] * torch.from_numpy(L.eps).double()
        out = v if isinstance(out, int) else out + torch.nn.functional.pad(v, (0, out.shape[-1] - v.shape[-1]))
    return out


@pytest.mark.parametrize("case", pe.CASES, ids=pe.case_id)
def test_sampler_is_the_reference_sampler(case):
    levels = [_level(case, li) for li in range(len(case.levels))]
    tls = [_torch_level(L) for L in levels]
    ref = _torch_sample(levels, tls).detach().numpy()
    got = pe.sample(levels)
    mag = _torch_sample([_abs(L) for L in levels], [_torch_level(_abs(L)) for L in levels]).detach().numpy()
    assert got.dtype == F32 and got.shape == (case.n, case.S, case.levels[0].cols_out)
    assert np.all(np.abs(got - ref) <= 8 * pe.U * mag + 1e-30)


def _abs(L):
    A = pe.SimpleNamespace(**vars(L))
    A.loc, A.eps = np.abs(L.loc), np.abs(L.eps)
    if L.z is not None:
        A.z = np.abs(L.z)
    return A


class _Geo:
    """what oracle.ref_cpu.sample_latent_weights reads of a Geometry"""
    patch = True

    def __init__(self, maps):
        self.maps = maps

    def level_maps(self, n):
        return tuple(torch.from_numpy(m) for m in self.maps)


@pytest.mark.parametrize("name", ["hier3", "hier3_n42"])
def test_plain_hierarchy_is_sample_latent_weights(name):
    case = pe.CASE[name]
    L = [_level(case, li) for li in range(3)]
    d = lambda a: torch.from_numpy(a).double()          # noqa: E731
    noise = O.Noise(replay=[d(v.eps) for v in L])
    ref = O.sample_latent_weights(_Geo([L[1].row_map, L[2].row_map]), d(L[0].loc), O.st(d(L[0].ls)), d(L[1].loc), O.st(d(L[1].ls)),
                                  d(L[2].loc), O.st(d(L[2].ls)), case.S, noise).numpy()
    assert np.abs(pe.sample(L) - ref).max() < 1e-6 * np.abs(ref).max()


@pytest.mark.parametrize("case,li", UPDATE_LEVELS, ids=map(lid, UPDATE_LEVELS))
def test_gradients_are_autograd_of_the_reference(case, li):
    L = _level(case, li)
    lv = _torch_level(L)
    d_out = torch.from_numpy(L.d_out).double()
    w = pe.kl_weight(L, 0.37, 0.5, use_beta=case.beta)
    loss = (_torch_sample([L], [lv]) * d_out).sum() + (torch.from_numpy(w).double() * lv.kl_elem()).sum()
    loss.backward()
    sig64, sp64 = pe.st_ref(L.ls), pe.st_ref(L.p_ls)
    g_mu, g_sig, b_mu, b_sig = pe.grads64(L, w, sig64, sp64)
    np.testing.assert_allclose(g_mu, lv.loc.grad.numpy(), rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(g_sig * pe.dst_ref(L.ls), lv.log_scale.grad.numpy(), rtol=1e-9, atol=1e-14)
    # the fp32 chain of the gather sits inside the derived bound around fp64
    a32, b32 = pe.gather32(L)
    a64, b64 = pe.gather64(L)
    assert np.all(np.abs(a32 - a64) <= b_mu) and np.all(np.abs(b32 - b64) <= b_sig)
    if case.beta:
        assert (L.beta == 0).any() and (w == 0).any()


# ---- inverses -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,li", UPDATE_LEVELS, ids=map(lid, UPDATE_LEVELS))
def test_level_spec_inverses_invert_the_forward_maps(case, li):
    L = _level(case, li)
    spec = LevelSpec(torch.from_numpy(L.loc), torch.from_numpy(L.ls), L.cols_out, L.n, row_map=L.row_map, row_perm=L.row_perm,
                     col_map=L.col_map)
    if L.row_map is not None:
        ptr, idx = spec.member_ptr.numpy(), spec.member_idx.numpy()
        assert ptr[0] == 0 and ptr[-1] == L.n and len(ptr) == L.rows + 1
        for r in range(L.rows):
            assert idx[ptr[r]:ptr[r + 1]].tolist() == np.flatnonzero(L.row_map == r).tolist()       # ascending INR index
    if L.row_perm is not None:
        inv = spec.row_perm_inv.numpy()
        cols = np.arange(L.cols)[None, :]
        assert np.array_equal(inv[L.row_perm, cols], np.broadcast_to(np.arange(L.rows)[:, None], inv.shape))
    if L.col_map is not None:
        inv = spec.col_inv.numpy()
        assert np.array_equal(inv[L.col_map], np.arange(L.cols_out))
        assert np.all(np.delete(inv, L.col_map) >= L.cols_out) and len(set(L.col_map.tolist())) == L.cols_out


# ---- definition: Adam, KL, annealing, fixed point ---------------------------------------------------------------------------------------
def test_adam_is_torch_adam():
    r = np.random.RandomState(4)
    p0 = r.randn(1000)
    ref = torch.from_numpy(p0.astype(F32).astype(F64)).requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=float(F32(2e-4)), betas=(float(F32(0.9)), float(F32(0.999))), eps=float(F32(1e-8)))
    p, m, v = pe.f32(p0), np.zeros(1000, F32), np.zeros(1000, F32)
    for step in (1, 2, 3):
        g = pe.f32(r.randn(1000) * 10.0 ** r.randint(-6, 2, 1000))
        ref.grad = torch.from_numpy(g.astype(F64))
        opt.step()
        m, v, p64, bound = pe.adam(p, g, m, v, pe.adam_scalars(2e-4, step))
        p = pe.f32(p64)
        assert np.all(bound >= 0.5 * pe.ulp(p64))
    np.testing.assert_allclose(p, ref.detach().numpy(), rtol=2e-6, atol=1e-9)
    s = pe.adam_scalars(2e-4, 1)
    assert s.w1 == F32(1 - float(F32(0.9))) and s.step_size == F32(float(F32(2e-4)) / (1 - float(F32(0.9))))
    m2, v2, p2, _ = pe.adam(p, np.zeros(1000, F32), np.zeros(1000, F32), np.zeros(1000, F32), s)
    assert np.array_equal(p2, p.astype(F64)) and not m2.any() and not v2.any()


def test_kl_sums_and_annealing_match_the_goldens():
    d = load("test_cifar.npz")
    loc, ls, pl, pls = t(d, "t_loc"), t(d, "t_log_scale"), t(d, "kw_p_loc"), t(d, "kw_p_log_scale")
    k32 = O.gauss_kl_elem(loc, O.st(ls), pl[None, :], O.st(pls)[None, :]).numpy()
    k64, _ = pe.kl_ref(loc.numpy(), O.st(ls).numpy(), pl.numpy()[None, :], O.st(pls).numpy()[None, :])
    ref64 = O.gauss_kl_elem(loc.double(), O.st(ls).double(), pl.double()[None, :], O.st(pls).double()[None, :]).numpy()
    np.testing.assert_allclose(k64, ref64, rtol=1e-12, atol=1e-15)
    seg = (d["G_start"].astype(np.int64), d["G_end"].astype(np.int64))
    rows, groups = pe.kl_rows(k32, seg=seg)
    np.testing.assert_array_equal(groups, d["kls"])
    beta = d["beta_before"].astype(F32)
    rows_b, _ = pe.kl_rows(k32, beta, d["G_group_idx"].astype(np.int64), seg)
    np.testing.assert_allclose(rows_b.sum(), float(d["kl_beta_weighted"]), rtol=2e-6)
    np.testing.assert_array_equal(pe.beta_update(d["kls"], beta, np.zeros_like(beta, bool)), d["beta_after"])
    done = np.zeros_like(beta, bool)
    done[0, 3] = True
    assert pe.beta_update(d["kls"], beta, done)[0, 3] == beta[0, 3]


def test_fixed_point_sums_are_exact():
    r = np.random.RandomState(8)
    loc, sig = pe.f32(0.3 - 0.4 * r.rand(9, 5) + 0.02 * r.randn(9, 5)), pe.f32(0.003 + 0.002 * r.rand(9, 5))
    loc[2, 1], loc[3, 1] = 100.0, np.nan
    loc[:, 0] = -np.abs(loc[:, 0])
    fx = pe.col_moments_fx(loc, sig)
    assert len(fx) == 31 and fx[30] == 3                    # 100^2, nan, nan^2
    s2 = pe.f32(sig * sig)
    for j in (0, 2, 4):
        for q, term in enumerate((lambda x: Fraction(x), lambda x: Fraction(x) ** 2)):
            exact = sum(term(float(x)) for x in loc[:, j])
            got = Fraction(fx[2 * q * 5 + j], 2 ** 30) + Fraction(fx[(2 * q + 1) * 5 + j], 2 ** 62)
            assert abs(got - exact) <= Fraction(9, 2 ** 63)
        assert Fraction(fx[4 * 5 + j], 2 ** 30) + Fraction(fx[5 * 5 + j], 2 ** 62) == sum(Fraction(float(x)) for x in s2[:, j])
    assert fx[0] < 0 and 0 <= fx[5] < 9 * 2 ** 32            # the floor branch: hi below, lo in [0, 1)
    k = np.array([[0.5, 1e-9], [4096.0, np.inf], [0.25 + 2.0 ** -31, 3.0]])
    assert pe.kl_colsum_fx(k) == [2 ** 29 + 2 ** 28, round(1e-9 * 2 ** 30) + 3 * 2 ** 30, 2]


# ---- lattice ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,li", UPDATE_LEVELS, ids=map(lid, UPDATE_LEVELS))
def test_lattice_partial_sums_are_exact(case, li):
    L = _level(case, li, lattice=True)
    h_mu, h_sig = pe.lattice_headroom(L)
    assert 0 < h_mu < 2 ** 24 and 0 < h_sig < 2 ** 24
    assert np.all(L.d_out * 2.0 ** 10 == np.rint(L.d_out * 2.0 ** 10)) and np.abs(L.eps * 2.0 ** 6).max() <= 255
    a32, b32 = pe.gather32(L)
    a64, b64 = pe.gather64(L)
    assert np.array_equal(a32.astype(F64), a64) and np.array_equal(b32.astype(F64), b64)
    a_rev, b_rev = pe.gather32(L, mutant="members_reversed")                 # exact sums: any order
    assert np.array_equal(a_rev, a32) and np.array_equal(b_rev, b32)


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return not all(np.array_equal(x, y) for x, y in zip(a, b))


def test_every_mutant_differs_from_the_evaluator():
    seen = {}
    for case, li in UPDATE_LEVELS:
        for lattice in (True, False):
            L = _level(case, li, lattice)
            base = pe.gather32(L)
            for mut in ("mask_early", "row_perm_not_inverted", "col_map_truncated") + (() if lattice else ("members_reversed",)):
                applies = {"mask_early": L.mask is not None and L.S * (1 if L.row_map is None else 2) > 1,
                           "row_perm_not_inverted": L.row_perm is not None, "col_map_truncated": L.col_map is not None and L.cols_out < L.cols,
                           "members_reversed": L.row_map is not None and max(L.spec.counts) > 2}[mut]
                if applies:
                    assert _differs(pe.gather32(L, mutant=mut), base), (case.name, li, mut, lattice)
                    seen[mut] = seen.get(mut, 0) + 1
        if case.beta and case.levels[li].col_map:
            L = _level(case, li)
            assert _differs([pe.kl_weight(L, 1.0, None, True, mutant="beta_at_d")], [pe.kl_weight(L, 1.0, None, True)]), case.name
            seen["beta_at_d"] = seen.get("beta_at_d", 0) + 1
    for case in pe.CASES:
        if any(v.cols_out < case.levels[0].cols_out for v in case.levels):
            levels = [_level(case, li) for li in range(len(case.levels))]
            assert _differs([pe.sample(levels, mutant="beyond_cols_out")], [pe.sample(levels)])
            seen["beyond_cols_out"] = seen.get("beyond_cols_out", 0) + 1
    base = pe.philox_normal_ref(64, 0x1234_5678_9ABC_DEF0, 3, 2 ** 32 + 7, group_offset=2 ** 32 - 2)[0]
    for mut in ("swap_stream_step", "drop_group_hi"):
        got = pe.philox_normal_ref(64, 0x1234_5678_9ABC_DEF0, 3, 2 ** 32 + 7, group_offset=2 ** 32 - 2, mutant=mut)[0]
        assert _differs([got], [base])
        seen[mut] = 1
    # the high group word matters from the third group of that launch on, and only there
    got = pe.philox_normal_ref(16, 1, 0, 7, group_offset=2 ** 32 - 2, mutant="drop_group_hi")[0]
    ref = pe.philox_normal_ref(16, 1, 0, 7, group_offset=2 ** 32 - 2)[0]
    assert np.array_equal(got[:8], ref[:8]) and not np.array_equal(got[8:], ref[8:])
    assert set(seen) == {"mask_early", "beta_at_d", "row_perm_not_inverted", "col_map_truncated", "members_reversed", "beyond_cols_out",
                         "swap_stream_step", "drop_group_hi"}, seen


# ---- dispatch --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pe.CASES, ids=pe.case_id)
def test_cases_reach_the_kernels_they_name(case):
    assert pe.fwd_reached(case) == case.fwd == pe.kernel_reached(case)["fwd"]
    assert all(b == v.bwd for b, v in zip(pe.kernel_reached(case)["bwd"], case.levels) if v.bwd)
    assert pe.fwd_reached(case, generic=True) == "reparam_fwd"
    for li, v in enumerate(case.levels):
        if v.bwd:
            assert (pe.bwd_reached(case, li, True, False), pe.bwd_reached(case, li, False, True)) == v.bwd
            assert pe.bwd_reached(case, li, True, False, generic=True) == pe.GEN
        assert v.cols_out <= v.cols and (v.counts is None or (sum(v.counts) == case.n and len(v.counts) == v.rows))
    assert case.levels[0].cols_out == max(v.cols_out for v in case.levels)


def test_dispatch_arithmetic_of_the_thresholds():
    C = pe.CASE
    assert 5 * 3840 * 8 == pe.LDS_LIMIT and 5 * 3841 * 8 > pe.LDS_LIMIT            # posterior_staged: exactly at the limit, and past it
    assert 9600 * 16 == pe.LDS_LIMIT and 9601 * 16 > pe.LDS_LIMIT                  # reparam_staged
    assert (4 * pe.D) % 4 == 0 and (5 * pe.D) % 4 != 0 and (44 * pe.D) % 4 == 0 and (42 * pe.D) % 4 != 0
    assert 512 * pe.cdiv(pe.D, 1024) == 1024 and 6 * pe.cdiv(pe.D, 1024) < 1024     # members4<256> from 1024 workgroups on
    assert pe.D == 4 * 257 + 1 and pe.D % 4 == 1 and pe.cdiv(pe.D, 1024) == 2
    # the second members4<256> workgroup of a row: lanes with 4, 1 and 0 valid columns
    nv = [max(0, min(4, pe.D - 4 * (256 + lane))) for lane in range(256)]
    assert nv[0] == 4 and nv[1] == 1 and nv[2] == 0
    assert sorted(pe.COUNTS42) == [0, 1, 7, 8, 9, 17] and sum(pe.COUNTS42) == 42 and sum(pe.COUNTS44) == 44
    rm = pe.row_map_of(pe.COUNTS42, ("members42", 0))
    assert (np.diff(rm) < 0).any() and np.bincount(rm, minlength=6).tolist() == list(pe.COUNTS42)
    gi, s, e = pe.groups_of(pe.D, ("x", 0))
    assert len(s) == 37 and e[0] - s[0] == 1 and len(set((e - s).tolist())) > 5 and np.all(np.diff(gi) >= 0) and e[-1] == pe.D
    assert C["testtime_l1"].n * C["testtime_l1"].S >= 8 > C["testtime_l1_s1"].n * C["testtime_l1_s1"].S
    reached = {pe.fwd_reached(c) for c in pe.CASES} | {k for c in pe.CASES for v in c.levels for k in v.bwd}
    assert reached == {"reparam_flat", "reparam_staged", "reparam_hier_flat", "reparam_fwd+packed", "reparam_fwd", pe.GEN, pe.BYD,
                       pe.SUMS, pe.M64, pe.M256, pe.FLAT, pe.STG}
