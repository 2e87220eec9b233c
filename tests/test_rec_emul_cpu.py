"""CPU tests of the evaluator of the A* scorers (tests/rec_emul.py): the premises of test_hip_rec_exact.py.

  oracle       exact_scores with host logs equals oracle.ref_cpu.rec_score's log_w BIT FOR BIT for group lengths 1 to 4 (the
               golden Sobol table of g = 3 and random jobs).  From g = 5 on the reference's `.sum(-1)` is torch's vectorised
               reduction (four accumulators at stride 4 for g = 8 and 12, another order again for g = 5 and 7), not the ascending
               sum of rec_exact_kernel: there (the golden Sobol table of g = 5, random jobs of g = 7, 12, 33) the per-element
               log-densities equal torch's Normal.log_prob bit for bit, the log-weights agree within the (g - 1) roundings of
               either sum order, and the arg-max is the same.
  certificate  on the adversarial families of rec_emul.FAMILIES x g in {1, 2, 3, 7, 12, 33, 70}, for every job
               max_k |exact - true| + max_k |fast - true| <= tau / 2 -- the premise under which a fast gap above tau proves the
               exact arg-max -- and the two one-sided bounds of the kernel's comment, (g + 12) u (S + G) and (2 g + 16) u (S + G).
               Worst ratios (printed by the test; all bounds hold with room):

                   family                      sum / (tau / 2)   exact / its bound   fast / its bound
                   ratio 0.03                  0.028             0.103               0.046
                   ratio 0.2                   0.022             0.053               0.038
                   ratio 1                     0.013             0.040               0.017
                   large means                 0.026             0.081               0.035
                   posterior = prior +- ulp    0.009             0.027               0.012
                   xi at the clamp             0.031             0.068               0.058

  near-ties    the 64 tuned jobs of rec_emul.arbiter_call: every fast gap is <= tau, the two evaluation orders disagree on the
               arg-max in 27 of 64 (>= 16 required) and the exact order takes the higher index of the pair in 24 (>= 8 required
               by the GPU test), every other job of a call has a top-2 gap above 1e-6 g.
  mutants      an always-certify decision rule (tau = -inf, so that an exact tie of the fast scores is certified too) returns a
               wrong index on that family in 27 of 64; a last-of-equals arg-max fails every tie
               placement; a NaN counts as largest."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch
from torch.distributions import Normal

import rec_emul as re_
from golden_util import GOLDEN, O


def _oracle(c_args, xi, gum):
    loc, scale, pl, ps = (torch.from_numpy(re_.f32(v)) for v in c_args)
    return O.rec_score(torch.from_numpy(xi), loc, scale, pl, ps, torch.from_numpy(gum))


def _jobs(seed, g, n):
    loc, scale, pl, ps, jr, js, _ = re_.random_problem(seed, 8, 100, [g], n, (0.03, 0.3, 1.0)[seed % 3])
    return [(loc[r, s:s + g], scale[r, s:s + g], pl[s:s + g], ps[s:s + g]) for r, s in zip(jr, js)]


def _sobol(g):
    return np.load(os.path.join(GOLDEN, "tables", "sobol_normal_g%d_seed42_f32.npy" % g)).astype(np.float64)


@pytest.mark.parametrize("g,golden", [(3, True), (1, False), (2, False), (3, False), (4, False)])
def test_exact_scores_equal_the_oracle_bit_for_bit(g, golden):
    xi = _sobol(g) if golden else re_.normal_table(g, 777, g, clamp=4)
    gum = O.gumbel_table(42) if golden else re_.gumbel_table(g, 777)
    for args in _jobs(10 + g, g, 6):
        mine = re_.exact_scores(re_.constants(*args), xi, gum)
        i, _, lw = _oracle(args, xi, gum)
        assert np.array_equal(mine, lw.numpy())
        assert re_.argmax_first(mine) == i


@pytest.mark.parametrize("g,golden", [(5, True), (7, False), (12, False), (33, False)])
def test_exact_terms_equal_the_oracle_where_its_sum_order_is_torchs(g, golden):
    xi = _sobol(g) if golden else re_.normal_table(g, 777, g, clamp=4)
    gum = O.gumbel_table(42) if golden else re_.gumbel_table(g, 777)
    for args in _jobs(10 + g, g, 4):
        c = re_.constants(*args)
        tq, tp = re_.exact_terms(c, xi)
        loc, scale, pl, ps = (torch.from_numpy(re_.f32(v)) for v in args)
        z = pl + ps * torch.from_numpy(xi)
        assert np.array_equal(tq, Normal(loc, scale).log_prob(z).numpy())
        assert np.array_equal(tp, Normal(pl, ps).log_prob(z).numpy())
        mine = re_.exact_scores(c, xi, gum)
        i, _, lw = _oracle(args, xi, gum)
        # two sums of g terms in either order: (g - 1) roundings each, every partial sum below sum |terms|
        bound = 2 * (g - 1) * 2.0 ** -53 * (np.abs(tq).sum(1) + np.abs(tp).sum(1)) + 2.0 ** -52 * np.abs(lw.numpy())
        assert (np.abs(mine - lw.numpy()) <= bound).all()
        assert re_.argmax_first(mine) == i


def _err(scores, true):
    return max(abs(float(Fraction(float(v)) - t)) for v, t in zip(scores, true))


@pytest.mark.parametrize("family", re_.FAMILIES)
def test_certificate_premise_on_adversarial_families(family):
    worst = np.zeros(3)
    for g in re_.FAMILY_LENS:
        c, xi, gum, X, G = re_.family_job(family, g)
        tau, SG = re_.tau(c, X, G)
        true = re_.true_scores(c, xi, gum)
        e_exact = _err(re_.exact_scores(c, xi, gum), true)
        e_fast = _err(re_.fast_scores(c, xi, gum, X), true)
        r = np.array([(e_exact + e_fast) / (tau / 2), e_exact / ((g + 12) * re_.U * SG), e_fast / ((2 * g + 16) * re_.U * SG)])
        worst = np.maximum(worst, r)
        assert e_exact + e_fast <= tau / 2, (family, g, r)
        assert e_exact <= (g + 12) * re_.U * SG, (family, g, r)
        assert e_fast <= (2 * g + 16) * re_.U * SG, (family, g, r)
    print("RATIO %-26s sum / (tau / 2) %.3f   exact / bound %.3f   fast / bound %.3f" % ((family,) + tuple(worst)))


def test_tau_is_the_kernels_formula():
    c, xi, gum, X, G = re_.family_job("ratio 0.2", 70)
    tau, SG = re_.tau(c, X, G)
    assert tau == 4.0 * (3.0 * 70 + 28.0) * 2.0 ** -53 * SG
    # 70 elements: lanes 0 .. 5 of the strided per-lane sum hold two terms each
    _, _, _, S = re_.fast_coefs(c, X)
    assert SG == S + G and S > 0


def _pick(fa, a, k2):
    return a if (fa[0] > fa[1] or (fa[0] == fa[1] and a < k2)) else k2


def test_near_tie_family_is_not_vacuous_and_needs_the_arbiter():
    tabs = re_.arbiter_tables()
    differ = higher = wrong_if_always_certified = 0
    for n in range(64):
        call, slot, (a, k2) = re_.arbiter_call(n, tables=tabs)
        exact = call.exact(slot)
        fa = call.fast(slot, cand=[a, k2])
        tau = call.tau(slot)
        # a and k2 are far above the rest, in the exact order and so (|fast - exact| <= tau / 4) in the fast order too
        assert np.delete(exact, [a, k2]).max() < min(exact[a], exact[k2]) - 7.0
        assert abs(fa[0] - fa[1]) <= tau, (n, fa, tau)
        fast_full = np.full(call.K, -np.inf)
        fast_full[[a, k2]] = fa
        i_exact = re_.argmax_first(exact)
        idx, unc = re_.decide(fast_full, exact, tau)
        assert (idx, unc) == (i_exact, 1)
        always = re_.decide(fast_full, exact, -np.inf)[0]        # the mutant: every job certified
        assert always == _pick(fa, a, k2)
        wrong_if_always_certified += always != i_exact
        differ += _pick(fa, a, k2) != i_exact
        higher += i_exact == max(a, k2)
        for b in range(call.n):
            if b != slot:
                v1, v2, _ = re_.top2(call.exact(b))
                assert v1 - v2 > 1e-6 * call.jg[b], (n, b)
    print("near-ties: fast arg-max != exact arg-max in %d of 64, exact took the higher index in %d" % (differ, higher))
    assert differ >= 16 and higher >= 8 and wrong_if_always_certified >= 16


def test_argmax_rules_and_tie_placements():
    assert re_.argmax_first([1.0, 3.0, 3.0, 2.0]) == 1 and re_.argmax_last([1.0, 3.0, 3.0, 2.0]) == 2
    assert re_.argmax_first([1.0, np.nan, 5.0, np.nan]) == 1
    assert re_.argmax_first(np.array([1.0, np.nan, 5.0])) == int(torch.argmax(torch.tensor([1.0, float("nan"), 5.0])))
    assert re_.top2([2.0, 7.0, 7.0]) == (7.0, 7.0, 1) and re_.top2([4.0]) == (4.0, -np.inf, 0)
    call = re_.make_call(3, 1025, (1, 2, 3), [2, 1, 2, 3, 2, 1, 3, 2, 2])
    ks = (5, 261, 1024)
    re_.place_tie(call, 2, ks)
    for b in range(call.n):
        w = call.exact(b)
        v1, v2, i = re_.top2(w)
        if call.jg[b] == 2:
            assert (v1 == v2) and i == ks[0] and w[ks[1]] == v1 and w[ks[2]] == v1
            assert re_.argmax_last(w) == ks[2]                     # the mutant is wrong on every tie job
            fa = call.fast(b, cand=ks)
            assert fa[0] == fa[1] == fa[2]
        else:
            assert i in ks and v1 > v2
