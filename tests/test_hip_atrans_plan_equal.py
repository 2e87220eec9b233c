"""Which workgroup computes a column block of the A transform changes no element: every output still accumulates its chunks in
order, in one segment (and K slice), from zero.  So the result under the planner's plan (runs priced by what a chunk iteration
costs) must be BIT FOR BIT the result under the plan the greedy planner of the parent commit made (atrans_plan_ref.parent_plan,
tied to the parent library by tests/golden/atrans_parent_plans.json), on real-valued inputs where the order of the sums matters.

The parent's plan goes in through ATransform._plans[rows]; n_cu is pinned, so the plans do not depend on the device.  The cases
are the smallest at which the two plans differ (asserted: a case with equal plans proves nothing):

    sizes            rows  n_cu  regime                the parent's plan straddles with
    (288, 288, 33)    513    16  S = 1                 [(0, 8, 1), (1, 0, 2)]
    (352, 352, 99)    300     8  S = 1, ragged tail    [(0, 6, 5), (1, 0, 1)]
    (528, 272, 51)    256     8  S = 2                 --
"""
import ctypes

import numpy as np
import pytest
import torch

import atrans_emul as ae
import atrans_plan_ref as pr

from recombiner_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(ae.Case((288, 288, 33), 513, 16), 1, [(0, 8, 1), (1, 0, 2)]),
         (ae.Case((352, 352, 99), 300, 8), 1, [(0, 6, 5), (1, 0, 1)]),
         (ae.Case((528, 272, 51), 256, 8), 2, None)]


def _inject(tr, case, raw):
    head = (ctypes.c_int32 * ae.PLAN_HEAD)(*[int(v) for v in raw[:ae.PLAN_HEAD]])
    sz = (ctypes.c_int32 * len(case.sizes))(*case.sizes)
    nws = int(_lib.load().rcb_atrans_workspace_floats(case.rows, len(case.sizes), sz, head))
    tr._plans[case.rows] = (torch.from_numpy(raw.astype(np.int32)).to(DEV), head, nws)


@pytest.mark.parametrize("case,S,straddle", CASES, ids=lambda v: ae.case_id(v) if isinstance(v, ae.Case) else "")
def test_result_under_the_parent_plan_is_bit_identical(case, S, straddle):
    new_raw = ae.read_plan(case.rows, case.sizes, case.n_cu).raw
    old_raw = pr.parent_plan(case.rows, case.sizes, case.n_cu)
    assert int(new_raw[2]) == int(old_raw[2]) == S
    assert not np.array_equal(new_raw, old_raw)                                   # the two plans differ
    old_runs, new_runs = pr.runs_of(old_raw), pr.runs_of(new_raw)
    assert sorted(map(tuple, old_runs)) != sorted(map(tuple, new_runs))           # ... in their runs, not only in their order
    if straddle is not None:
        assert straddle in old_runs and straddle not in new_runs
    x, A = ae.case_inputs(case, real=True)                                        # x = 0.03 randn, A = randn / sqrt(n)
    xg, Ag = x.to(DEV), [a.to(DEV) for a in A]
    planes = ops.Planes.from_float(xg)
    rows, D = case.rows, sum(case.sizes)
    for terms in (1, 2, 3):
        tn = ops.ATransform(ae.slices_of(case.sizes), DEV, terms=terms)
        tn.n_cu = case.n_cu
        to = ops.ATransform(ae.slices_of(case.sizes), DEV, terms=terms)
        to.n_cu = case.n_cu
        _inject(to, case, old_raw)
        tn.prepare(Ag)
        to.prepare(Ag)
        for form, src in (("rows", xg), ("planes", planes)):
            for name in ("forward", "dgrad"):
                got = getattr(tn, name)(src, torch.full((rows, D), float("nan"), device=DEV))
                ref = getattr(to, name)(src, torch.full((rows, D), float("nan"), device=DEV))
                assert not bool(got.isnan().any()), (name, terms, form)
                assert torch.equal(got, ref), "%s, terms %d, %s: %d elements differ" % (name, terms, form, int((got != ref).sum()))
        assert np.array_equal(tn._plan(rows)[0].cpu().numpy(), new_raw)           # the planner's plan was the one that ran
        assert np.array_equal(to._plan(rows)[0].cpu().numpy(), old_raw)
