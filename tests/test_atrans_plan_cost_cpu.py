"""CPU tests of the A-transform planner's cost model: a segment of `blocks` column blocks over `chunks` chunk iterations costs its
workgroup chunks * (F + blocks) + E (atrans_plan_ref.F / E / F_RAGGED = PLAN_F / PLAN_E / PLAN_F_RAGGED of atrans.hip; F_RAGGED for
F in layers whose size is no multiple of 8), not blocks * chunks + 6.

The reference is the planner of the parent commit, restated in atrans_plan_ref.parent_plan and tied to the parent library by
tests/golden/atrans_parent_plans.json (recorded from the parent's rcb_atrans_plan).  Over rows x CU counts x layer lists of
test_atrans_emul_cpu.py, the headline (4096 rows, 256 CUs) and the CIFAR test-time batch (2500 rows):
  * priced by the new model, the most expensive workgroup of the new plan costs no more than that of the parent's plan;
  * the new plan has no more workgroups than the parent's rules allow: R runs per row tile (S = 1); K-split: no more than the
    parent's plan itself (and so at most every layer in its fewest segments plus one more per run boundary, times its slices);
  * headline and 2500 rows: no run holds segments of two layers of 8 or more blocks.
The library must be built; a GPU is not needed."""
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

import atrans_emul as ae
import atrans_plan_ref as pr
from test_atrans_emul_cpu import PLAN_CUS, PLAN_ROWS, PLAN_SIZES

HEADLINE = (1056, 1056, 1056, 99)
EXTRA = ((4096, 256, HEADLINE), (2500, 256, HEADLINE))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "atrans_parent_plans.json")


def _key(rows, n_cu, sizes):
    return "%d/%d/%s" % (rows, n_cu, "x".join(map(str, sizes)))


def _grid(sizes):
    pts = [(r, c, sizes) for r, c in itertools.product(PLAN_ROWS, PLAN_CUS)]
    return pts + [p for p in EXTRA if p[2] == sizes]


def test_the_constants_are_the_library_s():
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "recombiner_amd", "csrc", "atrans.hip")).read()
    assert "constexpr int PLAN_F = %d, PLAN_E = %d, PLAN_F_RAGGED = %d;" % (pr.F, pr.E, pr.F_RAGGED) in src


@pytest.mark.parametrize("sizes", PLAN_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_restated_parent_planner_is_the_recorded_one(sizes):
    gold = json.load(open(GOLDEN))
    for rows, n_cu, _ in _grid(sizes):
        raw = pr.parent_plan(rows, sizes, n_cu)
        assert hashlib.sha256(raw.astype("<i4").tobytes()).hexdigest()[:16] == gold["sha256_16"][_key(rows, n_cu, sizes)], (rows, n_cu)


def test_restated_parent_planner_reproduces_the_recorded_integers():
    gold = json.load(open(GOLDEN))
    assert len(gold["plans"]) == 3
    for key, ints in gold["plans"].items():
        rows, n_cu, sizes = key.split("/")
        raw = pr.parent_plan(int(rows), tuple(int(s) for s in sizes.split("x")), int(n_cu))
        assert raw.tolist() == ints, key


@pytest.mark.parametrize("sizes", PLAN_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_largest_run_cost_and_workgroup_count_against_the_parent_plan(sizes):
    strictly_better = 0
    for rows, n_cu, _ in _grid(sizes):
        where = (rows, n_cu, sizes)
        new = ae.read_plan(rows, sizes, n_cu).raw
        old = pr.parent_plan(rows, sizes, n_cu)
        m_tiles, R, S = pr.regime(rows, sizes, n_cu)
        assert int(new[2]) == S == int(old[2]), where
        c_new, c_old = int(pr.run_costs(new, sizes).max()), int(pr.run_costs(old, sizes).max())
        assert c_new <= c_old, where
        strictly_better += c_new < c_old
        if S == 1:
            allowed = m_tiles * R
        else:
            nblk = [ae.pad32(L) // 32 for L in sizes]
            fewest = sum(min(S, n) * -(-n // (2 if L % 8 else ae.MAXSEG)) for n, L in zip(nblk, sizes))
            assert int(old[0]) <= m_tiles * (fewest + (R - 1) * S), where
            allowed = int(old[0])
        assert int(new[0]) <= allowed, where
        if S == 1:                       # every run is one workgroup: as many as the parent's rule R allows, where it pays
            assert int(new[0]) % m_tiles == 0 and int(new[0]) // m_tiles <= R, where
    if len(sizes) > 1 and max(sizes) >= 256:
        assert strictly_better > 0       # layer lists with wide layers: somewhere the parent's plan paid for a straddling run


@pytest.mark.parametrize("rows,n_cu,sizes", EXTRA, ids=lambda v: str(v) if isinstance(v, int) else "headline")
def test_no_run_over_two_wide_layers(rows, n_cu, sizes):
    nblk = [ae.pad32(L) // 32 for L in sizes]
    wide = lambda run: {l for l, _, _ in run if nblk[l] >= 8}
    new_runs = pr.runs_of(ae.read_plan(rows, sizes, n_cu).raw)
    assert all(len(wide(run)) <= 1 for run in new_runs)
    assert all(len(run) == 1 for run in new_runs if wide(run))           # a wide layer's run is one segment, nothing rides along
    # (the parent's plan had them: the premise of the change)
    assert sum(len(wide(run)) > 1 for run in pr.runs_of(pr.parent_plan(rows, sizes, n_cu))) == 2 * ((rows + ae.BM - 1) // ae.BM)
