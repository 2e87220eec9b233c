"""The A* scorers of rec_score.hip (rec_prep / rec_fast / rec_finish / rec_exact and the arbiter launch) against the evaluator of
tests/rec_emul.py, whose premises test_rec_emul_cpu.py checks on the CPU.  Everything goes through ops.RecTables, ops.RecJobs,
ops.rec_score and ops.rec_commit.

  logf        the device's fp32 logf is RECOVERED, not assumed: an EXACT-mode call on one-element jobs (K = 1, table [[0]], Gumbel
              [0], loc = p_loc = 0, p_scale = 1) returns best[j, 0] = fl(fl(-l - c) + c), l = logf(scale[j]), c = log sqrt(2 pi);
              exactly one of the five fp32 neighbours of the host log reproduces it (device_logf asserts that).  Every
              bit-exact test below hands these logs to the evaluator, for posterior and prior scales alike.
  exact       logw_job0 (all K) and best / idx of every job in EXACT mode, bit for bit: K in {1, 5, 255, 1000, 1024, 1025, 4099},
              each with 1, 7, 8, 9 and 17 jobs, g cycling through {1, 2, 3, 7, 12, 33} from another start in every case, unsorted job lists.
  fast        best[:, 0], best[:, 1], idx and the certificate of every job in FAST mode against fast_scores, bit for bit
              (K <= 1025, g <= 12): the file is compiled with contraction off, fp64 division is IEEE, the FMAs are explicit.
              It holds: see FAST_BIT_FOR_BIT below.
  tau / 4     |best_fast[:, 0] - best_exact[:, 0]| <= tau / 4 per job, tau from the evaluator, on the 3 x 4096 random jobs of
              test_rec_fast_scorer_equals_exact_scorer_on_many_random_jobs (whose limit was 1e-7, a thousand times tau).
  ties        two or three candidates with identical table rows and Gumbel values above all others, placed in one thread, in
              neighbouring lanes, in lanes 0 and 63, in two waves, in two spans, in the first and the last span and in spans s
              and s + 64 (one lane of rec_finish_kernel); K in {1025, 4099, 65 536, 66 563}: the lowest index wins in both modes,
              best[:, 0] == best[:, 1], FAST mode flags the job; the other jobs of the call return the evaluator's arg-max.
  arbiter     64 calls of 16 jobs with one tuned near-tie each (rec_emul.arbiter_call): FAST idx == EXACT idx, `uncertified` is
              1 exactly at the tuned job, whose best is the exact scorer's bit for bit; the others keep the fast scorer's.
  mixed runs  an unsorted device job list with lengths 2, 5, 2, (no table), 5, 2, 1, 5 in its first workgroup.
  NaN         a job whose scores are all NaN: idx = -1 in both modes, nothing committed, neighbours unaffected.
              (rec_exact_kernel returned 2147483647, the never-pushed sentinel, until this suite; the reference's torch.argmax
              would code such a group at index 0.)

Where a test compares an index with host-log evaluator scores, the evaluator's top-2 gap is first ASSERTED to exceed 1e-6 g, far
above what a one-ulp logf difference (6e-8 |log s| per element, the same for every candidate up to fp64 rounding) can move: a
condition on the inputs; no job is left out."""
import copy

import numpy as np
import pytest
import torch

import rec_emul as re_
from golden_util import O

from recombiner_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = np.float32, np.float64
MODES = (ops.REC_EXACT, ops.REC_FAST)
G6 = (1, 2, 3, 7, 12, 33)
G5 = (1, 2, 3, 7, 12)

# from the first MI355X run (the tests print these figures with -s; no limit is derived from them)
FAST_BIT_FOR_BIT = """
fast scorer against fast_scores         bit for bit on all six cases (51 jobs): best[:, 0], best[:, 1], idx
exact scorer against exact_scores       bit for bit on all 35 cases, logw_job0 included
winner score, |fast - exact| / (tau/4)  worst 0.018 over the 12 288 jobs
device logf against the host's          differs (by one or two fp32 ulps) in 12 697 of 25 002 probed values; always unique
arbiter                                 overrode the fast scorer's pick in 27 of the 64 tuned jobs; the exact scorer took the
                                        higher index of the pair in 24
"""


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tables_of(call):
    return ops.RecTables.from_dict({g: torch.from_numpy(t) for g, t in call.tables.items()}, DEV, call.K)


def run(call, mode, tabs=None, want_logw0=False, jobs=None):
    """-> idx, best [n, 2], uncertified, logw0 as numpy; the job list goes to the device in the call's own order"""
    tabs = tables_of(call) if tabs is None else tabs
    if jobs is None:
        jobs, _ = ops.RecJobs.from_host(DEV, call.jr, call.js, call.jg, sort=False)
    idx, best, unc, lw0 = ops.rec_score(dev(call.loc), dev(call.scale), dev(call.pl), dev(call.ps), tabs, dev(call.gumbel), jobs,
                                        mode, want_logw0)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), best.cpu().numpy(), unc.cpu().numpy(), None if lw0 is None else lw0.cpu().numpy()


# ---- 3a: the device's logf ----------------------------------------------------------------------------------------------------
class DeviceLogs:
    """logf of the device for the given fp32 values, recovered through the exact scorer; call it with an fp32 array"""

    def __init__(self, values):
        v = np.unique(re_.f32(values).reshape(-1))
        host = re_.host_logf(v)
        assert (np.abs(host) >= 2.0 ** -20).all(), "probe scales too close to 1"
        n = v.shape[0]
        tabs = ops.RecTables.from_dict({1: torch.zeros(1, 1, dtype=torch.float64)}, DEV, 1)
        jobs, _ = ops.RecJobs.from_host(DEV, np.zeros(n), np.arange(n), np.ones(n), sort=False)
        _, best, _, _ = ops.rec_score(dev(np.zeros((1, n), F32)), dev(v[None]), dev(np.zeros(n, F32)), dev(np.ones(n, F32)), tabs,
                                      dev(np.zeros(1, F64)), jobs, ops.REC_EXACT)
        got = best[:, 0].cpu().numpy()
        up1 = np.nextafter(host, F32(np.inf))
        dn1 = np.nextafter(host, F32(-np.inf))
        cands = np.stack([np.nextafter(dn1, F32(-np.inf)), dn1, host, up1, np.nextafter(up1, F32(np.inf))], 1)
        pred = (-cands.astype(F64) - re_.LOG_SQRT_2PI) + re_.LOG_SQRT_2PI
        hit = pred == got[:, None]
        assert (hit.sum(1) == 1).all(), "the device's logf is not one of the five fp32 neighbours of the host's, or not unique"
        self.v, self.log = v, cands[np.arange(n), hit.argmax(1)]
        self.n_differ = int((self.log != host).sum())

    def __call__(self, s):
        s = re_.f32(s)
        i = np.searchsorted(self.v, s)
        assert np.array_equal(self.v[i], s)
        return self.log[i]


def logs_of(*calls):
    return DeviceLogs(np.concatenate([np.concatenate([c.scale.reshape(-1), c.ps]) for c in calls]))


def test_device_logf_is_recovered_uniquely():
    rs = np.random.RandomState(0)
    v = np.concatenate([np.exp(rs.uniform(-12, 3, size=20000)), 0.015 + 0.01 * rs.rand(5000), [0.5, 2.0, 1e-15, 1e15, 0.999, 1.001]])
    logs = DeviceLogs(v.astype(F32))                      # asserts that one neighbour, and only one, reproduces each value
    print("device logf differs from the host's in %d of %d probed values" % (logs.n_differ, logs.v.shape[0]))


# ---- 3b: the exact scorer, bit for bit ----------------------------------------------------------------------------------------
EXACT_CASES = [(K, n) for K in (1, 5, 255, 1000, 1024, 1025, 4099) for n in (1, 7, 8, 9, 17)]      # job b of case i: g = G6[(i + b) % 6]


@pytest.mark.parametrize("i", range(len(EXACT_CASES)), ids=["K%d-n%d" % c for c in EXACT_CASES])
def test_exact_scorer_bit_for_bit(i):
    K, n = EXACT_CASES[i]
    jg = [G6[(i + b) % 6] for b in range(n)]
    call = re_.make_call(20 + i, K, sorted(set(jg)), jg, ratio=(0.03, 0.3, 1.0)[i % 3], clamp=2)
    logs = logs_of(call)
    idx, best, unc, lw0 = run(call, ops.REC_EXACT, want_logw0=True)
    assert not unc.any()
    for b in range(n):
        w = call.exact(b, logs)
        v1, v2, k = re_.top2(w)
        if b == 0:
            assert np.array_equal(lw0, w), (K, jg[0], int((lw0 != w).sum()), float(np.abs(lw0 - w).max()))
        assert (idx[b], best[b, 0], best[b, 1]) == (k, v1, v2), (K, b, jg[b])


# ---- 3c: the fast scorer, bit for bit -----------------------------------------------------------------------------------------
FAST_CASES = [(1, 8), (5, 9), (255, 7), (1000, 1), (1024, 9), (1025, 17)]


@pytest.mark.parametrize("i", range(len(FAST_CASES)), ids=["K%d-n%d" % c for c in FAST_CASES])
def test_fast_scorer_bit_for_bit(i):
    K, n = FAST_CASES[i]
    jg = [G5[(i + b) % 5] for b in range(n)]
    call = re_.make_call(40 + i, K, sorted(set(jg)), jg, ratio=(0.03, 0.3, 1.0)[(i + 1) % 3], clamp=2)
    logs = logs_of(call)
    idx, best, unc, _ = run(call, ops.REC_FAST)
    worst = 0.0
    for b in range(n):
        w = call.fast(b, logs)
        v1, v2, k = re_.top2(w)
        tau = call.tau(b, logs)
        if K > 1:
            worst = max(worst, abs(best[b, 0] - v1) / tau, abs(best[b, 1] - v2) / tau)
        if (v1 - v2) > tau:
            assert unc[b] == 0 and (idx[b], best[b, 0], best[b, 1]) == (k, v1, v2), (K, b, jg[b], best[b], (v1, v2))
        else:                                   # the arbiter's: index and both scores are the exact scorer's
            e1, e2, ke = re_.top2(call.exact(b, logs))
            assert unc[b] == 1 and (idx[b], best[b, 0], best[b, 1]) == (ke, e1, e2), (K, b, jg[b])
    print("fast scorer K = %d: worst |device - evaluator| / tau = %.3g" % (K, worst))


def test_fast_and_exact_winner_scores_agree_within_a_quarter_of_tau():
    """the 3 x 4096 jobs of test_rec_fast_scorer_equals_exact_scorer_on_many_random_jobs.  tau is the evaluator's with host logs:
    an ulp of logf moves S, a sum of magnitudes of which |log s| is one term of six, by less than 1e-7 of itself."""
    K = 65536
    gum_c = O.gumbel_table(42)
    gum = dev(gum_c)
    tabs = ops.RecTables(DEV, K)
    X = {}
    for gl in range(1, 13):
        t = O.sobol_normal_table(gl)
        tabs.add(gl, t)
        X[gl] = float(t.abs().max())
    G = float(np.abs(gum_c).max())
    worst = 0.0
    for seed, ratio in ((1, 0.03), (2, 0.2), (3, 1.0)):
        loc, scale, pl, ps, jr, js, jg = re_.random_problem(seed, 64, 600, list(range(1, 13)), 4096, ratio)
        jobs, order = ops.RecJobs.from_host(DEV, jr, js, jg, rows=64, cols=600)
        args = (dev(loc), dev(scale), dev(pl), dev(ps), tabs, gum)
        i_exact, b_exact, _, _ = ops.rec_score(*args, jobs, ops.REC_EXACT)
        i_fast, b_fast, unc, _ = ops.rec_score(*args, jobs, ops.REC_FAST)
        assert torch.equal(i_exact, i_fast)
        err = (b_fast[:, 0] - b_exact[:, 0]).abs().cpu().numpy()
        jr, js, jg = jr[order], js[order], jg[order]
        tau = np.zeros(4096)
        for gl in range(1, 13):
            m = np.nonzero(jg == gl)[0]
            cols = js[m, None] + np.arange(gl)[None]
            c = re_.constants(loc[jr[m, None], cols], scale[jr[m, None], cols], pl[cols], ps[cols])
            tau[m] = re_.tau(c, X[gl], G)[0]
        assert (tau > 0).all() and (err <= tau / 4).all(), float((err / tau).max())
        worst = max(worst, float((err / (tau / 4)).max()))
    print("winner score, |fast - exact| / (tau / 4): worst %.4f" % worst)


# ---- 3d: ties -----------------------------------------------------------------------------------------------------------------
def placements(K):
    n_span = (K + re_.SPAN - 1) // re_.SPAN
    last = (n_span - 1) * re_.SPAN
    p = {"one thread": (7, 7 + re_.THREADS), "neighbouring lanes": (130, 131), "lanes 0 and 63": (192, 255),
         "two waves": (70, 134), "two spans": (K - 1 - re_.SPAN, K - 1), "first and last span": (3, last),
         "three: two waves and the last span": (200, 264, last), "three in one thread": (9, 9 + 2 * re_.THREADS, 9 + 3 * re_.THREADS)}
    if n_span > 64:
        p["spans 0 and 64"] = (10, 64 * re_.SPAN + 10)
        p["spans 1 and 65"] = (re_.SPAN + 5, 65 * re_.SPAN + 1)
        p["three: spans 0, 1 and 64"] = (600, re_.SPAN + 600, 64 * re_.SPAN + 600)
    assert all(0 <= k < K for ks in p.values() for k in ks)
    return p


TIE_JG = [2, 1, 2, 3, 2, 1, 3, 2, 2, 1, 3]


@pytest.mark.parametrize("K", [1025, 4099, 65536, 66563])
def test_ties_take_the_lowest_index_wherever_they_are_placed(K):
    base = re_.make_call(60 + K % 7, K, (1, 2, 3), TIE_JG, ratio=0.5)
    for name, ks in placements(K).items():
        call = re_.place_tie(copy.deepcopy(base), 2, ks)
        want = []
        for b in range(call.n):
            v1, v2, k = re_.top2(call.exact(b))
            if call.jg[b] == 2:
                assert v1 == v2 and k == ks[0]
            else:
                assert v1 - v2 > 1e-6 * call.jg[b], (name, b)       # a condition on the inputs
            want.append(k)
        tabs = tables_of(call)
        for mode in MODES:
            idx, best, unc, _ = run(call, mode, tabs)
            assert idx.tolist() == want, (K, name, mode, idx.tolist(), want)
            tie = call.jg == 2
            assert (best[tie, 0] == best[tie, 1]).all() and (best[~tie, 0] > best[~tie, 1]).all(), (K, name, mode)
            assert unc.tolist() == ((tie.astype(int)).tolist() if mode == ops.REC_FAST else [0] * call.n), (K, name, mode)


# ---- 3e: the arbiter ----------------------------------------------------------------------------------------------------------
def _pick(fa, a, k2):
    return a if (fa[0] > fa[1] or (fa[0] == fa[1] and a < k2)) else k2


def test_the_arbiter_decides_tuned_near_ties():
    K = 4099
    t = re_.arbiter_tables(K)
    tabs = ops.RecTables.from_dict({g: torch.from_numpy(t[g]) for g in re_.ARB_LENS}, DEV, K)
    calls = [re_.arbiter_call(n, K, tables=t) for n in range(64)]
    logs = logs_of(*[c[0] for c in calls])
    higher = overridden = 0
    for n, (call, slot, (a, k2)) in enumerate(calls):
        i_e, b_e, _, _ = run(call, ops.REC_EXACT, tabs)
        i_f, b_f, unc, _ = run(call, ops.REC_FAST, tabs)
        assert np.array_equal(i_e, i_f), (n, i_e, i_f)
        assert unc.tolist() == [int(b == slot) for b in range(call.n)], (n, slot, unc)
        assert (b_f[slot, 0], b_f[slot, 1]) == (b_e[slot, 0], b_e[slot, 1]), (n, b_f[slot], b_e[slot])
        for b in range(call.n):
            w = call.exact(b, logs)
            v1, v2, k = re_.top2(w)
            assert (i_e[b], b_e[b, 0], b_e[b, 1]) == (k, v1, v2), (n, b)
            fa = call.fast(b, logs, cand=[a, k2])            # a and k2 are >= 8 above every other candidate in every job
            if b != slot:
                assert (b_f[b, 0], b_f[b, 1]) == (max(fa), min(fa)) and i_f[b] == _pick(fa, a, k2), (n, b, b_f[b], fa)
            else:
                assert abs(fa[0] - fa[1]) <= call.tau(b, logs)
                overridden += _pick(fa, a, k2) != i_f[b]
                higher += i_f[b] == max(a, k2)
    print("arbiter: overrode the fast pick in %d of 64 tuned jobs; the exact scorer took the higher index in %d" % (overridden, higher))
    assert higher >= 8, higher


# ---- 3f, 3g: mixed runs, rejected and NaN jobs inside a workgroup ------------------------------------------------------------------
def _windowed_call(seed, jg, lens, K=1025):
    """jobs on disjoint windows (job b: row b % 6, columns 6 b ..), so that what rec_commit writes for one job is its own"""
    call = re_.make_call(seed, K, lens, jg, ratio=0.5, N=6, D=6 * len(jg))
    call.jr, call.js = np.arange(call.n) % 6, 6 * np.arange(call.n)
    return call


def _score_and_commit(call, mode, tabs):
    i32 = torch.int32
    n = call.n
    jobs = ops.RecJobs(*(torch.tensor(v, dtype=i32, device=DEV) for v in (call.jr, call.js, call.jg, np.arange(n))))
    idx, best, unc, _ = run(call, mode, tabs, jobs=jobs)
    sample = torch.zeros(6, call.pl.shape[0], device=DEV)
    done = torch.zeros(6, n, device=DEV, dtype=torch.uint8)
    igw = torch.full((6, n), -7, device=DEV, dtype=i32)
    ops.rec_commit(dev(call.pl), dev(call.ps), tabs, jobs, torch.from_numpy(idx).to(DEV), n_groups=n, enc_sample=sample, done=done,
                   idx_groupwise=igw)
    torch.cuda.synchronize()
    return idx, sample.cpu().numpy(), done.cpu().numpy(), igw.cpu().numpy()


def _check_jobs(call, bad, idx, sample, done, igw, what):
    for b in range(call.n):
        r, s, g = int(call.jr[b]), int(call.js[b]), int(call.jg[b])
        if b == bad:
            assert idx[b] == -1, (what, idx)
            assert (sample[r, s:s + 6] == 0).all() and done[r, b] == 0 and igw[r, b] == -7, what
            continue
        v1, v2, k = re_.top2(call.exact(b))
        assert v1 - v2 > 1e-6 * g, (what, b)                      # a condition on the inputs
        assert idx[b] == k, (what, b, idx[b], k)
        z = call.pl[s:s + g].astype(F64) + call.ps[s:s + g].astype(F64) * call.xi(b)[k]
        assert np.array_equal(sample[r, s:s + g], z.astype(F32)) and done[r, b] == 1 and igw[r, b] == k, (what, b)
    assert int(done.sum()) == call.n - 1


def test_mixed_runs_and_a_rejected_job_inside_one_workgroup():
    jg = [2, 5, 2, 4, 5, 2, 1, 5] + [1, 2, 5, 5, 2, 1, 2, 5, 1]
    call = _windowed_call(71, jg, (1, 2, 5))                      # no table of length 4: job 3 is rejected on the device
    tabs = tables_of(call)
    for mode in MODES:
        _check_jobs(call, 3, *_score_and_commit(call, mode, tabs), what=("mixed", mode))


@pytest.mark.parametrize("slot,field", [(3, "loc"), (0, "loc"), (12, "scale")])
def test_a_job_with_nan_scores_is_left_uncoded(slot, field):
    jg = [3] * 9 + [1, 1, 2, 2, 2, 3, 3, 1]
    call = _windowed_call(72, jg, (1, 2, 3))
    getattr(call, field)[call.jr[slot], call.js[slot] + call.jg[slot] - 1] = np.nan
    assert np.isnan(call.exact(slot)).all()
    tabs = tables_of(call)
    for mode in MODES:
        _check_jobs(call, slot, *_score_and_commit(call, mode, tabs), what=("nan", slot, field, mode))
