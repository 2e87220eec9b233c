"""The A-transform planner as it was BEFORE runs were priced by what a chunk iteration costs, restated in plain Python, and the
cost model the planner uses now -- the reference of test_atrans_plan_cost_cpu.py and the source of the plans that
test_hip_atrans_plan_equal.py injects.

`parent_plan` is the greedy planner of the parent commit: a column block of a layer costs its number of contraction chunks, a
segment `blocks * chunks + 6`; binary search on the largest run cost, greedy maximal runs, at most R runs per row tile; few rows:
R = ceil(blocks / 7) runs and S slices of the contraction, one workgroup per (segment, slice).  It is tied to the parent LIBRARY by
tests/golden/atrans_parent_plans.json: plan integers recorded from the parent's rcb_atrans_plan, which the restatement must
reproduce int for int.

`run_costs` prices a plan (either planner's) under the new model: a segment of `blocks` column blocks over `chunks` chunk
iterations costs chunks * (F + blocks) + E, with F_RAGGED for F in a layer whose size is no multiple of 8 (its x rows are staged
through registers); a workgroup pays the sum of its segments (S = 1) or its one (segment, slice)."""
import numpy as np

import atrans_emul as ae

# the constants of recombiner_amd/csrc/atrans.hip (PLAN_F, PLAN_E, PLAN_F_RAGGED), from profiles/r09_atrans_wg_stamps_*.txt
F, E, F_RAGGED = 3, 28, 20


def _blocks(sizes):
    return [(l, cb, ae.pad32(L) // ae.BK, 2 if L % 8 else ae.MAXSEG) for l, L in enumerate(sizes) for cb in range(ae.pad32(L) // 32)]


def _run(blks, b0, b1, seg_cost):
    """(cost, [(layer, first block, blocks)]) of blocks [b0, b1) as one run: cut at layer boundaries, pieces of more than maxseg
    blocks in near-equal parts"""
    cost, segs, i = 0, [], b0
    while i < b1:
        j = i
        while j < b1 and blks[j][0] == blks[i][0]:
            j += 1
        n, ms = j - i, blks[i][3]
        parts = (n + ms - 1) // ms
        done = 0
        for p in range(parts):
            m = (n - done + (parts - p) - 1) // (parts - p)
            cost += seg_cost(m, blks[i][2])
            segs.append((blks[i][0], blks[i + done][1], m))
            done += m
        i = j
    return cost, segs


def regime(rows, sizes, n_cu):
    """(row tiles, R, S) by the rules both planners share"""
    nb = len(_blocks(sizes))
    m_tiles = (rows + ae.BM - 1) // ae.BM
    R = min(max(1, n_cu // m_tiles), (nb + 1) // 2)
    runs_full = (nb + ae.MAXSEG - 1) // ae.MAXSEG
    S = 1
    if m_tiles * runs_full * 2 <= n_cu:
        S = min(8, n_cu // (m_tiles * runs_full))
        R = runs_full
    return m_tiles, R, S


def parent_runs(rows, sizes, n_cu):
    """the parent's runs of one row tile: [[(layer, first block, blocks), ...], ...]"""
    blks = _blocks(sizes)
    nb = len(blks)
    _, R, _ = regime(rows, sizes, n_cu)
    old = lambda m, w: m * w + 6

    def fits(bound):
        b, cuts = 0, []
        while b < nb:
            e = b + 1
            if _run(blks, b, e, old)[0] > bound:
                return None
            while e < nb and _run(blks, b, e + 1, old)[0] <= bound:
                e += 1
            cuts.append(e)
            b = e
            if len(cuts) > R:
                return None
        return cuts

    lo, hi = 0, _run(blks, 0, nb, old)[0]
    while lo < hi:
        mid = (lo + hi) // 2
        if fits(mid) is not None:
            hi = mid
        else:
            lo = mid + 1
    out, b = [], 0
    for e in fits(hi):
        out.append(_run(blks, b, e, old)[1])
        b = e
    return out


def encode(rows, sizes, n_cu, runs):
    """the plan integers rcb_atrans_plan writes for these runs of a row tile (the layout atrans_emul.read_plan parses)"""
    m_tiles, _, S = regime(rows, sizes, n_cu)
    nc = [ae.pad32(L) // ae.BK for L in sizes]
    slabs = [min(S, c) for c in nc]
    begin, segs = [], []
    for mt in range(m_tiles):
        for run in runs:
            if S == 1:
                begin.append(len(segs))
                segs += [[l, mt * ae.BM, cb, m, 0, nc[l], -1, 0] for l, cb, m in run]
            else:
                for l, cb, m in run:
                    for k in range(slabs[l]):
                        begin.append(len(segs))
                        segs.append([l, mt * ae.BM, cb, m, k * nc[l] // slabs[l], (k + 1) * nc[l] // slabs[l], k, 0])
    begin.append(len(segs))
    n_wg = len(begin) - 1
    head = (ae.PLAN_HEAD + n_wg + 1 + 3) // 4 * 4
    raw = np.zeros(head + 8 * len(segs), dtype=np.int32)
    raw[0], raw[1], raw[2] = n_wg, len(segs), S
    if S > 1:
        raw[4:4 + len(sizes)] = slabs
    raw[ae.PLAN_HEAD:ae.PLAN_HEAD + n_wg + 1] = begin
    raw[head:] = np.array(segs, dtype=np.int32).reshape(-1)
    return raw


def parent_plan(rows, sizes, n_cu):
    return encode(rows, sizes, n_cu, parent_runs(rows, sizes, n_cu))


def parse(raw):
    """(seg_begin, segs [n, 8], S) of plan integers"""
    n_wg, n_segs = int(raw[0]), int(raw[1])
    head = (ae.PLAN_HEAD + n_wg + 1 + 3) // 4 * 4
    return raw[ae.PLAN_HEAD:ae.PLAN_HEAD + n_wg + 1], raw[head:head + 8 * n_segs].reshape(n_segs, 8), int(raw[2])


def run_costs(raw, sizes):
    """cost of every workgroup of a plan under the new model"""
    begin, segs, _ = parse(raw)
    f = np.array([F_RAGGED if L % 8 else F for L in sizes])[segs[:, 0]]
    c = (segs[:, 5] - segs[:, 4]).astype(np.int64) * (f + segs[:, 3]) + E
    cum = np.r_[0, np.cumsum(c)]
    return cum[begin[1:]] - cum[begin[:-1]]


def runs_of(raw):
    """[[(layer, first block, blocks), ...] per workgroup]"""
    begin, segs, _ = parse(raw)
    return [[(int(s[0]), int(s[2]), int(s[3])) for s in segs[begin[i]:begin[i + 1]]] for i in range(len(begin) - 1)]
