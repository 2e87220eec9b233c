"""The arithmetic of the A-transform kernels (recombiner_amd/csrc/atrans.hip, the pack body of prepare_bodies.h) in fp64, written
from the definition

    forward        out[:, lo_l:hi_l] = x[:, lo_l:hi_l] @ A[l]
    data gradient  out[:, lo_l:hi_l] = x[:, lo_l:hi_l] @ A[l]^T
    weight grad.   dA[l]             = h[:, lo_l:hi_l]^T @ dw[:, lo_l:hi_l]

with the operands the kernels keep: x = hi + lo, A = hi + lo as bf16 pairs (`split`), and per number of terms

    1: x_hi A_hi        2: (x_hi + x_lo) A_hi        3: (x_hi + x_lo) A_hi + x_hi A_lo        (x_lo A_lo is never formed).

Plain torch on the CPU, float64; no indexing code is shared with the kernels.  `read_plan` is the one exception to "nothing from
recombiner_amd": it calls the host planner rcb_atrans_plan through the binding and only PARSES what comes back -- the planner is
itself under test (test_atrans_emul_cpu.py), and the fault switches that speak of segments, slices and slabs need its answer.

`lattice`: x = s (256 a + b), a in {1, 2, 3}, b in {0, 1}, s = +-1.  bf16(x) = s 256 a and lo = s b, so with x and A both from the
lattice every product of all three term forms is a multiple of 256 and at most 9 * 65536; `budget` is sum |p| / 256 per output
element and stays below 2^24 up to K = 4160 (worst case 4160 * 2310 = 0.573 * 2^24).  Every fp32 partial sum is then exact in any
order, and a kernel must return the evaluator's value bit for bit.

`FAULTS` / `WGRAD_FAULTS`: deliberately wrong evaluators, one named switch per defect the inputs must expose (never a property of a kernel).

`wgrad_narrow_chain`: the fp32 restatement of wgrad_narrow_kernel + wgrad_narrow_sum_kernel, one correctly rounded fma per row
in row order (`fma32`: exact product in fp64, TwoSum, round to odd, round to fp32), waves as ((w0 + w1) + w2) + w3, slabs in
slab order.
"""
import ctypes
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

F64 = torch.float64
F32 = torch.float32
BF = torch.bfloat16
EXACT = 2.0 ** 24
EPS32 = 2.0 ** -23
PLAN_HEAD = 12                      # RCB_ATRANS_PLAN_HEAD
MAX_LAYERS = 8                      # RCB_ATRANS_MAX_LAYERS
BM, BK, MAXSEG = 256, 32, 7         # row tile, contraction chunk, longest segment (atrans.hip)


def pad32(n):
    return (n + 31) // 32 * 32


def slices_of(sizes):
    cum = np.cumsum([0] + list(sizes))
    return [(int(cum[i]), int(cum[i + 1])) for i in range(len(sizes))]


def split(v):
    """fp32 -> (hi, lo) bf16: hi = bf16(v), lo = bf16(v - hi), by torch casts (ops.Planes.from_float, the kernels' x_convert)"""
    v = v.to(F32)
    hi = v.to(BF)
    lo = (v - hi.to(F32)).to(BF)
    return hi, lo


_SPLITS = {}


def split64(v, keep=False):
    """the split as fp64; keep: remember it for this tensor (the mappings of a case are split once, not once per call)"""
    if keep and id(v) in _SPLITS and _SPLITS[id(v)][0] is v:
        return _SPLITS[id(v)][1:]
    hi, lo = split(v)
    hi, lo = hi.to(F64), lo.to(F64)
    if keep:
        if len(_SPLITS) >= 16:
            _SPLITS.clear()
        _SPLITS[id(v)] = (v, hi, lo)
    return hi, lo


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def lattice(shape, gen):
    a = torch.randint(1, 4, shape, generator=gen)
    b = torch.randint(0, 2, shape, generator=gen)
    s = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (s * (256 * a + b)).to(F32)


def small_ints(shape, gen, m=4):
    return torch.randint(-m, m + 1, shape, generator=gen).to(F32)


Case = namedtuple("Case", "sizes rows n_cu")

# the lattice cases of test_hip_atrans_exact.py; test_atrans_emul_cpu.py derives from their plans which kernel instances they run
LATTICE_CASES = [
    Case((224, 40, 8, 33), 33, 256), Case((224, 40, 8, 33), 257, 1), Case((224, 40, 8, 33), 257, 256), Case((224, 40, 8, 33), 1, 8),
    Case((1056, 99), 300, 1), Case((1056, 99), 513, 256), Case((1056, 99), 33, 256),
    Case((528, 272, 51), 256, 8), Case((528, 272, 51), 257, 1), Case((528, 272, 51), 1, 256),
    Case((32,), 33, 1), Case((32,), 300, 256),
    Case((64, 64), 256, 8), Case((64, 64), 513, 1),
    Case((96,), 257, 256), Case((96,), 33, 1),
    Case((128,), 300, 8), Case((128,), 1, 1),
    Case((7,), 33, 1), Case((7,), 513, 256),
    Case((424, 440, 63), 300, 8), Case((424, 440, 63), 513, 1),
    Case((1584, 2352, 147), 64, 256), Case((1584, 2352, 147), 64, 8),
]
# real-valued inputs, held element by element to n 2^-23 sum |p|
REAL_CASES = [Case((224, 40, 8, 33), 257, 256), Case((224, 40, 8, 33), 33, 256), Case((1056, 99), 300, 1), Case((528, 272, 51), 1, 256)]

# narrow weight gradient: (L, rows); the slab count is ops.ATransform.wgrad's
WGRAD_L = (1, 31, 33, 99, 147, 256)
WGRAD_ROWS = (1, 2, 63, 65, 129, 1000, 4097)
WGRAD_CASES = [(L, r) for L in WGRAD_L for r in WGRAD_ROWS]          # at 4097 rows the trailing slabs are empty


def case_id(c):
    return "x".join(str(s) for s in c.sizes) + "-r%d-cu%d" % (c.rows, c.n_cu)


def case_inputs(case, real=False):
    """(x [rows, D], A list), seeded by the case"""
    gen = torch.Generator().manual_seed(1000 * case.rows + 7 * sum(case.sizes) + case.n_cu)
    D = sum(case.sizes)
    if real:
        return torch.randn(case.rows, D, generator=gen) * 0.03, [torch.randn(n, n, generator=gen) / n ** 0.5 for n in case.sizes]
    return lattice((case.rows, D), gen), [lattice((n, n), gen) for n in case.sizes]


def chain_inputs():
    """the real-valued narrow weight-gradient case (70 rows, L = 33) at the scales of the existing tests"""
    gen = torch.Generator().manual_seed(70033)
    return torch.randn(70, 33, generator=gen) * 0.03, torch.randn(70, 33, generator=gen) * 1e-3


def narrow_slabs(rows):
    """the slab count ops.ATransform.wgrad gives rcb_atrans_wgrad_narrow"""
    return max(1, min(64, (rows + 63) // 64))


# ---- the host planner's answer, parsed --------------------------------------------------------------------------------------------
class PlanError(Exception):
    def __init__(self, code, message):
        super().__init__("rcb_atrans_plan: %d: %s" % (code, message))
        self.code, self.message = code, message


def _planner():
    from recombiner_amd import _lib
    return _lib.load()


def read_plan(rows, sizes, n_cu):
    """rcb_atrans_plan: the size query, then the fill.  segs: one row per segment,
    [layer, row0, first column block, blocks, first chunk, end chunk, slab or -1, 0]"""
    lib = _planner()
    n = len(sizes)
    sz = (ctypes.c_int32 * max(n, 1))(*sizes)
    need = lib.rcb_atrans_plan(rows, n, sz, n_cu, None, 0)
    if need <= 0:
        raise PlanError(need, lib.rcb_last_error_string().decode(errors="replace"))
    buf = (ctypes.c_int32 * need)()
    got = lib.rcb_atrans_plan(rows, n, sz, n_cu, buf, need)
    if got <= 0:
        raise PlanError(got, lib.rcb_last_error_string().decode(errors="replace"))
    raw = np.frombuffer(buf, dtype=np.int32).copy()
    n_wg, n_segs, S = int(raw[0]), int(raw[1]), int(raw[2])
    head = (PLAN_HEAD + n_wg + 1 + 3) // 4 * 4                # where the kernel looks for the segments
    ws = int(lib.rcb_atrans_workspace_floats(rows, n, sz, (ctypes.c_int32 * PLAN_HEAD)(*[int(v) for v in raw[:PLAN_HEAD]])))
    return SimpleNamespace(raw=raw, need=int(need), written=int(got), n_wg=n_wg, n_segs=n_segs, S=S, slabs=raw[4:4 + MAX_LAYERS].copy(),
                           seg_begin=raw[PLAN_HEAD:PLAN_HEAD + n_wg + 1].copy(), head=head,
                           segs=raw[head:head + 8 * n_segs].reshape(n_segs, 8).copy(), ws_floats=ws)


def instances(plan, sizes, terms):
    """the run_segment instances a launch with this plan executes, keyed
    (effective NCB, ragged, terms, nk class 1 / 2 / 3 / 4 = `>= 4`, K-split, (blocks of the split segment, half) or None):
    a ragged layer (L % 8) runs NCB 1 or 2; the three-term form runs a segment of more than 4 blocks as two halves"""
    out = set()
    for l, _, _, w, c0, c1, slab, _ in plan.segs.tolist():
        ragged, nkc, ks = sizes[l] % 8 != 0, min(c1 - c0, 4), slab >= 0
        if ragged:
            out.add((2 if w > 1 else 1, True, terms, nkc, ks, None))
        elif terms == 3 and w > 4:
            n1 = (w + 1) // 2
            out.add((min(n1, 4), False, terms, nkc, ks, (w, 0)))
            out.add((min(w - n1, 4), False, terms, nkc, ks, (w, 1)))
        else:
            out.add((min(w, MAXSEG), False, terms, nkc, ks, None))
    return out


# ---- forward / data gradient -------------------------------------------------------------------------------------------------------
FAULTS = ("transposed", "layer_offset", "drop_partial_chunk", "padding_nonzero", "row_beyond_rows", "drop_k_slice", "slabs_as_S",
          "xlo_odd_ksteps", "alo_blocks_ge4", "terms2_for_3", "rho_swap")
WGRAD_FAULTS = ("slab_not_rounded8", "kn_swapped")


def fault_applies(fault, case, terms, plan):
    """whether the defect can show on this case at all"""
    sizes, rows = case.sizes, case.rows
    if fault == "transposed":
        return any(n > 1 for n in sizes)
    if fault == "layer_offset":
        return len(sizes) > 1
    if fault == "drop_partial_chunk":
        return any(n % 32 for n in sizes)
    if fault == "padding_nonzero":        # ragged layers zero-fill x beyond the layer: the padding rows never meet a non-zero there
        return any(n % 32 and n % 8 == 0 for n in sizes)
    if fault == "row_beyond_rows":        # 8-aligned layers compute the rows beyond the end from a repeat of the LAST row: the same
        return rows % BM != 0 and any(n % 8 for n in sizes)      # value lands on it; ragged layers zero-fill them
    if fault == "drop_k_slice":
        return plan.S > 1 and any(plan.slabs[l] > 1 for l in range(len(sizes)))
    if fault == "slabs_as_S":
        return plan.S > 1 and any(plan.slabs[l] < plan.S for l in range(len(sizes)))
    if fault == "xlo_odd_ksteps":
        return terms >= 2 and any(n > 16 for n in sizes)
    if fault == "alo_blocks_ge4":
        return terms == 3 and bool((plan.segs[:, 3] > 4).any())
    if fault == "terms2_for_3":
        return terms == 3
    if fault == "rho_swap":
        return rows >= 5
    raise KeyError(fault)


def apply(x, A_list, slices, terms, transpose, fault=None, plan=None):
    """(out, sum |p|) in fp64, [rows, D] each.  `fault`: one of FAULTS (those that speak of segments and slices read `plan`)"""
    assert fault is None or fault in FAULTS
    rows, D = x.shape[0], slices[-1][1]
    out = torch.zeros(rows, D, dtype=F64)
    sabs = torch.zeros(rows, D, dtype=F64)
    if fault == "terms2_for_3" and terms == 3:
        terms = 2
    for l, ((a, b), A) in enumerate(zip(slices, A_list)):
        K = b - a
        xs = x[:, a - 1:b - 1] if (fault == "layer_offset" and l > 0) else x[:, a:b]
        xh, xl = split64(xs)
        Ah, Al = split64(A, keep=True)
        if bool(transpose) != (fault == "transposed"):
            Ah, Al = Ah.t(), Al.t()
        kh = torch.ones(K, dtype=F64)               # which contraction indices the hi / lo part of x contributes at
        kl = torch.ones(K, dtype=F64)
        if fault == "drop_partial_chunk" and K % 32:
            kh[K // 32 * 32:] = 0
            kl[K // 32 * 32:] = 0
        if fault == "drop_k_slice" and l == min(i for i in range(len(slices)) if plan.slabs[i] > 1):
            nc, sl = pad32(K) // BK, int(plan.slabs[l])
            kh[32 * (nc // sl):32 * (2 * nc // sl)] = 0          # slab 1 of the layer
            kl[32 * (nc // sl):32 * (2 * nc // sl)] = 0
        if fault == "xlo_odd_ksteps":
            kl[(torch.arange(K) // 16) % 2 == 1] = 0
        o = (xh * kh) @ Ah
        s = (xh * kh).abs() @ Ah.abs()
        if terms >= 2:
            o += (xl * kl) @ Ah
            s += (xl * kl).abs() @ Ah.abs()
        if terms == 3:
            p3 = (xh * kh) @ Al
            if fault == "alo_blocks_ge4":
                for sl_, _, cb0, w, _, _, _, _ in plan.segs.tolist():
                    if sl_ == l and w > 4:
                        p3[:, 32 * (cb0 + 4):32 * (cb0 + w)] = 0
            o += p3
            s += (xh * kh).abs() @ Al.abs()
        if fault == "padding_nonzero" and K % 32 and K % 8 == 0:
            # the chunks beyond the layer repeat its last 16 bytes of x; they meet mapping rows that hold 256 instead of 0
            xf = xh + xl if terms >= 2 else xh
            k = torch.arange(K, pad32(K))
            o += 256.0 * xf[:, K - 4 + k % 4].sum(1, keepdim=True)
        if fault == "slabs_as_S" and plan.slabs[l] < plan.S:
            o += 256.0 * float(plan.S - plan.slabs[l])              # slabs nobody wrote, added all the same
        if fault == "row_beyond_rows" and rows % BM and K % 8:
            o[rows - 1] = 0                                          # a zero-filled row stored over the last one
        out[:, a:b] = o
        sabs[:, a:b] = s
    if fault == "rho_swap" and rows >= 5:
        out[[1, 4]] = out[[4, 1]]                                    # accumulator registers (1, half 0) and (0, half 1)
    return out, sabs


def budget(x, A_list, slices):
    """max over the output elements, both directions, of sum |p| / 256 for the three-term form (the largest of the three)"""
    return max(float(apply(x, A_list, slices, 3, t)[1].max()) / 256.0 for t in (0, 1))


def n_products(K, terms):
    return K * terms


# ---- packed images -----------------------------------------------------------------------------------------------------------------
def packed_images(A_list, want_lo):
    """[forward hi, data-gradient hi, forward lo, data-gradient lo]: one flat bf16 plane each (lo: None unless want_lo); per layer
    a pad32(L) x pad32(L) row-major image, zero-padded, at offset sum pad32^2 of the earlier layers.  The forward image holds A^T
    (row = output column, contraction index contiguous), the data-gradient image A."""
    planes = [[], [], [], []]
    for A in A_list:
        L = A.shape[0]
        Lp = pad32(L)
        hi, lo = split(A)
        for i, m in enumerate((hi.t(), hi, lo.t(), lo)):
            img = torch.zeros(Lp, Lp, dtype=BF)
            img[:L, :L] = m
            planes[i].append(img.reshape(-1))
    flat = [torch.cat(p) for p in planes]
    return flat if want_lo else [flat[0], flat[1], None, None]


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------
def wgrad(h, dw, fault=None):
    """(h^T @ dw, sum |p|) in fp64"""
    assert fault is None or fault in WGRAD_FAULTS
    g = h.to(F64).t() @ dw.to(F64)
    s = h.to(F64).abs().t() @ dw.to(F64).abs()
    L = g.shape[0]
    if fault == "kn_swapped" and L > 32:
        nt = (L + 31) // 32
        p = torch.zeros(nt * 32, nt * 32, dtype=F64)
        p[:L, :L] = g
        g = p.view(nt, 32, nt, 32).transpose(0, 2).reshape(nt * 32, nt * 32)[:L, :L].clone()
    return g, s


def fma32(a, b, c):
    """the correctly rounded fp32 fma of fp32 values held in fp64 tensors: a * b is exact in fp64 (48 bits), the sum with c is
    formed with its TwoSum error and rounded TO ODD in fp64, and the second rounding to fp32 then cannot err (53 >= 2 * 24 + 2)"""
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.contiguous().view(torch.int64) & 1) == 0
    need = (e != 0) & even
    toward = torch.where(e > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    s = torch.where(need, torch.nextafter(s, toward), s)
    return s.to(F32).to(F64)


def _add32(a, b):
    return (a.to(F32) + b.to(F32)).to(F64)


def wgrad_narrow_chain(h, dw, rows, L, n_slabs, fault=None):
    """fp32 [L, L]: wgrad_narrow_kernel + wgrad_narrow_sum_kernel restated.  Rows are cut into n_slabs slabs of
    per = ceil8(ceil(rows / n_slabs)); within a slab wave w takes the row pairs m_begin + 2 w + 64 i + 8 u (i = 0, 1, ..; u = 0..7),
    one fma per row in row order; waves ((w0 + w1) + w2) + w3; slabs in slab order"""
    assert fault is None or fault in WGRAD_FAULTS
    h, dw = h.to(F32).to(F64), dw.to(F32).to(F64)
    per = (rows + n_slabs - 1) // n_slabs
    if fault != "slab_not_rounded8":
        per = (per + 7) // 8 * 8
    total = torch.zeros(L, L, dtype=F64)
    for slab in range(n_slabs):
        m_begin, m_end = slab * per, min(rows, slab * per + per)
        acc = [torch.zeros(L, L, dtype=F64) for _ in range(4)]
        for m in range(m_begin, m_end):
            w = ((m - m_begin) % 8) // 2
            acc[w] = fma32(h[m][:, None].expand(L, L), dw[m][None, :].expand(L, L), acc[w])
        total = _add32(total, _add32(_add32(_add32(acc[0], acc[1]), acc[2]), acc[3]))
    return total.to(F32)
