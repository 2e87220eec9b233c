"""Evaluator of the variational-posterior path (posterior.hip, posterior_bodies.h, the helpers of rcb_common.h), numpy only, written
from the definitions in include/rcb.h and the reference lines they cite.  It uses the FORWARD maps (row_map, row_perm, col_map)
only -- the host-built inverses of ops.LevelSpec (member_ptr / member_idx, row_perm_inv, col_inv) are what it checks -- and takes
nothing from the kernels' loops.

The path is approximated pieces joined by exactly rounded glue.  The glue is fp32 add / mul / sub with contraction off in a
documented order: np.float32 arithmetic, one operation per rounding, reproduces it.  The pieces (st_f32, dst_f32, kl_elem_f32,
Adam's square root and divisions, Philox + Box-Muller) are observed alone through the C ABI ("taps", test_hip_posterior_exact.py),
bounded once against fp64, and their DEVICE values are fed into this evaluator so that composites compare bit for bit.

u = 2^-24 is the unit roundoff.  A correctly rounded operation has relative error <= u, i.e. <= 1/2 ulp; a hardware
transcendental (v_exp, v_log, v_rcp, v_sqrt) is taken to be within 1 ulp of its result, as rcb_common.h takes it, i.e. relative
error <= rel_ulp(y) = ulp(y) / |y| in (u, 2u].

DERIVED BOUNDS (nothing here is measured on the code under test)

ST_ULPS / DST_ULPS   |st_f32(x) - softplus(x)/6| <= ST_ULPS ulp(ref) on [-80, 88.7], same for dst_f32 against sigmoid(x)/6.
  exp_fast: the argument x log2(e) is carried as hi + lo with L + L_lo = log2(e) to 2^-49, so the argument error is below
  1e-6 ulp; e = v_exp(hi): 1 ulp; fma(e, lo ln2, e): 1/2 ulp (the dropped (lo ln2)^2 / 2 < 2^-36).  t = e^x (1 + d_t),
  |d_t| <= 1.5 rel_ulp(e^x).
  st, t < 2^-6 (series): sp = t P(t); P's last fma lands in (0.99, 1]: 1/2 ulp there, the inner roundings arrive multiplied by
  t <= 2^-6 (+ 2^-5 of it), truncation t^5 / 6 < 2^-32 relative; the product t P: 1/2 ulp; log1p's condition number
  k(t) = t / ((1 + t) ln(1 + t)) <= 1 carries d_t.
  st, t >= 2^-6 (general): u = fl(1 + t), c = t - (u - 1) EXACTLY (u - 1 and the difference are representable), ln(1 + t) =
  ln u + c / u - (c / u)^2 / 2 with |c / u| <= 2^-24: the dropped term is < 2^-43 relative.  log_fast(u): v_log 1 ulp of log2 u,
  the constant ln 2 as a float is off by 0.046 u, the product 1/2 ulp; the closing fma 1/2 ulp; k(t) d_t as above.
  x > 20: sp = x exactly.  Division by 6 (quotient by the rounded reciprocal + one exact residual step): 1/2 ulp + 2^-47.
  dst: d = fl(1 + T), T = e^-x (1 + d_t): T / (1 + T) d_t + 1/2 ulp; the reciprocal after its Newton step: 1/2 ulp (the 1 ulp of
  v_rcp enters squared); the division by 6: 1/2 ulp.
  Each "1/2 ulp of y" costs 1/2 rel_ulp(y) / rel_ulp(ref) ulp(ref), between 1/4 and 1, depending on where y and ref sit in
  their binades, and the worst positions do not coincide.  st_ulp_bound(x) / dst_ulp_bound(x) evaluate the sum above at x in fp64
  (taking the worse binade for any y within 1e-5 of a power of two, and the worse branch next to the switch); ST_ULPS and
  DST_ULPS are their suprema, rounded up.  test_posterior_emul_cpu.py evaluates them over a grid of 4e5 points and every float
  next to the switch and asserts the constants cover them.  (With every factor at its own worst the count is 8.02 for st.)

KL_C = 4.001  |kl_elem_f32 - KL| <= KL_C u (ratio^2 + t^2 + 1 + |ln ratio^2|),  ratio = sig_q / sig_p,  t = (mu_q - mu_p) / sig_p.
  The two quotients (reciprocal, product, exact residual, one fma): u each.  var_ratio = fl(ratio^2): 3u; dm = fl(mu_q - mu_p): u of
  the exact difference; t: 2u; t1 = fl(t^2): 5u -- or 4u when the compiler contracts var_ratio + t1 into fma(t, t, var_ratio),
  which it may: kl_elem_f32 is defined before the `contract(off)` pragma.  The sum: u (var_ratio + t1) either way; - 1:
  u (var_ratio + t1 + 1); log_fast(var_ratio) = ln(var_ratio (1 + 3u)) (1 + 3.05u): 3u + 3.05u |ln|; the last subtraction
  u (var_ratio + t1 + 1 + |ln|); the halving is exact.  Sum / 2: u (3 var_ratio + 4 t1 + 2.5 + 2.03 |ln|) <= 4u (...); the .001 of
  KL_C = 4.001 carries the second-order terms (< 1e-6 of the first).

ADAM_C = 4    |p - p64| <= 1/2 ulp(p) + ADAM_C 2^-23 step_size |m / denom|, p64 the fp64 update from the (bit-exact) m and v.
  sq (v_sqrt + residual step, "<= 1 ulp"): 2u; sq / bc2_sqrt ("<= 1 ulp"): 2u; + eps: u -> denom 5u; m / denom: 2u more;
  times step_size: u; total 8u = 4 2^-23 on the step, then the rounding of p + step: 1/2 ulp(p).  PRECONDITION (rcb_common.h):
  |g| >= 1e-15 or g = 0, so that no intermediate (w2 g^2 >= 1e-33) is denormal.

GRAD bound    per element, fp64:  |g - g64| <= u ((K + 2) A + 8 P),  A = (1 - mask) sum |terms| of the gather (K = members x
  samples terms: K - 1 additions, each <= u of the partial sums <= A, one rounding per product d_out eps, one for the closing
  add), P = the KL part with its cancelling pair taken apart, |w| (|loc - p_loc| / sig_p^2) and |w| (sig / sig_p^2 + 1 / sig):
  sig_p^2 u, 1 / . 2u, the product / difference u each, times w u, the closing add u: <= 7u, 8 with the second-order terms.
  g_log_scale = fl(g_sig dst): dst (the tap's value) times the bound of g_sig, + u |g_log_scale|.

KL log        |sum of the slots / 2^24 - KL64| <= sum of the element bounds (KL_C) + W 2^-25 + N 2^-53 sum |k|: every one of the W
  workgroups rounds its fp64 partial sum once to the grid of 2^-24 nats (1/2 unit each); the last term covers the fp64 additions
  themselves, the N - 1 of the kernel's partial sums in whatever order its waves take and those of the reference sum (each
  <= 2^-53 of a partial sum <= sum |k|).  The same N 2^-53 sum |term| is all that separates kl_row from the evaluator's sum of
  the tapped elements.
"""
import math
import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
ST_ULPS = 6.0
DST_ULPS = 5.0
KL_C = 4.001
ADAM_C = 4.0
LDS_LIMIT = 150 * 1024


def f32(x):
    return np.asarray(x, dtype=F32)


def ulp(x):
    """ulp of the fp32 binade that holds |x| (x fp64; normal range)"""
    a = np.abs(np.asarray(x, F64))
    return np.exp2(np.floor(np.log2(np.maximum(a, 2.0 ** -126))) - 23)


# ---- the elementary functions in fp64 ---------------------------------------------------------------------------------------------
def st_ref(x):
    """softplus(x, beta=1, threshold=20) / 6 (prior_model.py:88)"""
    x = np.asarray(x, F64)
    with np.errstate(over="ignore"):
        return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 30.0)))) / 6


def dst_ref(x):
    x = np.asarray(x, F64)
    with np.errstate(over="ignore"):
        return np.where(x > 20, 1.0, 1 / (1 + np.exp(-x))) / 6


def _mant(y):
    y = np.abs(np.asarray(y, F64))
    y = np.where(y > 0, y, 1.0)
    return y / np.exp2(np.floor(np.log2(y)))


def _rel_ulp(y):
    """ulp(y) / |y| in units of u, the worse binade where y is within 1e-5 of the next power of two"""
    m = _mant(y)
    return np.where(m > 2 - 1e-5, 2.0, 2.0 / m)


def _exp_err(x):
    return 1.5 * _rel_ulp(np.exp(x)) + 1e-3


def st_ulp_bound(x):
    """the count of the module docstring at x, in ulp(st_ref(x))"""
    x = np.asarray(x, F64)
    ref = st_ref(x)
    xs = np.minimum(x, 20.0)
    t = np.exp(xs)
    sp = np.log1p(t)
    k = t / ((1 + t) * sp)
    dt = _exp_err(xs)
    ser = k * dt + 0.5 * (1 + 2.0 ** -5) * _rel_ulp(1 - t / 2) + 0.01 + 0.5 * _rel_ulp(sp)
    u_ = 1 + t
    gen = k * dt + (_rel_ulp(np.log2(u_)) + 0.046 + 0.5 * _rel_ulp(np.log(u_))) + 0.5 * _rel_ulp(sp) + 1e-3
    near = np.abs(t - 2.0 ** -6) < 2.0 ** -6 * 1e-4
    rel = np.where(near, np.maximum(ser, gen), np.where(t < 2.0 ** -6, ser, gen))
    rel = np.where(x > 20, 0.0, rel)
    return (rel + 0.5 * _rel_ulp(ref) + 1e-3) * _mant(ref) / 2          # relative error rho u = rho m / 2 ulp(ref)


def dst_ulp_bound(x):
    x = np.asarray(x, F64)
    ref = dst_ref(x)
    T = np.exp(np.minimum(-x, 80.0))
    d = 1 + T
    rel = T / d * _exp_err(np.minimum(-x, 80.0)) + 0.5 * _rel_ulp(d) + 0.5 * _rel_ulp(1 / d) + 1e-3
    rel = np.where(x > 20, 0.0, rel)
    return (rel + 0.5 * _rel_ulp(ref) + 1e-3) * _mant(ref) / 2


def kl_ref(mu_q, sig_q, mu_p, sig_p):
    """KL(N(mu_q, sig_q) || N(mu_p, sig_p)) in fp64 (torch.distributions.kl._kl_normal_normal) and the bound's magnitude"""
    mu_q, sig_q, mu_p, sig_p = (np.asarray(a, F64) for a in (mu_q, sig_q, mu_p, sig_p))
    vr = (sig_q / sig_p) ** 2
    t1 = ((mu_q - mu_p) / sig_p) ** 2
    return 0.5 * (vr + t1 - 1 - np.log(vr)), vr + t1 + 1 + np.abs(np.log(vr))


def kl_bound(mu_q, sig_q, mu_p, sig_p):
    return KL_C * U * kl_ref(mu_q, sig_q, mu_p, sig_p)[1]


# ---- Philox4x32-10 + Box-Muller -------------------------------------------------------------------------------------------------
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 -> 4 uint64 arrays holding 32-bit words"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK32 for v in counter]
    k = [np.uint64(int(v) & 0xFFFFFFFF) for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + np.uint64(W0)) & MASK32, (k[1] + np.uint64(W1)) & MASK32]
    return c


def philox_counter(groups, seed, stream, step, mutant=None):
    """the counter layout of rcb.h / philox_normal4: (group lo, group hi, stream ^ (step >> 32) * 0x85EBCA6B, step lo), key (seed lo,
    seed hi); groups: uint64 array (wraps at 2^64 like the kernel's unsigned sum)"""
    step, seed, stream = int(step) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1), int(stream) & 0xFFFFFFFF
    if mutant == "swap_stream_step":
        stream, step = step & 0xFFFFFFFF, (step & ~0xFFFFFFFF) | stream
    hi = groups >> np.uint64(32)
    if mutant == "drop_group_hi":
        hi = np.zeros_like(hi)
    w2 = stream ^ (((step >> 32) * 0x85EBCA6B) & 0xFFFFFFFF)
    n = groups.shape[0]
    return ([groups & MASK32, hi, np.full(n, w2, np.uint64), np.full(n, step & 0xFFFFFFFF, np.uint64)],
            [seed & 0xFFFFFFFF, seed >> 32])


def philox_normal_ref(n, seed, stream, step, group_offset=0, mutant=None):
    """-> (normals fp64 [n], u1-is-one mask [n]): element i is normal i % 4 of Philox group i / 4 + group_offset.  The four uniforms
    are formed in fp32 as the kernel forms them -- (float)(r >> 8) + 0.5f is not representable above 2^23 and rounds to even, so
    u1 can be exactly 1 and the normal exactly 0 -- and Box-Muller is taken in fp64."""
    n4 = (n + 3) // 4
    groups = (np.arange(n4, dtype=np.uint64) + np.uint64(int(group_offset) & (2 ** 64 - 1)))      # wraps
    ctr, key = philox_counter(groups, seed, stream, step, mutant)
    r = philox4x32_10(ctr, key)
    K = F32(1.0 / 16777216.0)
    top = [(v >> np.uint64(8)).astype(np.int64).astype(F32) for v in r]
    u1, u2, u3, u4 = (top[0] + F32(0.5)) * K, top[1] * K, (top[2] + F32(0.5)) * K, top[3] * K
    ra, rb = np.sqrt(-2 * np.log(u1.astype(F64))), np.sqrt(-2 * np.log(u3.astype(F64)))
    a2, a4 = 2 * np.pi * u2.astype(F64), 2 * np.pi * u4.astype(F64)
    out = np.stack([ra * np.cos(a2), ra * np.sin(a2), rb * np.cos(a4), rb * np.sin(a4)], 1).reshape(-1)[:n]
    one = np.stack([u1 == 1, u1 == 1, u3 == 1, u3 == 1], 1).reshape(-1)[:n]
    return out, one


# ---- cases ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Lv:
    rows: int
    cols: int
    cols_out: int
    counts: tuple = None          # members per source row (an unsorted, interleaved row map); None: one row per INR
    row_perm: bool = False        # oracle.ref_cpu.column_row_perms
    col_map: bool = False         # a permutation (cols_out == cols) or an injective map into the columns
    mask: bool = False            # encode mask + sample
    sigma: bool = False           # scale_is_sigma
    bwd: tuple = ()               # kernels the update of this level is meant to reach: (Adam, want_grads)


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    S: int
    levels: tuple
    fwd: str                      # kernel the sampler is meant to reach (default dispatch)
    beta: bool = False            # per-group beta (and kl_scalar_dev) in the update
    update: bool = True           # run the update tests on it (the large sampler-only cases do not)


COUNTS42 = (0, 1, 7, 8, 9, 17)
COUNTS44 = (0, 1, 7, 8, 11, 17)
D = 1029        # 4 * 257 + 1: rows only 4-byte aligned; one past 1024: a second trip of the 1024-strided loops
GEN, BYD, SUMS = "posterior_bwd", "posterior_bwd+by_d", "sample_sums+posterior_bwd"
M64, M256, FLAT, STG = "posterior_members4<64>", "posterior_members4<256>", "posterior_flat", "posterior_staged"


def _tt(rows, cols_out, counts=None, cols=D, bwd=()):
    return Lv(rows, cols, cols_out, counts, row_perm=True, col_map=True, mask=True, bwd=bwd)


CASES = (
    Case("flat4", 4, 1, (Lv(4, D, D, bwd=(FLAT, GEN)),), "reparam_flat"),
    Case("flat5", 5, 1, (Lv(5, D, D, bwd=(GEN, GEN)),), "reparam_flat"),
    Case("tiny7", 3, 1, (Lv(3, 7, 7, bwd=(GEN, GEN)),), "reparam_flat"),
    Case("sigma", 5, 2, (Lv(5, D, D, sigma=True, bwd=()),), "reparam_fwd", update=False),
    Case("members42", 42, 1, (Lv(6, D, D, COUNTS42, bwd=(M64, GEN)),), "reparam_fwd"),
    Case("members1024", 1024, 1, (Lv(512, D, D, (1, 3) * 256, bwd=(M256, GEN)),), "reparam_fwd"),
    Case("hier2", 44, 1, (Lv(44, D, D, bwd=(FLAT, GEN)), Lv(6, D, D, COUNTS44, bwd=(M64, GEN))), "reparam_hier_flat"),
    Case("hier3", 44, 1, (Lv(44, D, D, bwd=(FLAT, GEN)), Lv(6, D, D, COUNTS44, bwd=(M64, GEN)), Lv(2, D, D, (0, 44), bwd=(M64, GEN))),
         "reparam_hier_flat"),
    Case("hier3_n42", 42, 1, (Lv(42, D, D, bwd=(GEN, GEN)), Lv(6, D, D, COUNTS42, bwd=(M64, GEN)), Lv(2, D, D, (0, 42), bwd=(M64, GEN))),
         "reparam_fwd"),
    Case("staged3840", 2, 5, (Lv(2, 3840, 3840, col_map=True, mask=True, bwd=(STG, STG)),), "reparam_staged", beta=True),
    Case("staged3841", 2, 5, (Lv(2, 3841, 3841, col_map=True, mask=True, bwd=(SUMS, SUMS)),), "reparam_staged", beta=True),
    Case("staged_out901", 6, 5, (Lv(6, D, 901, col_map=True, mask=True, bwd=(STG, STG)),), "reparam_staged", beta=True),
    Case("testtime_l1", 6, 5, (_tt(6, D, bwd=(SUMS, SUMS)),), "reparam_fwd+packed", beta=True),
    Case("testtime_l1_out901", 6, 5, (_tt(6, 901, bwd=(SUMS, SUMS)),), "reparam_fwd+packed", beta=True),
    Case("testtime_l1_s1", 6, 1, (_tt(6, D, bwd=(GEN, GEN)),), "reparam_fwd", beta=True),
    Case("testtime_coarse", 42, 5, (_tt(6, D, COUNTS42, bwd=(BYD, BYD)),), "reparam_fwd+packed", beta=True),
    Case("testtime_coarse_out901", 42, 5, (_tt(6, 901, COUNTS42, bwd=(GEN, GEN)),), "reparam_fwd+packed", beta=True),
    Case("testtime3", 42, 5, (_tt(42, D, bwd=(SUMS, SUMS)), _tt(6, 901, COUNTS42, bwd=(GEN, GEN)),
                              Lv(2, D, 901, (0, 42), col_map=True, mask=True, bwd=(GEN, GEN))), "reparam_fwd+packed", beta=True),
    Case("testtime7", 42, 5, (_tt(6, 7, COUNTS42, cols=7, bwd=(BYD, BYD)),), "reparam_fwd+packed", beta=True),
    Case("restaged9600", 2, 2, (Lv(2, 9600, 9600, col_map=True, bwd=()),), "reparam_staged", update=False),
    Case("restaged9601", 2, 2, (Lv(2, 9601, 9601, col_map=True, bwd=()),), "reparam_fwd", update=False),
)
CASE = {c.name: c for c in CASES}


def case_id(c):
    return c.name


def cdiv(a, b):
    return -(-a // b)


def fwd_reached(case, generic=False):
    """the sampler's dispatch as rcb.h and the comments above each kernel give it (ops.reparam_fwd hands the packing scratch to
    gathered levels when n * S >= 8 and the one-level staged kernel does not apply)"""
    L = case.levels
    L0, n, S, out_cols = L[0], case.n, case.S, L[0].cols_out
    plain = lambda v: not (v.mask or v.row_perm or v.col_map or v.sigma)              # noqa: E731
    staged = (len(L) == 1 and not L0.sigma and L0.col_map and L0.counts is None and not L0.row_perm and L0.rows == n
              and L0.cols * 16 <= LDS_LIMIT)
    if not generic:
        if len(L) == 1 and S == 1 and plain(L0) and L0.counts is None and L0.cols == out_cols and L0.rows == n:
            return "reparam_flat"
        if staged:
            return "reparam_staged"
        if (len(L) >= 2 and S == 1 and (n * out_cols) % 4 == 0 and L0.counts is None and L0.rows == n
                and all(plain(v) and v.cols == out_cols == v.cols_out for v in L)):
            return "reparam_hier_flat"
        if any(v.col_map or v.row_perm for v in L) and n * S >= 8:
            return "reparam_fwd+packed"
    return "reparam_fwd"


def bwd_reached(case, li, adam, want_grads, generic=False):
    """rcb_posterior_bwd's dispatch for level li of the case, in the order of the C entry point"""
    v, S, beta = case.levels[li], case.S, case.beta
    members = v.counts is not None
    if not generic:
        if v.col_map and not members and not v.row_perm and S * v.cols_out * 8 <= LDS_LIMIT:
            return STG
        simple = adam and S == 1 and v.cols_out == v.cols and not v.mask and not beta and not v.row_perm and not v.col_map and not want_grads
        if simple and not members and (v.rows * v.cols) % 4 == 0:
            return FLAT
        if simple and members:
            return M256 if v.rows * cdiv(v.cols, 1024) >= 1024 else M64
        if not members and S >= 2 and v.col_map and v.rows == case.n:
            return SUMS
        if v.col_map and members and v.cols_out == v.cols:
            return BYD
    return GEN


def kernel_reached(case, generic=False):
    """-> {"fwd": sampler kernel, "bwd": per level (with Adam, with gradient outputs)}: what the case table claims, restated"""
    return {"fwd": fwd_reached(case, generic),
            "bwd": tuple((bwd_reached(case, li, True, False, generic), bwd_reached(case, li, False, True, generic)) for li in range(len(case.levels)))}


def kl_workgroups(kernel, v):
    """workgroups that add one rounded partial sum each to the KL slots"""
    if kernel == FLAT:
        return cdiv(v.rows * v.cols // 4, 256)
    if kernel == STG:
        return v.rows
    if kernel == M256:
        return v.rows * cdiv(v.cols, 1024)
    return v.rows * cdiv(v.cols, 256)


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def row_map_of(counts, key):
    rm = np.repeat(np.arange(len(counts)), counts)
    return _rng("row_map", key).permutation(rm).astype(np.int64)


def groups_of(cols, key):
    """-> (group_idx [cols] ascending, seg_start, seg_end): G = 37 groups of uneven length (3 for 7 columns), the first of one column"""
    G = 37 if cols >= 100 else 3
    cuts = np.sort(_rng("groups", key).choice(np.arange(2, cols), G - 2, replace=False))
    start = np.r_[0, 1, cuts]
    end = np.r_[start[1:], cols]
    return np.repeat(np.arange(G), end - start).astype(np.int64), start.astype(np.int64), end.astype(np.int64)


def level_data(case, li, lattice=False, column_row_perms=None):
    """the arrays of level li (numpy; the sigma / dst / prior-sigma taps are filled in by the caller: .sig, .dst, .sp)"""
    v = case.levels[li]
    r = _rng(case.name, li)
    L = SimpleNamespace(spec=v, rows=v.rows, cols=v.cols, cols_out=v.cols_out, n=case.n, S=case.S, scale_is_sigma=v.sigma)
    L.loc = f32(0.02 * r.randn(v.rows, v.cols))
    L.ls = f32(-4 + 0.5 * r.randn(v.rows, v.cols))
    if v.sigma:
        L.ls = f32(0.003 + 0.002 * r.rand(v.rows, v.cols))
    L.row_map = row_map_of(v.counts, (case.name, li)) if v.counts is not None else None
    assert (L.row_map is None and v.rows == case.n) or (L.row_map is not None and len(L.row_map) == case.n)
    L.row_perm = None
    if v.row_perm:
        L.row_perm = column_row_perms(v.rows, v.cols) if column_row_perms else np.stack(
            [_rng("rp", c).permutation(v.rows) for c in range(v.cols)], 1)
    L.col_map = r.permutation(v.cols)[:v.cols_out].astype(np.int64) if v.col_map else None
    L.group_idx, L.seg_start, L.seg_end = groups_of(v.cols, (case.name, li))
    G = len(L.seg_start)
    L.beta = f32(r.rand(v.rows, G) * 1e-3)
    L.beta[r.rand(v.rows, G) < 0.15] = 0
    L.beta[:, 2] = 0                                   # group 2: encoded everywhere, beta 0
    L.mask = L.z = None
    if v.mask:
        L.mask = f32(r.rand(v.rows, v.cols) < 0.3)
        L.mask[:, L.group_idx == 2] = 1
        L.z = f32(0.02 * r.randn(v.rows, v.cols))
    L.p_loc = f32(0.01 * r.randn(v.cols))
    L.p_ls = f32(-3 + 0.2 * r.randn(v.cols))
    shape = (case.n, case.S, v.cols_out)
    if lattice:                                        # d_out in k 2^-10, |k| <= 64;  eps in k 2^-6, |k| <= 255
        L.d_out = f32(r.randint(-64, 65, shape) * 2.0 ** -10)
        L.eps = f32(r.randint(-255, 256, shape) * 2.0 ** -6)
    else:
        L.d_out = f32(1e-3 * r.randn(*shape))
        L.eps = f32(r.randn(*shape))
    return L


def lattice_headroom(L):
    """max over the source elements of sum |term| / grid for the two gathered sums: below 2^24 every fp32 partial sum is exact"""
    a_mu, a_sig = gather64(L, np.abs(L.d_out.astype(F64)) * 2.0 ** 10, np.abs(L.d_out.astype(F64) * L.eps.astype(F64)) * 2.0 ** 16)
    return float(a_mu.max()), float(a_sig.max())


# ---- the sampler ----------------------------------------------------------------------------------------------------------------
def source(L, mutant=None):
    """-> (r [n, cols_out], j [cols_out]): the source element of (n, d) by the forward maps (rcb.h, rcb_level)"""
    d = np.arange(L.cols_out)
    j = L.col_map[d] if L.col_map is not None else d
    if mutant == "col_map_truncated" and L.col_map is not None:
        j = np.argsort(np.argsort(L.col_map))                     # a permutation of cols_out
    r0 = L.row_map if L.row_map is not None else np.arange(L.n)
    r = np.broadcast_to(r0[:, None], (L.n, L.cols_out))
    if L.row_perm is not None:
        rp = L.row_perm
        if mutant == "row_perm_not_inverted":
            rp = np.argsort(rp, axis=0)
        r = rp[r0[:, None], j[None, :]]
    return r, j


def mu_sigma(L):
    """effective (mu, sigma) of every parameter element in fp32: loc (1 - m) + z m, sigma (1 - m) + 1e-15 m (test_model.py:289-290)"""
    mu, sg = L.loc, (L.ls if L.scale_is_sigma else L.sig)
    if L.mask is not None:
        keep = F32(1) - L.mask
        mu = mu * keep + L.z * L.mask
        sg = sg * keep + F32(1e-15) * L.mask
    return f32(mu), f32(sg)


def sample(levels, mutant=None):
    """out[n, s, d] = sum over the levels of mu + sigma eps, fp32: per level add(mu, mul(sigma, eps)), levels added in ascending
    order; a level contributes to d < cols_out only"""
    out = None
    for L in levels:
        r, j = source(L)
        mu, sg = mu_sigma(L)
        v = f32(mu[r, j][:, None, :] + f32(sg[r, j][:, None, :] * L.eps))
        if out is None:
            out = v.copy()
            continue
        out[..., :L.cols_out] = out[..., :L.cols_out] + v
        if mutant == "beyond_cols_out" and L.cols_out < out.shape[-1]:
            d = np.arange(L.cols_out, out.shape[-1])
            out[..., L.cols_out:] = out[..., L.cols_out:] + mu[(L.row_map if L.row_map is not None else np.arange(L.n))[:, None], d[None, :]][:, None, :]
    return out


# ---- the gradient gather --------------------------------------------------------------------------------------------------------
def _scatter(L, a, b, dtype, mutant=None):
    """sum a[n, s, d] and b[n, s, d] onto the source elements: n ascending (members of a source row in ascending INR index), then s
    ascending, one rounding per addition in `dtype`"""
    r, j = source(L, mutant if mutant in ("row_perm_not_inverted", "col_map_truncated") else None)
    jj = np.broadcast_to(j[None, :], r.shape)
    ga, gb = np.zeros((L.rows, L.cols), dtype), np.zeros((L.rows, L.cols), dtype)
    order = range(L.n - 1, -1, -1) if mutant == "members_reversed" else range(L.n)
    first = True
    for n in order:
        for s in range(L.S):
            ga[r[n], jj[n]] = ga[r[n], jj[n]] + a[n, s]
            gb[r[n], jj[n]] = gb[r[n], jj[n]] + b[n, s]
            if mutant == "mask_early" and first and L.mask is not None:
                ga, gb = ga * (1 - L.mask).astype(dtype), gb * (1 - L.mask).astype(dtype)
            first = False
    return ga, gb


def gather32(L, mutant=None):
    """(g_mu, g_sig) of the gather in the fp32 chain, times 1 - mask"""
    ga, gb = _scatter(L, L.d_out, f32(L.d_out * L.eps), F32, mutant)
    if L.mask is not None and mutant != "mask_early":
        keep = F32(1) - L.mask
        ga, gb = ga * keep, gb * keep
    return f32(ga), f32(gb)


def gather64(L, a=None, b=None):
    a = L.d_out.astype(F64) if a is None else a
    b = L.d_out.astype(F64) * L.eps.astype(F64) if b is None else b
    ga, gb = _scatter(L, a, b, F64)
    if L.mask is not None:
        ga, gb = ga * (1 - L.mask), gb * (1 - L.mask)
    return ga, gb


def kl_weight(L, kl_scalar, kl_scalar_dev=None, use_beta=False, mutant=None):
    """w[r, j] = kl_scalar * [kl_scalar_dev] * [beta[r, group_idx[j]]], multiplied in fp32 in that order"""
    w = F32(kl_scalar)
    if kl_scalar_dev is not None:
        w = F32(w * F32(kl_scalar_dev))
    w = np.full((L.rows, L.cols), w, F32)
    if use_beta:
        gi = L.group_idx
        if mutant == "beta_at_d" and L.col_map is not None:
            inv = np.zeros(L.cols, np.int64)
            inv[L.col_map] = np.arange(L.cols_out)
            gi = L.group_idx[np.minimum(inv, L.cols - 1)]
        w = f32(w * L.beta[:, gi])
    return w


def grads64(L, w, sig, sp):
    """fp64 gradients from the definition (the adjoint of the sampler + w dKL) and the magnitudes of the bound: -> g_mu, g_sig,
    bound_mu, bound_sig.  sig / sp: the sigmas the kernel used (the taps' values), fp32"""
    g_mu, g_sig = gather64(L)
    a_mu, a_sig = gather64(L, np.abs(L.d_out.astype(F64)), np.abs(L.d_out.astype(F64) * L.eps.astype(F64)))
    K = L.S * (np.bincount(L.row_map, minlength=L.rows).max() if L.row_map is not None else 1)
    w, sig, sp, loc = w.astype(F64), sig.astype(F64), sp.astype(F64)[None, :], L.loc.astype(F64)
    k_mu = w * (loc - L.p_loc.astype(F64)[None, :]) / sp ** 2
    k_sig = w * (sig / sp ** 2 - 1 / sig)
    p_mu, p_sig = np.abs(k_mu), np.abs(w) * (sig / sp ** 2 + 1 / sig)
    return g_mu + k_mu, g_sig + k_sig, U * ((K + 2) * a_mu + 8 * p_mu), U * ((K + 2) * a_sig + 8 * p_sig)


# ---- Adam -----------------------------------------------------------------------------------------------------------------------
def adam_scalars(lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    """make_adam: double arithmetic from the FLOAT lr, beta1, beta2, rounded to float"""
    lr, b1, b2 = float(F32(lr)), float(F32(beta1)), float(F32(beta2))
    return SimpleNamespace(w1=F32(1.0 - b1), beta2=F32(beta2), w2=F32(1.0 - b2), step_size=F32(lr / (1.0 - b1 ** step)),
                           bc2_sqrt=F32(np.sqrt(1.0 - b2 ** step)), eps=F32(eps))


def adam(p, g, m, v, s):
    """-> (m', v' as fp32 chains: m + w1 (g - m), v beta2 + (w2 g) g; p' in fp64 from those; the bound on |p' - kernel|)"""
    p, g, m, v = f32(p), f32(g), f32(m), f32(v)
    m2 = f32(m + f32(s.w1 * f32(g - m)))
    v2 = f32(f32(v * s.beta2) + f32(f32(s.w2 * g) * g))
    denom = np.sqrt(v2.astype(F64)) / float(s.bc2_sqrt) + float(s.eps)
    stepv = float(s.step_size) * m2.astype(F64) / denom
    p2 = p.astype(F64) - stepv
    bound = 0.5 * ulp(np.abs(p2) + ADAM_C * 2.0 ** -23 * np.abs(stepv)) + ADAM_C * 2.0 ** -23 * np.abs(stepv)
    return m2, v2, p2, bound


# ---- KL sums, annealing, fixed point --------------------------------------------------------------------------------------------
def kl_rows(k32, beta=None, group_idx=None, seg=None):
    """kl_rows_kernel's two forms on the elements k32 [rows, cols] (fp32).  Without segments: each fl32(k beta) summed (fp64, any
    order: the caller bounds it).  With segments: sum over g of fp64 beta_g * (ascending fp64 sum over the group) -> rows, groups"""
    if seg is None:
        k = k32 if beta is None else f32(k32 * beta[:, group_idx])
        return k.astype(F64).sum(1), None
    start, end = seg
    groups = np.zeros((k32.shape[0], len(start)), F64)
    for g_, (a, b) in enumerate(zip(start, end)):
        acc = np.zeros(k32.shape[0], F64)
        for j in range(a, b):
            acc = acc + k32[:, j].astype(F64)
        groups[:, g_] = acc
    wts = np.ones_like(groups) if beta is None else beta.astype(F64)
    return (wts * groups).sum(1), groups


def beta_update(kl, beta, done, bits=16.0, upper=0.0, lower=0.4, step=0.05):
    """test_model.py:404-413 as rcb.h restates it: strict > and <=, clamp [0, 1e4], done keeps"""
    b = kl.astype(F64) / 0.6931471805599453
    f = F32(1.0 + step)
    nb = f32(beta * np.where(b > bits + upper, f, F32(1)))
    nb = f32(nb / np.where(b <= bits - lower, f, F32(1)))
    nb = np.minimum(np.maximum(nb, F32(0)), F32(10000))
    return np.where(done.astype(bool), beta, nb).astype(F32)


def _fx_split(v):
    """one term as Python integers: hi = floor(v 2^30), lo = rint((v 2^30 - hi) 2^32); |v| < 4096 else counted"""
    if not (abs(v) < 4096.0):
        return 0, 0, 1
    s = v * 2.0 ** 30
    f = math.floor(s)
    return f, round((s - f) * 2.0 ** 32), 0                # (round: half to even, as rint)


def col_moments_fx(loc, sig):
    """rcb_col_moments: [3][2][cols] (hi, lo) sums of x, x^2 (fp64 from the fp32 x) and fl32(sigma sigma), + the count"""
    rows, cols = loc.shape
    out = [0] * (6 * cols + 1)
    s2 = f32(sig * sig)
    for r in range(rows):
        for j in range(cols):
            x = float(loc[r, j])
            for q, v in enumerate((x, x * x, float(s2[r, j]))):
                hi, lo, bad = _fx_split(v)
                out[(2 * q) * cols + j] += hi
                out[(2 * q + 1) * cols + j] += lo
                out[6 * cols] += bad
    return out


def kl_colsum_fx(k64):
    """sum over rows of rint(k 2^30) as Python integers, elements with |k| >= 4096 / NaN counted"""
    ok = np.abs(k64) < 4096.0
    q = np.rint(np.where(ok, k64, 0.0) * 2.0 ** 30)
    return [int(v) for v in q.astype(np.int64).sum(0)] + [int((~ok).sum())]
