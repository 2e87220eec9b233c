"""CPU evaluator of the A* scorers of recombiner_amd/csrc/rec_score.hip (numpy fp64, fractions, torch for the host logf).

What it restates, operation for operation, with every rounding where the kernels round:

  constants     the seven per-element constants of rec_prep_kernel: mq, mp, sp widened from fp32; 2 * (s * s) formed in fp32 and
                then widened; log(s) taken in fp32 and then widened.  The fp32 logs are an INPUT (lq, lp): host and device logf
                differ by an ulp here and there, so the GPU tests recover the device's values (test_hip_rec_exact.py, 3a) and
                hand them in; the default is torch.log on the fp32 host tensor, which is what the oracle uses.
  exact_scores  all K log-weights in the order of rec_exact_kernel: z = mp + sp * x with separate multiply and add, true
                division by 2 var, the j == 0 start of the two sums, (lq - lp) + gumbel.  Vectorised over K.
  fast_scores   the quadratic form of rec_prep_kernel + rec_fast_kernel: rq = 1 / v2q, c1 = ((-2 dmq) sp) rq, c2 = sp2 rp - sp2 rq,
                nothing fused; c0 and S summed per lane at stride 64 and then through the xor butterfly of wave_sum (offsets
                32 .. 1); acc = fma(c1, x, fma(c2, x * x, acc)) over ascending j with the FMA exact through Fraction;
                (acc + c0) + gumbel.  One Python-level rational FMA per (candidate, element, term): SMALL K ONLY (K * g of a
                few ten thousand per job), or a handful of candidates through `cand`.
  true_scores   the same formula on the same constants in rational arithmetic (Fraction), no rounding at all.
  tau           the certification threshold 4 (3 g + 28) u (S + G) of rec_prep_kernel, and S + G.
  argmax_first  the reference's rule (torch.argmax): the first of equal values wins, a NaN counts as largest.
  decide        the decision rule of rec_finish_kernel + the arbiter launch: the fast arg-max if its top-2 gap exceeds tau,
                the exact arg-max otherwise.

Builders: random problems (the generator of test_hip_kernels._rec_problem), candidate tables of fp32-precision normals for any
K, a Gumbel table for any K, tie placements (identical table rows and Gumbel values, put above all others), tuned near-ties
(one Gumbel value set so that the TRUE scores of a pair differ by less than half an ulp of it), and the adversarial parameter
families of the certificate test."""
from fractions import Fraction

import numpy as np
import torch

F32, F64 = np.float32, np.float64
LOG_SQRT_2PI = 0.91893853320467267      # kLogSqrt2Pi
U = 1.1102230246251565e-16              # 2^-53
SPAN, THREADS = 1024, 256                # candidates per workgroup of the fast scorer, threads per workgroup
FIELDS = ("mq", "mp", "sp", "v2q", "v2p", "lq", "lp")


def f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=F32))


def host_logf(s):
    return torch.log(torch.from_numpy(f32(s))).numpy()


class Consts:
    """mq, mp, sp, v2q, v2p, lq, lp: fp64 [g] (one job), or [n, g] for fast_coefs / tau of n jobs of one length at once"""

    def __init__(self, **kw):
        for k in FIELDS:
            setattr(self, k, np.asarray(kw[k], dtype=F64))
        self.g = int(self.mq.shape[-1])


def constants(loc, scale, p_loc, p_scale, lq=None, lp=None):
    loc, scale, p_loc, p_scale = (f32(v) for v in (loc, scale, p_loc, p_scale))
    two = F32(2.0)
    lq = host_logf(scale) if lq is None else f32(lq)
    lp = host_logf(p_scale) if lp is None else f32(lp)
    with np.errstate(all="ignore"):
        return Consts(mq=loc, mp=p_loc, sp=p_scale, v2q=two * (scale * scale), v2p=two * (p_scale * p_scale), lq=lq, lp=lp)


def exact_terms(c, xi):
    """the per-element log-densities of rec_exact_kernel, fp64 [K, g] each: (log N_q, log N_p)"""
    xi = np.asarray(xi, dtype=F64)
    with np.errstate(all="ignore"):
        z = c.mp[None] + c.sp[None] * xi
        dq = z - c.mq[None]
        dp = z - c.mp[None]
        tq = ((-(dq * dq)) / c.v2q[None] - c.lq[None]) - LOG_SQRT_2PI
        tp = ((-(dp * dp)) / c.v2p[None] - c.lp[None]) - LOG_SQRT_2PI
    return tq, tp


def exact_scores(c, xi, gumbel):
    """xi: fp64 [K, g] (fp32-precision values), gumbel: fp64 [K] -> fp64 [K]; the two sums run over ascending j from term 0"""
    tq, tp = exact_terms(c, xi)
    sq, sp_ = tq[:, 0], tp[:, 0]
    with np.errstate(all="ignore"):
        for j in range(1, c.g):
            sq = sq + tq[:, j]
            sp_ = sp_ + tp[:, j]
        return (sq - sp_) + np.asarray(gumbel, dtype=F64)


def wave_sum(terms):
    """terms [..., g] -> per-lane sums at stride 64 from 0.0 in ascending j, then the xor butterfly 32 .. 1 (every lane ends
    with the same value)"""
    terms = np.asarray(terms, dtype=F64)
    v = np.zeros(terms.shape[:-1] + (64,), dtype=F64)
    with np.errstate(all="ignore"):
        for j in range(terms.shape[-1]):
            v[..., j % 64] = v[..., j % 64] + terms[..., j]
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[..., lanes ^ off]
    return v[..., 0]


def fast_coefs(c, X):
    """-> c1 [g], c2 [g], c0, S as rec_prep_kernel forms them; X = max |xi| of the job's table"""
    with np.errstate(all="ignore"):
        rq, rp = 1.0 / c.v2q, 1.0 / c.v2p
        dmq = c.mp - c.mq
        sp2 = c.sp * c.sp
        c1 = ((-2.0 * dmq) * c.sp) * rq
        c2 = sp2 * rp - sp2 * rq
        t0 = ((-(dmq * dmq)) * rq - c.lq) + c.lp
        aq = (np.abs(c.mp) + np.abs(c.mq)) + c.sp * X
        ap = 2.0 * np.abs(c.mp) + c.sp * X
        ts = (((((aq * aq) * rq + np.abs(c.lq)) + LOG_SQRT_2PI) + (ap * ap) * rp) + np.abs(c.lp)) + LOG_SQRT_2PI
    return c1, c2, wave_sum(t0), wave_sum(ts)


def tau(c, X, gumbel_absmax):
    """-> (tau, S + G)"""
    S = fast_coefs(c, X)[3]
    S = float(S) if np.ndim(S) == 0 else S
    return 4.0 * (3.0 * c.g + 28.0) * U * (S + gumbel_absmax), S + gumbel_absmax


def fma(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(F64(a) * F64(b) + F64(c))
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fast_scores(c, xi, gumbel, X, cand=None):
    """fp64 [len(cand)] (all K candidates when cand is None).  Rational FMAs: small K, or a few candidates, only."""
    c1, c2, c0, _ = fast_coefs(c, X)
    c0 = float(c0)
    cand = range(xi.shape[0]) if cand is None else cand
    out = []
    finite = bool(np.isfinite(c1).all() and np.isfinite(c2).all())
    f1 = [Fraction(float(v)) for v in c1] if finite else None
    f2 = [Fraction(float(v)) for v in c2] if finite else None
    for k in cand:
        acc = 0.0
        for j in range(c.g):
            x = float(xi[k, j])
            x2 = x * x
            if finite:
                acc = float(f1[j] * Fraction(x) + Fraction(float(f2[j] * Fraction(x2) + Fraction(acc))))
            else:
                acc = fma(float(c1[j]), x, fma(float(c2[j]), x2, acc))
        with np.errstate(all="ignore"):
            out.append((F64(acc) + F64(c0)) + F64(gumbel[k]))
    return np.asarray(out, dtype=F64)


def true_scores(c, xi, gumbel=None, cand=None):
    """list of Fraction: sum_j logN_q - sum_j logN_p (+ gumbel) on the constants of `c`, exactly"""
    fc = {k: [Fraction(float(v)) for v in getattr(c, k)] for k in FIELDS}
    C = Fraction(LOG_SQRT_2PI)
    cand = range(xi.shape[0]) if cand is None else cand
    out = []
    for k in cand:
        s = Fraction(0)
        for j in range(c.g):
            z = fc["mp"][j] + fc["sp"][j] * Fraction(float(xi[k, j]))
            dq, dp = z - fc["mq"][j], z - fc["mp"][j]
            s += (-(dq * dq) / fc["v2q"][j] - fc["lq"][j] - C) - (-(dp * dp) / fc["v2p"][j] - fc["lp"][j] - C)
        out.append(s if gumbel is None else s + Fraction(float(gumbel[k])))
    return out


def argmax_first(v):
    v = np.asarray(v)
    nan = np.isnan(v)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(v))              # numpy: the first occurrence of the maximum


def argmax_last(v):
    """the wrong rule the tie placements must be able to see"""
    v = np.asarray(v)
    return int(len(v) - 1 - np.argmax(v[::-1]))


def top2(v):
    """(best, runner-up, first index of the best); the runner-up of a tie is the best itself, of one candidate -inf"""
    v = np.asarray(v, dtype=F64)
    i = argmax_first(v)
    rest = np.delete(v, i)
    return float(v[i]), (float(rest.max()) if rest.size else -np.inf), i


def decide(fast, exact, tau_):
    """-> (index, uncertified): rec_finish_kernel's certificate and the arbiter"""
    v1, v2, i = top2(fast)
    if (v1 - v2) > tau_:
        return i, 0
    return argmax_first(exact), 1


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def gumbel_table(seed, K):
    """a decreasing truncated-Gumbel sequence, fp64 [K]"""
    log_u = np.log(np.random.RandomState(seed).rand(K))
    out = np.empty(K, dtype=F64)
    b = -np.log(-log_u[0])
    out[0] = b
    for i in range(1, K):
        b = -np.log(-log_u[i] + np.exp(-b))
        out[i] = b
    return out


def normal_table(seed, K, g, clamp=0):
    """fp64 [K, g] of fp32-precision standard normals; `clamp` entries set to +-100, the clamp of the reference's tables"""
    rs = np.random.RandomState(seed)
    t = rs.standard_normal((K, g)).astype(F32).astype(F64)
    for n in range(clamp):
        t[rs.randint(K), rs.randint(g)] = 100.0 if n % 2 else -100.0
    return t


def random_problem(seed, N, D, lens_pool, n_jobs, ratio):
    """the generator of test_hip_kernels._rec_problem: posterior-to-prior scale ratio around `ratio`; fp32 numpy arrays"""
    gen = torch.Generator().manual_seed(seed)
    pl = 0.01 * torch.randn(D, generator=gen)
    ps = 0.015 + 0.01 * torch.rand(D, generator=gen)
    loc = pl[None] + ps[None] * 1.5 * torch.randn(N, D, generator=gen)
    scale = ps[None] * ratio * (0.5 + torch.rand(N, D, generator=gen))
    rs = np.random.RandomState(seed)
    jr = rs.randint(N, size=n_jobs)
    jg = np.asarray(lens_pool)[rs.randint(len(lens_pool), size=n_jobs)]
    js = np.array([rs.randint(D - gl + 1) for gl in jg])
    return loc.numpy(), scale.numpy(), pl.numpy(), ps.numpy(), jr, js, jg


class Call:
    """one rec_score call: parameters fp32 [N, D] / [D], tables {g: fp64 [K, g]}, gumbel fp64 [K], jobs (row, start, glen)"""

    def __init__(self, loc, scale, pl, ps, tables, gumbel, jr, js, jg):
        self.loc, self.scale, self.pl, self.ps = f32(loc), f32(scale), f32(pl), f32(ps)
        self.tables = {int(g): np.array(t, dtype=F64) for g, t in tables.items()}
        self.gumbel = np.array(gumbel, dtype=F64)
        self.jr, self.js, self.jg = (np.asarray(v, dtype=np.int64) for v in (jr, js, jg))
        self.K = int(self.gumbel.shape[0])
        self.n = int(self.jr.shape[0])

    def consts(self, b, logf=None):
        r, s, g = int(self.jr[b]), int(self.js[b]), int(self.jg[b])
        sc, psc = self.scale[r, s:s + g], self.ps[s:s + g]
        lq, lp = (None, None) if logf is None else (logf(sc), logf(psc))
        return constants(self.loc[r, s:s + g], sc, self.pl[s:s + g], psc, lq, lp)

    def xi(self, b):
        return self.tables[int(self.jg[b])]

    def X(self, b):
        return float(np.abs(self.xi(b)).max())

    def gabs(self):
        return float(np.abs(self.gumbel).max())

    def exact(self, b, logf=None):
        return exact_scores(self.consts(b, logf), self.xi(b), self.gumbel)

    def fast(self, b, logf=None, cand=None):
        return fast_scores(self.consts(b, logf), self.xi(b), self.gumbel, self.X(b), cand)

    def tau(self, b, logf=None):
        return tau(self.consts(b, logf), self.X(b), self.gabs())[0]

    def sink(self, ks):
        """put the candidates `ks` above all others in every job of the call by lowering the others' Gumbel values: the scores
        of `ks` keep their magnitude, so their rounding errors stay those of an ordinary job"""
        ks = list(ks)
        rest = np.ones(self.K, dtype=bool)
        rest[ks] = False
        if not rest.any():
            return
        need = 0.0
        for b in range(self.n):
            w = self.exact(b)
            need = max(need, float(w[rest].max() - w[ks].min()))
        self.gumbel[rest] -= float(np.ceil(need + 8.0))


def make_call(seed, K, lens, jg, ratio=0.5, N=6, D=96, clamp=0):
    """a call with custom tables for `lens`, jobs of the lengths `jg` at random windows (row, start)"""
    loc, scale, pl, ps, _, _, _ = random_problem(seed, N, D, [1], 1, ratio)
    rs = np.random.RandomState(seed + 1000)
    jg = np.asarray(jg, dtype=np.int64)
    jr = rs.randint(N, size=len(jg))
    js = np.array([rs.randint(D - gl + 1) for gl in jg])
    tables = {g: normal_table(seed * 131 + g, K, g, clamp) for g in lens}
    return Call(loc, scale, pl, ps, tables, gumbel_table(seed, K), jr, js, jg)


def place_tie(call, g_tie, ks):
    """jobs of length g_tie tie bitwise on the candidates ks: identical table rows, identical Gumbel values, above all others.
    Jobs of other lengths see the same Gumbel values on different rows: they choose among ks without a tie."""
    ks = list(ks)
    call.tables[g_tie][ks[1:]] = call.tables[g_tie][ks[0]]
    call.gumbel[ks] = call.gumbel[ks[0]]
    call.sink(ks)
    return call


def tune_pair(call, b, a, k2):
    """set gumbel[k2] to the fp64 nearest gumbel[a] + T_a - T_k2, T the true Gumbel-free scores of job b, and put both above
    the rest in every job: the two best true scores of job b then differ by at most half an ulp of a Gumbel value."""
    Ta, Tb = true_scores(call.consts(b), call.xi(b), None, [a, k2])
    call.gumbel[k2] = float(Fraction(float(call.gumbel[a])) + (Ta - Tb))
    call.sink([a, k2])
    return call


ARB_LENS = (1, 2, 3, 5, 12, 33)


def arbiter_call(n, K=4099, n_jobs=16, tables=None):
    """call n of the arbiter family: 16 jobs of length ARB_LENS[n % 6], one tuned near-tie at slot n % 16 on a pair of
    candidates that changes with n; the scale ratio cycles through 0.03, 0.2, 1.  -> (call, slot, (a, b))"""
    g = ARB_LENS[n % len(ARB_LENS)]
    ratio = (0.03, 0.2, 1.0)[(n // len(ARB_LENS)) % 3]
    loc, scale, pl, ps, _, _, _ = random_problem(100 + n, 8, 120, [g], 1, ratio)
    jr, jg = np.arange(n_jobs) % 8, np.full(n_jobs, g)
    js = np.random.RandomState(8000 + n).choice(120 - g + 1, size=n_jobs, replace=False)      # sixteen different jobs
    xi = normal_table(7000 + g, K, g) if tables is None else tables[g]
    call = Call(loc, scale, pl, ps, {g: xi}, gumbel_table(5, K) if tables is None else tables["gumbel"], jr, js, jg)
    slot = n % n_jobs
    # the pair: two of the tuned job's sixteen best candidates, so that the scores that tie are of ordinary magnitude
    top = np.argsort(-call.exact(slot), kind="stable")[:16]
    a, k2 = (int(v) for v in np.random.RandomState(9000 + n).choice(top, size=2, replace=False))
    tune_pair(call, slot, a, k2)
    return call, slot, (a, k2)


def arbiter_tables(K=4099):
    t = {g: normal_table(7000 + g, K, g) for g in ARB_LENS}
    t["gumbel"] = gumbel_table(5, K)
    return t


# ---- the adversarial families of the certificate test --------------------------------------------------------------------------
FAMILY_LENS = (1, 2, 3, 7, 12, 33, 70)
FAMILIES = ("ratio 0.03", "ratio 0.2", "ratio 1", "large means", "posterior = prior +- ulp", "xi at the clamp")


def family_job(family, g, seed=0):
    """-> (Consts, xi [K, g], gumbel [K], X, G) of one job of a family; K = 256, 128 from g = 33 on"""
    K = 256 if g < 33 else 128
    rs = np.random.RandomState(seed * 977 + g * 13 + FAMILIES.index(family))
    mp = (0.01 * rs.standard_normal(g)).astype(F32)
    sp = (0.015 + 0.01 * rs.rand(g)).astype(F32)
    ratio = {"ratio 0.03": 0.03, "ratio 0.2": 0.2}.get(family, 1.0)
    mq = (mp + sp * 1.5 * rs.standard_normal(g)).astype(F32)
    sq = (sp * ratio * (0.5 + rs.rand(g))).astype(F32)
    clamp = 0
    if family == "large means":
        mp = (5.0 * (2 * rs.rand(g) - 1)).astype(F32)
        mq = (5.0 * (2 * rs.rand(g) - 1)).astype(F32)
    elif family == "posterior = prior +- ulp":
        step = rs.randint(-1, 2, size=g)
        mq = np.where(step == 0, mp, np.nextafter(mp, np.where(step > 0, F32(np.inf), F32(-np.inf)))).astype(F32)
        step = rs.randint(-1, 2, size=g)
        sq = np.where(step == 0, sp, np.nextafter(sp, np.where(step > 0, F32(np.inf), F32(-np.inf)))).astype(F32)
    elif family == "xi at the clamp":
        clamp = max(8, K // 8)
    xi = normal_table(seed * 31 + g, K, g, clamp)
    gum = gumbel_table(seed + 3, K)
    return constants(mq, sq, mp, sp), xi, gum, float(np.abs(xi).max()), float(np.abs(gum).max())
