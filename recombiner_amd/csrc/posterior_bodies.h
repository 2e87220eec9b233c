// Device bodies of the posterior-path kernels that run in two places: behind their own launches (posterior.hip) and
// inside the combined launches of a captured training step (step_fused.hip).  One body, two callers.
//
// INCLUDE ORDER: after "rcb_common.h" and after `#pragma clang fp contract(off)`.  The arithmetic below feeds parity checks
// and is written un-fused; the translation unit that includes this file must have switched contraction off first (a
// pragma in a header would also switch it off for everything the includer defines afterwards, so it is not set here).
// rcb_common.h goes BEFORE that pragma in both translation units: its helpers (st_f32, div_fast, ...) write their fmas out
// and must see the same contraction setting in both, or the two callers would not agree to the bit.
#pragma once
#include "rcb_common.h"

using namespace rcb;

// Rounded-once arithmetic that must NOT be contracted into FMAs.  These helpers are defined under the includer's pragma
// on purpose: HIP's __fadd_rn / __fmul_rn / ... are inline functions from headers compiled with the default
// -ffp-contract=fast, so after inlining their operations carry the `contract` flag and LLVM may fuse exactly them.
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }

// ---- order-independent reductions --------------------------------------------------------------------------------------
// Sums that many workgroups (or ranks) contribute to are accumulated in 64-bit FIXED POINT with integer atomics: integer
// addition is associative, so the result does not depend on the order in which the contributions arrive -- bitwise
// reproducible from run to run, and identical whether the rows sit on one GPU or are sharded (the all-reduce over ranks
// is an integer sum as well).  A contribution is rounded once, to the fixed-point grid, where it enters.
constexpr double KL_FX = 16777216.0;          // RCB_KL_FX_SCALE = 2^24 units per nat
// KL accumulators of a step: slots [0, RCB_KL_SLOTS - 1) hold partial sums, the LAST slot counts the contributions that
// could not be represented (NaN / Inf, or beyond 2^30 nats from one workgroup): a diverged run must surface as NaN in the
// ELBO log, as it does in the reference, not as an arbitrary finite integer (__double2ll_rn(NaN) is 0).
__device__ __forceinline__ void fx_add_kl(int64_t* slots, unsigned which, double v) {
  if (fabs(v) < 1073741824.0)
    atomicAdd(reinterpret_cast<unsigned long long*>(slots + which % (RCB_KL_SLOTS - 1)), (unsigned long long)__double2ll_rn(v * KL_FX));
  else
    atomicAdd(reinterpret_cast<unsigned long long*>(slots + (RCB_KL_SLOTS - 1)), 1ull);
}

// ---- counter-based noise (Philox4x32-10 + Box-Muller) ----------------------------------------------------------
// eps of element i depends only on (seed, stream, step, i): no generator state, nothing to capture, and a replayed
// HIP graph draws fresh noise because `step` is read from device memory.  4 normals per Philox call.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
    const unsigned hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += W0;
    k.y += W1;
  }
  return c;
}

__device__ __forceinline__ float4 philox_normal4(unsigned long long group, unsigned stream, unsigned long long step,
                                                 unsigned long long seed) {
  const uint4 r = philox4x32_10(make_uint4((unsigned)group, (unsigned)(group >> 32), stream ^ (unsigned)(step >> 32) * 0x85EBCA6Bu,
                                           (unsigned)step),
                                make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
  // 24-bit uniforms: u2 in [0, 1), u1 in (0, 1] -- (float)(r >> 8) + 0.5f is not representable above 2^23 and rounds to even, so
  // r >> 8 = 2^24 - 1 gives u1 = 1 exactly and a normal of exactly 0 (one draw in 2^24; pinned by tests/posterior_emul.py)
  constexpr float K = 1.0f / 16777216.0f;
  const float u1 = ((float)(r.x >> 8) + 0.5f) * K, u2 = (float)(r.y >> 8) * K;
  const float u3 = ((float)(r.z >> 8) + 0.5f) * K, u4 = (float)(r.w >> 8) * K;
  // hardware transcendentals (about 1 ulp: ample for noise): v_log_f32 is log2, v_sin / v_cos take revolutions
  constexpr float M2LN2 = -1.3862943611198906f;             // -2 ln 2
  const float ra = __builtin_amdgcn_sqrtf(M2LN2 * __builtin_amdgcn_logf(u1));
  const float rb = __builtin_amdgcn_sqrtf(M2LN2 * __builtin_amdgcn_logf(u3));
  return make_float4(ra * __builtin_amdgcn_cosf(u2), ra * __builtin_amdgcn_sinf(u2), rb * __builtin_amdgcn_cosf(u4),
                     rb * __builtin_amdgcn_sinf(u4));
}

// four consecutive flat elements `first .. first + 3` of a [rows][cols] array as bf16 into [rows][ld16]: 4-byte stores where
// the four stay in one row and are aligned
__device__ __forceinline__ void store_bf16_row4(__bf16* __restrict__ out16, long long first, int cols, long long ld16, float4 o) {
  long long r = first / cols;
  int c = (int)(first - r * cols);
  const float ov[4] = {o.x, o.y, o.z, o.w};
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  if (c + 3 < cols && (ld16 & 1) == 0) {
    __bf16* d = out16 + r * ld16 + c;
    const bf16x2 p01 = {(__bf16)ov[0], (__bf16)ov[1]}, p12 = {(__bf16)ov[1], (__bf16)ov[2]}, p23 = {(__bf16)ov[2], (__bf16)ov[3]};
    if ((c & 1) == 0) {
      *reinterpret_cast<bf16x2*>(d) = p01;
      *reinterpret_cast<bf16x2*>(d + 2) = p23;
    } else {
      d[0] = (__bf16)ov[0];
      *reinterpret_cast<bf16x2*>(d + 1) = p12;
      d[3] = (__bf16)ov[3];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      out16[r * ld16 + c] = (__bf16)ov[k];
      if (++c == cols) { c = 0; ++r; }
    }
  }
}

// the (hi, lo) bf16 planes of four consecutive flat elements: hi = bf16(v), lo = bf16(v - hi) -- the split the A-transform
// kernel would form from the fp32 value, made by the producer instead (rcb_atrans_apply's plane operands)
__device__ __forceinline__ void store_planes_row4(__bf16* __restrict__ hi, __bf16* __restrict__ lo, long long first, int cols,
                                                  long long ld16, float4 o) {
  store_bf16_row4(hi, first, cols, ld16, o);
  if (lo) {
    const float4 r = make_float4(o.x - (float)(__bf16)o.x, o.y - (float)(__bf16)o.y, o.z - (float)(__bf16)o.z, o.w - (float)(__bf16)o.w);
    store_bf16_row4(lo, first, cols, ld16, r);
  }
}

struct AdamScalars {
  float w1;         // 1 - beta1
  float beta2;      // beta2
  float w2;         // 1 - beta2
  float step_size;  // lr / (1 - beta1^t)
  float bc2_sqrt;   // sqrt(1 - beta2^t)
  float eps;
  int enabled;
  const float* dyn;   // optional device pair {step_size, bc2_sqrt} overriding the by-value ones (graph replay)
};

static AdamScalars make_adam(const rcb_adam_cfg* c) {
  AdamScalars s;
  memset(&s, 0, sizeof(s));
  if (!c) return s;
  double bc1 = 1.0 - pow((double)c->beta1, (double)c->step);
  double bc2 = 1.0 - pow((double)c->beta2, (double)c->step);
  s.w1 = (float)(1.0 - (double)c->beta1);
  s.beta2 = c->beta2;
  s.w2 = (float)(1.0 - (double)c->beta2);
  s.step_size = (float)((double)c->lr / bc1);
  s.bc2_sqrt = (float)sqrt(bc2);
  s.eps = c->eps;
  s.enabled = 1;
  s.dyn = c->dyn_scalars;
  return s;
}

// torch.optim.Adam single step (default flags), operation order as in torch/optim/adam.py
__device__ __forceinline__ void adam_apply(float& p, float g, float& m, float& v, const AdamScalars& s) {
  const float step_size = s.dyn ? s.dyn[0] : s.step_size;
  const float bc2_sqrt = s.dyn ? s.dyn[1] : s.bc2_sqrt;
  m = add_rn(m, mul_rn(s.w1, sub_rn(g, m)));                    // exp_avg.lerp_(grad, 1-beta1)
  v = add_rn(mul_rn(v, s.beta2), mul_rn(mul_rn(s.w2, g), g));  // mul_(beta2).addcmul_(g, g, 1-beta2)
  // sqrt: hardware v_sqrt_f32 with one residual step (<= 1 ulp, 0 -> 0); the two divisions by reciprocal + residual
  // (rcb_common.h); the operation ORDER stays torch's
  float sq = __builtin_amdgcn_sqrtf(v);
  if (sq > 0.0f) sq = __builtin_fmaf(__builtin_fmaf(-sq, sq, v), 0.5f * __builtin_amdgcn_rcpf(sq), sq);
  float denom = add_rn(div_fast(sq, bc2_sqrt), s.eps);
  p = add_rn(p, mul_rn(-step_size, div_fast(m, denom)));        // addcdiv_(exp_avg, denom, -step_size)
}

struct PostBwdArgs {
  rcb_level_bwd L;
  AdamScalars adam;
};

// KL part of the gradient and the chain rule through softplus, with explicitly unfused roundings: the generic and the
// flat kernel must produce the same bits, and the reference computes these with separate torch ops anyway
__device__ __forceinline__ void kl_grad_add(float loc, float sig, float pl, float sp, float w, float& g_mu, float& g_sig) {
  const float inv_var_p = div_fast(1.0f, mul_rn(sp, sp));
  g_mu = add_rn(g_mu, mul_rn(w, mul_rn(sub_rn(loc, pl), inv_var_p)));
  g_sig = add_rn(g_sig, mul_rn(w, sub_rn(mul_rn(sig, inv_var_p), div_fast(1.0f, sig))));
}

// Fast path of posterior_bwd_kernel (posterior.hip) for the plain case (prior training of un-patched presets): one sample, no hierarchy /
// permutation / column maps, no encode mask, no per-group beta, Adam enabled, every column produced.  Purely
// elementwise over the flat [rows * cols] arrays with 16-byte accesses (rows of 3267 floats are not 16-byte aligned,
// the flat arrays are); same per-element arithmetic, so the updated parameters are bit-identical.
// Workgroup `bid` of `nblk` workgroups of 256 threads (the caller's block range: its own grid, or a range of a combined one).
__device__ __forceinline__ void posterior_flat_body(const PostBwdArgs& a, long long n_total, unsigned bid, unsigned nblk) {
  const rcb_level_bwd& L = a.L;
  // grid-stride form: with g_post_wg_per_cu > 0 the launch is capped at a few workgroups per CU that walk the array (an
  // experiment of round 4, see g_post_wg_per_cu: no effect on the forked step); uncapped, every workgroup makes one trip
  double kl = 0.0;
  const float w = L.kl_scalar_dev ? mul_rn(L.kl_scalar, *L.kl_scalar_dev) : L.kl_scalar;
  for (long long i4 = (long long)bid * 256 + threadIdx.x; i4 * 4 < n_total; i4 += (long long)nblk * 256) {
  const long long b = i4 * 4;                                                  // n_total % 4 == 0 on this path
  // streaming accesses: everything here is read once and written once per step (900 MB against 256 MB of Infinity Cache).
  // Non-temporal loads / stores took the kernel from 93.6 to 86.3 us per launch (same box) and leave the sample written at
  // the end -- the next step's first operand -- a better chance to stay cached (with loc / log_scale non-temporal as well the
  // next step's A transform took 85.4 instead of 89.4 us).
  typedef float nt_f4 __attribute__((ext_vector_type(4)));
  auto nt_ld = [](const float* p) {
    const nt_f4 t = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(p));
    return make_float4(t[0], t[1], t[2], t[3]);
  };
  auto nt_st = [](float* p, float4 v) {
    const nt_f4 t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<nt_f4*>(p));
  };
#define RCB_LD4(p) nt_ld(p)
#define RCB_ST4(p, v) nt_st(p, v)
#define RCB_LD4P(p) nt_ld(p)
#define RCB_ST4P(p, v) nt_st(p, v)
  float4 loc4 = RCB_LD4P(L.loc + b);
  float4 ls4 = RCB_LD4P(L.log_scale + b);
  const float4 go4 = RCB_LD4(L.d_out + b);
  // eps: the stored noise of this step's sample, or -- eps_from_rng -- re-drawn from the counter it was drawn from (a pure
  // function of (seed, stream, counter, element): the same bits), which saves its 4-byte write and 4-byte read per element
  const float4 ep4 = L.eps_from_rng
                         ? philox_normal4((unsigned long long)i4 + L.rng_group_offset, L.rng_stream,
                                          (unsigned long long)(*L.rng_step_dev + L.rng_step_add - 1), L.rng_seed)
                         : RCB_LD4(L.eps + b);
  float4 m14 = RCB_LD4(L.m_loc + b), v14 = RCB_LD4(L.v_loc + b);
  float4 m24 = RCB_LD4(L.m_ls + b), v24 = RCB_LD4(L.v_ls + b);
  float* locv = &loc4.x; float* lsv = &ls4.x;
  const float* gov = &go4.x; const float* epv = &ep4.x;
  float* m1v = &m14.x; float* v1v = &v14.x; float* m2v = &m24.x; float* v2v = &v24.x;
  int j = (int)(b % L.cols);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float loc = locv[k], ls = lsv[k];
    const float sig = st_f32(ls);
    float g_mu = gov[k];
    float g_sig = mul_rn(gov[k], epv[k]);
    const float pl = L.p_loc[j];
    const float sp = L.p_scale_is_log ? st_f32(L.p_scale[j]) : L.p_scale[j];
    if (L.kl_accum) kl += (double)kl_elem_f32(loc, sig, pl, sp);
    if (w != 0.0f) kl_grad_add(loc, sig, pl, sp, w, g_mu, g_sig);
    const float g_ls = mul_rn(g_sig, dst_f32(ls));
    adam_apply(loc, g_mu, m1v[k], v1v[k], a.adam);
    adam_apply(ls, g_ls, m2v[k], v2v[k], a.adam);
    locv[k] = loc;
    lsv[k] = ls;
    if (++j == L.cols) j = 0;
  }
  RCB_ST4P(L.loc + b, loc4);
  RCB_ST4P(L.log_scale + b, ls4);
  RCB_ST4(L.m_loc + b, m14);
  RCB_ST4(L.v_loc + b, v14);
  RCB_ST4(L.m_ls + b, m24);
  RCB_ST4(L.v_ls + b, v24);
  if (L.next_out || L.next_out_bf16) {
    // the next step's sample from the updated parameters: the arithmetic of reparam_rng_kernel on Philox group i4 at the
    // step counter the next step will see
    const unsigned long long step = (unsigned long long)(*L.rng_step_dev + L.rng_step_add);
    const float4 e = philox_normal4((unsigned long long)i4 + L.rng_group_offset, L.rng_stream, step, L.rng_seed);
    float4 o;
    o.x = add_rn(loc4.x, mul_rn(st_f32(ls4.x), e.x));
    o.y = add_rn(loc4.y, mul_rn(st_f32(ls4.y), e.y));
    o.z = add_rn(loc4.z, mul_rn(st_f32(ls4.z), e.z));
    o.w = add_rn(loc4.w, mul_rn(st_f32(ls4.w), e.w));
    if (L.next_eps) nt_st(L.next_eps + b, e);            // (read again by the NEXT step's update only: non-temporal, as above)
    if (L.next_out) reinterpret_cast<float4*>(L.next_out + b)[0] = o;
    if (L.next_out_bf16)
      store_planes_row4(reinterpret_cast<__bf16*>(L.next_out_bf16), reinterpret_cast<__bf16*>(L.next_out_lo), b, L.cols, L.next_ld_bf16, o);
  }
  }      // grid-stride loop
  if (L.kl_accum) {      // one fixed-point contribution per workgroup (fixed grid for a given size: reproducible)
    __shared__ double s_kl[4];
    const double kv = wave_sum(kl);
    if ((threadIdx.x & 63) == 0) s_kl[threadIdx.x >> 6] = kv;
    __syncthreads();
    if (threadIdx.x == 0)
      fx_add_kl(L.kl_accum, bid, (s_kl[0] + s_kl[1]) + (s_kl[2] + s_kl[3]));
  }
#undef RCB_LD4
#undef RCB_ST4
#undef RCB_LD4P
#undef RCB_ST4P
}

// ---- per-step bookkeeping of a captured training step (device-resident step counter) -------------------------
// One workgroup of NT threads (1024: the launch of its own; 256: a block of the combined launch, four slots per thread).
template <int NT>
__device__ __forceinline__ void step_begin_body(const float* __restrict__ table, long long n_steps,
                                                const long long* __restrict__ step, float* __restrict__ dyn,
                                                long long* __restrict__ kl_slots) {
  const int t = threadIdx.x;
  if (t < 2) {
    long long s = *step;
    if (s < 0) s = 0;
    if (s >= n_steps) s = n_steps - 1;      // replayed past the table: keep the last row rather than read outside
    dyn[t] = table[2 * s + t];
  }
  if (kl_slots)
#pragma unroll
    for (int i = t; i < RCB_KL_SLOTS; i += NT) kl_slots[i] = 0;
}

// fixed-order fp64 sums (thread-strided partials, then a tree over LDS): the same value eagerly and under replay; the KL
// slots are fixed-point integers (exact sum).
// The sum is DEFINED over 1024 virtual threads: partial v = sse[v] + sse[v + 1024] + ..., then the tree 512, 256, ..., 1.
// A workgroup of NT = 1024 threads holds one virtual thread each; one of NT = 256 (a block of the combined launch) holds
// v = t, t + 256, t + 512, t + 768 and takes the tree's first two levels in registers, (r[t] + r[t+512]) + (r[t+256] + r[t+768]),
// before the LDS tree from 128 down: the same additions in the same association, the same bits.
// ATOMIC_SLOTS: the KL slots were added to by other workgroups of THIS launch (the caller has ordered them before this
// call with a ticket, rcb_common.h): read them with agent-scope atomic loads, past the caches.
template <int NT, bool ATOMIC_SLOTS>
__device__ __forceinline__ void step_end_body(const float* __restrict__ sse, int n_sse, double mse_scale,
                                              const long long* kl_slots, double* __restrict__ mse_log,
                                              double* __restrict__ kl_log, long long n_log,
                                              long long* __restrict__ step, long long* __restrict__ aux_counter) {
  static_assert(NT == 1024 || NT == 256, "the tree is written for these two");
  constexpr int V = 1024 / NT;
  __shared__ double red[NT];
  __shared__ long long redk[NT];
  const int t = threadIdx.x;
  auto slot = [&](int i) -> long long {
    if (ATOMIC_SLOTS) return agent_load(kl_slots + i);
    return kl_slots[i];
  };
  double r[V];
  long long rk[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int vt = t + NT * j;
    double a = 0.0;
    if (sse)
      for (int i = vt; i < n_sse; i += 1024) a += (double)sse[i];
    r[j] = a;
    rk[j] = (kl_slots && vt < RCB_KL_SLOTS - 1) ? slot(vt) : 0;       // (the last slot is the not-representable counter)
  }
#pragma unroll
  for (int off = 512; off >= NT; off >>= 1)      // tree levels above the workgroup size: virtual thread v += v + off
#pragma unroll
    for (int j = 0; j < off / NT; ++j) {
      r[j] += r[j + off / NT];
      rk[j] += rk[j + off / NT];
    }
  red[t] = r[0];
  redk[t] = rk[0];
  __syncthreads();
  for (int off = NT / 2; off > 0; off >>= 1) {
    if (t < off) {
      red[t] += red[t + off];
      redk[t] += redk[t + off];
    }
    __syncthreads();
  }
  if (t == 0) {
    const long long s = *step;
    if (s >= 0 && s < n_log) {
      if (mse_log && sse) mse_log[s] = red[0] * mse_scale;
      if (kl_log && kl_slots)
        kl_log[s] = slot(RCB_KL_SLOTS - 1) ? __builtin_nan("") : (double)redk[0] * (1.0 / KL_FX);
    }
    *step = s + 1;
    if (aux_counter) *aux_counter += 1;      // e.g. the noise counter, which is NOT reset between train() calls
  }
}

struct AdamMultiArgs {
  float* p[RCB_ADAM_MAX_TENSORS];
  const float* g[RCB_ADAM_MAX_TENSORS];
  float* m[RCB_ADAM_MAX_TENSORS];
  float* v[RCB_ADAM_MAX_TENSORS];
  long long n[RCB_ADAM_MAX_TENSORS];
  int blk_start[RCB_ADAM_MAX_TENSORS + 1];   // first block of each tensor (1024 elements per block)
  int count;
  AdamScalars s;
};

// one launch for a list of tensors (the shared mappings: 4 A matrices + 6 conv tensors)
// (workgroup `bid` of the a.blk_start[a.count] workgroups of 256 threads)
__device__ __forceinline__ void adam_multi_body(const AdamMultiArgs& a, int bid) {
  int t = 0;
#pragma unroll 1
  while (t + 1 < a.count && bid >= a.blk_start[t + 1]) ++t;
  const long long base = (long long)(bid - a.blk_start[t]) * 1024;
  float* p = a.p[t];
  const float* g = a.g[t];
  float* m = a.m[t];
  float* v = a.v[t];
  const long long n = a.n[t];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = base + k * 256 + threadIdx.x;
    if (i < n) {
      // (moments and gradient: streamed once per step, non-temporal; the parameter itself is read by the next kernel)
      float pi = p[i], mi = __builtin_nontemporal_load(m + i), vi = __builtin_nontemporal_load(v + i);
      adam_apply(pi, __builtin_nontemporal_load(g + i), mi, vi, a.s);
      p[i] = pi;
      __builtin_nontemporal_store(mi, m + i);
      __builtin_nontemporal_store(vi, v + i);
    }
  }
}
