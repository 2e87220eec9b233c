// Shared host/device helpers for librcb_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/rcb.h"

namespace rcb {

constexpr int kWave = 64;

// thread-local last error text (diagnostics only)
char* last_error_buf();
int fail(int code, const char* fmt, ...);

#ifndef RCB_REQUIRE   // (siren_route.h states the same macro for programs built without HIP; either order of inclusion works)
#define RCB_REQUIRE(cond, code, ...)            \
  do {                                          \
    if (!(cond)) return rcb::fail((code), __VA_ARGS__); \
  } while (0)
#endif

#define RCB_LAUNCH_CHECK()                                                         \
  do {                                                                             \
    hipError_t e__ = hipGetLastError();                                            \
    if (e__ != hipSuccess) return rcb::fail((int)e__, "launch failed: %s", hipGetErrorString(e__)); \
  } while (0)

// ---- elementwise math of the posterior kernels ----------------------------------------------------------------------
// The library forms (expf, log1pf, logf, IEEE division as v_div_scale / v_div_fmas / v_div_fixup) cost 30 - 150 VALU
// instructions each: softplus + sigmoid + Gaussian KL + two Adam updates came to ~680 instructions per parameter
// element and made the "HBM-bound" posterior kernels compute-bound.  These forms use the hardware v_exp / v_log / v_rcp
// / v_sqrt with one correction step each: <= 2 ulp from the correctly rounded value (the library forms are <= 1 - 2 ulp
// themselves, and torch's CPU kernels differ from either by an ulp here and there), ~10x fewer instructions.
// Their fmas are written out; the functions themselves are defined BEFORE the includers' `#pragma clang fp contract(off)`, so a
// plain a * b + c in them (kl_elem_f32's var_ratio + t1) may still be contracted, kernel by kernel.
// Adam's square root and divisions (adam_apply, posterior_bodies.h) are built from div_fast and v_sqrt in the same way and share
// the PRECONDITION of the helpers below: no denormal intermediate, i.e. a gradient is 0 or |g| >= 1e-15 (w2 g^2 >= 1e-33).  Under
// it the suite enforces: m and v bit for bit the fp32 chains of torch/optim/adam.py, the parameter within 1/2 ulp +
// 4 * 2^-23 * step_size * |m / denom| of the fp64 update from them.

// a / b for finite, normal operands: reciprocal + one residual correction (<= 1 ulp)
__device__ __forceinline__ float div_fast(float a, float b) {
  const float r = __builtin_amdgcn_rcpf(b);
  const float q = a * r;
  const float e = __builtin_fmaf(-b, q, a);
  return __builtin_fmaf(e, r, q);
}

// e^x, |x| <= 80: the product x * log2(e) is carried as hi + lo so that the argument error does not grow with |x|
__device__ __forceinline__ float exp_fast(float x) {
  const float L = 1.44269502162933349609375f, L_lo = 1.92596299112661746e-8f;     // log2(e) = L + L_lo
  const float hi = x * L;
  const float lo = __builtin_fmaf(x, L, -hi) + x * L_lo;
  const float e = __builtin_amdgcn_exp2f(hi);
  return __builtin_fmaf(e, lo * 0.693147182464599609375f, e);                       // e * 2^lo ~ e (1 + lo ln 2)
}

// ln u for u away from 0 (hardware log2, <= 1 ulp, times ln 2).  PRECONDITION shared with div_fast / kl_elem_f32: normal,
// finite operands.  v_log / v_rcp flush denormal inputs, so a denormal variance ratio or prior scale would give -inf / inf
// where the library forms stay finite.  Not enforced: the scales here are softplus(log_scale) / 6 with log_scale started at
// -4 (prior_model.py:103) and moved by Adam steps of ~1e-4, and softplus(x) / 6 stays a normal float down to x ~ -85.
__device__ __forceinline__ float log_fast(float u) { return __builtin_amdgcn_logf(u) * 0.693147182464599609375f; }

// softplus(x, beta=1, threshold=20) / 6 in fp32  (prior_model.py:88)
// ENFORCED (tests/test_hip_posterior_exact.py, counted in tests/posterior_emul.py): within 6 ulp of the fp64 value for every x in
// [-80, 88.7] -- swept over every float around the series / log switch at t = 2^-6 (x = -4.159; log_scale starts at -4) and around
// the threshold 20 -- and x / 6 to 1/2 ulp above; measured worst 3.9 ulp.  NaN gives NaN.  +-inf give NaN, where softplus gives inf
// and 0: exp_fast forms inf - inf in `lo`.  Pinned by that test as it is: a log_scale of +-inf is a diverged run either way.
__device__ __forceinline__ float st_f32(float x) {
  const float t = exp_fast(x);
  // log1p(t): series for t < 2^-6 (truncation error t^5 / 6 relative), otherwise ln(u) + (t - (u - 1)) / u with u = fl(1 + t):
  // the second term restores what the rounding of 1 + t lost
  const float ser = t * __builtin_fmaf(t, __builtin_fmaf(t, __builtin_fmaf(t, __builtin_fmaf(t, 0.2f, -0.25f), 0.333333343f), -0.5f), 1.0f);
  const float u = 1.0f + t;
  const float c = t - (u - 1.0f);
  const float gen = __builtin_fmaf(c, __builtin_amdgcn_rcpf(u), log_fast(u));
  float sp = (t < 0.015625f) ? ser : gen;
  sp = (x > 20.0f) ? x : sp;
  // sp / 6, correctly rounded: quotient by the rounded reciprocal, one residual step
  const float q = sp * 0.16666667163372039794921875f;
  return __builtin_fmaf(__builtin_fmaf(-6.0f, q, sp), 0.16666667163372039794921875f, q);
}
// d/dx [softplus(x)/6] = sigmoid(x)/6 (1/6 above the threshold)
// ENFORCED (same tests): within 5 ulp of the fp64 value on [-80, 80] (measured worst 2.9), exactly fl(1/6) above 20 and for +inf,
// 0 for -inf; a finite x below -80 gives the value of -80 (3e-36 where sigmoid / 6 goes on to 0).  NaN gives NaN: the clamp is a
// compare and select, not fminf, which returns its other operand for a NaN and made dst_f32(NaN) the finite value of -80.
__device__ __forceinline__ float dst_f32(float x) {
  const float nx = -x;
  const float d = 1.0f + exp_fast(nx > 80.0f ? 80.0f : nx);      // (finite: the Newton step below must not see inf * 0)
  float r = __builtin_amdgcn_rcpf(d);
  r = __builtin_fmaf(__builtin_fmaf(-d, r, 1.0f), r, r);                            // Newton step: <= 1 ulp
  float sg = (x > 20.0f) ? 1.0f : r;
  sg = (x == -__builtin_inff()) ? 0.0f : sg;                                        // sigmoid(-inf) = 0, not the clamped value
  const float q = sg * 0.16666667163372039794921875f;
  return __builtin_fmaf(__builtin_fmaf(-6.0f, q, sg), 0.16666667163372039794921875f, q);
}

// torch.distributions.kl._kl_normal_normal in fp32
// ENFORCED (same tests): |result - KL| <= 4.001 * 2^-24 * (ratio^2 + t^2 + 1 + |ln ratio^2|), ratio = sig_q / sig_p, t = (mu_q -
// mu_p) / sig_p, on a grid with ratio in [2^-8, 2^8] and |t| up to 2^8; exactly 0 for q = p.  This function sits BEFORE the includers'
// `contract(off)` pragma, so `var_ratio + t1` may become fma(t, t, var_ratio) in one kernel and not in another: the bound covers both,
// and no test assumes that two kernels agree on its bits.
__device__ __forceinline__ float kl_elem_f32(float mu_q, float sig_q, float mu_p, float sig_p) {
  const float rp = __builtin_amdgcn_rcpf(sig_p);
  float ratio = sig_q * rp;
  ratio = __builtin_fmaf(__builtin_fmaf(-sig_p, ratio, sig_q), rp, ratio);          // sig_q / sig_p
  const float var_ratio = ratio * ratio;
  const float dm = mu_q - mu_p;
  float t = dm * rp;
  t = __builtin_fmaf(__builtin_fmaf(-sig_p, t, dm), rp, t);                         // (mu_q - mu_p) / sig_p
  const float t1 = t * t;
  return 0.5f * (var_ratio + t1 - 1.0f - log_fast(var_ratio));
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// ---- "the workgroup that finishes last does the epilogue", without fences -----------------------------------------------
// The textbook form (every workgroup: __threadfence(), then an atomicAdd ticket; the last one: __threadfence(), then read) is
// ruinous on this chip: the L2 is per XCD and not coherent across XCDs, so an agent-scope release fence WRITES BACK the L2
// and an acquire INVALIDATES it, and the fences of a launch serialise there -- measured 31-37 ns per fence and wave: +680 us
// on a 5 400-block launch of 30 us, +150 us on a 1 024-block one.  What the last workgroup must see is little, so it is made
// to travel past the L2 instead: data as agent-scope relaxed atomics (sc1: performed at the memory side, coherent for the
// whole device by themselves), and the ORDER "my data, then my ticket" by waiting for the data operations' completion
// (s_waitcnt 0: every outstanding load, store and atomic of the wave acknowledged) before the ticket atomic is issued.  A
// workgroup that draws the last ticket therefore finds every other workgroup's data performed, and reads it with agent-scope
// atomic loads.  Plain loads and stores of the same launch are NOT ordered by this: only what goes through these helpers.
__device__ __forceinline__ void vmem_wait_all() { __builtin_amdgcn_s_waitcnt(0); }
template <typename T>
__device__ __forceinline__ void agent_store(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ T agent_load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

}  // namespace rcb
