// N4: what one element of a reconstruction becomes and what it adds to a sum of squared errors -- the per-element arithmetic and the
// workgroup sum of recon.hip (rcb_recon_finish and its _crop / _fmt / _ragged forms) and of recon_regions.hip (rcb_recon_regions),
// stated once: the two files differ in WHICH elements a workgroup adds, never in what an element is or in how a workgroup's lanes
// are combined.  The modes are those of include/rcb.h (409, 412); see the head of recon.hip.
#pragma once
#include "patch_grid.h"

// (the term dd * dd and the addition to the running sum are two roundings: never one fma)
#pragma clang fp contract(off)

namespace rcb {

// modes 2 and 3: u = fminf(rintf(c * scale), cap), the stored word (int)u - bias
struct SampleRule16 {
  float scale, cap;       // u16 at depth b: M = 2^b - 1 and M (the clamp never binds); s16: 65536 and 65535
  int bias;               // u16: 0; s16: 32768
};

inline SampleRule16 sample_rule16(int mode, int depth) {
  SampleRule16 r;
  r.scale = mode == 2 ? (float)((1 << depth) - 1) : 65536.0f;
  r.cap = mode == 2 ? r.scale : 65535.0f;
  r.bias = mode == 3 ? 32768 : 0;
  return r;
}

// the mode / depth rule of rcb_recon_finish_fmt and rcb_recon_regions
inline int check_mode_fmt(const char* who, int mode, int depth) {
  RCB_REQUIRE(mode >= 0 && mode <= 3, RCB_ERR_ARG, "%s: mode %d (0 = 8-bit, 1 = raw, 2 = u16, 3 = s16)", who, mode);
  RCB_REQUIRE(mode == 2 ? (depth >= 9 && depth <= 16) : depth == 0, RCB_ERR_ARG,
              "%s: depth %d for mode %d (9 .. 16 for u16, 0 for the others)", who, depth, mode);
  return RCB_OK;
}

struct Elem {
  float v;
  unsigned q;
  bool bad;
};

__device__ __forceinline__ bool not_finite(float x) { return !(fabsf(x) < __builtin_inff()); }

__device__ __forceinline__ Elem finish(float x, int mode) {
  Elem e;
  e.bad = not_finite(x);
  if (mode == 0) {
    const float c = (x != x) ? 0.0f : fminf(fmaxf(x, 0.0f), 1.0f);
    const float q = rintf(c * 255.0f);
    e.q = (unsigned)q;
    e.v = q / 255.0f;
  } else {
    e.q = 0;
    e.v = x;
  }
  return e;
}

// modes 2 and 3: v is formed from the INTEGER (q = 0 gives +0.0 whatever the sign of x); for s16 (float)(int)u = u and the division
// by 65536 is exact, for u16 it is the one IEEE fp32 division by M.  e.q: the 16-bit word to store.
__device__ __forceinline__ Elem finish16(float x, float scale, float cap, int bias) {
  Elem e;
  e.bad = not_finite(x);
  const float c = (x != x) ? 0.0f : fminf(fmaxf(x, 0.0f), 1.0f);
  const int u = (int)fminf(rintf(c * scale), cap);
  e.q = (unsigned)(u - bias) & 0xffffu;
  e.v = (float)u / scale;
  return e;
}

// What element e (an Elem) against target t adds: to `bad` its non-finite x and t (one with both counts twice), to `acc` the term
// (double)d * (double)d, d = t - v in fp32 -- +0.0 for a bad element (the reduce kernels make the sum NaN) and, `in` false, for an
// element that does not exist, which is never counted either.
// A macro and not a function: the register figures of recon_kernel's instantiations are held line by line from round to round
// (profiles/r*_resources.txt), and every function form of these five statements -- by reference, by value, returning the term --
// moved the scalar and vector register counts of the CROP instantiations by a few; the expansion is token for token what
// recon_kernel has always compiled.
#define RCB_RECON_ADD_TERM(e, t, in, acc, bad)                        \
  do {                                                                \
    const bool in__ = (in);                                           \
    const bool b__ = (e).bad || !(fabsf(t) < __builtin_inff());       \
    (bad) += in__ ? (int)(e).bad + (int)!(fabsf(t) < __builtin_inff()) : 0; \
    const float df__ = (t) - (e).v;                                   \
    const double dd__ = (double)df__;                                 \
    (acc) += (b__ || !in__) ? 0.0 : dd__ * dd__;                      \
  } while (0)

// The workgroup's sum of (acc, bad), valid in thread 0 (-> true there): the 64 lanes of a wave by the xor butterfly, the waves in
// wave order -- the same additions whatever the launch.
__device__ __forceinline__ bool block_sum(double& acc, int& bad) {
  __shared__ double s_acc[kThreads / kWave];
  __shared__ int s_bad[kThreads / kWave];
  acc = wave_sum(acc);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off, 64);
  if ((threadIdx.x & 63) == 0) {
    s_acc[threadIdx.x >> 6] = acc;
    s_bad[threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  acc = s_acc[0];
  bad = s_bad[0];
  for (int w = 1; w < kThreads / kWave; ++w) {
    acc += s_acc[w];
    bad += s_bad[w];
  }
  return true;
}

}  // namespace rcb
