// Device bodies (and the host code that fills their arguments) of the two once-per-step conversions of the shared
// mappings -- the packed bf16 images of the A matrices and the phase-form weights of the upsampling net -- which run behind
// their own launches (atrans.hip, upconv_weff.hip) and as block ranges of rcb_step_prepare (step_fused.hip).  One body, two
// callers.  Sums and conversions only: nothing here depends on the includer's floating-point contraction setting.
#pragma once
#include "rcb_common.h"

namespace rcb {

// ==== A transform: packed images of the mappings (atrans.hip) ====
// ---- packed images of the mappings ------------------------------------------------------------------------------------
struct PackArgs {
  const float* A[RCB_ATRANS_MAX_LAYERS];
  int L[RCB_ATRANS_MAX_LAYERS], Lp[RCB_ATRANS_MAX_LAYERS], tile0[RCB_ATRANS_MAX_LAYERS + 1];     // first 32 x 32 tile of every layer
  long long poff[RCB_ATRANS_MAX_LAYERS];      // element offset of the layer inside one plane
  long long plane;                            // elements of one plane
  __bf16* out;
  int n_layers, want_lo;
};

// (workgroup `bid` of the a.tile0[a.n_layers] workgroups of 256 threads)
__device__ __forceinline__ void atrans_pack_body(const PackArgs& a, int bid) {
  // one 32 x 32 tile per block; a thread takes four consecutive elements of a row: one 16-byte load (layer sizes that are
  // multiples of 4), 8-byte bf16 stores in both orientations (2-byte stores made this kernel 13 us for 40 MB)
  __shared__ float tile[32][33];
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  int l = 0;
  while (l + 1 < a.n_layers && bid >= a.tile0[l + 1]) ++l;
  const int L = a.L[l], Lp = a.Lp[l], nt = Lp >> 5;
  const int tl = bid - a.tile0[l];
  const int k0 = (tl / nt) * 32, j0 = (tl % nt) * 32;
  const float* __restrict__ A = a.A[l];
  const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
  __bf16* __restrict__ fwd_hi = a.out + a.poff[l];
  __bf16* __restrict__ dg_hi = a.out + a.plane + a.poff[l];
  __bf16* __restrict__ fwd_lo = a.out + 2 * a.plane + a.poff[l];
  __bf16* __restrict__ dg_lo = a.out + 3 * a.plane + a.poff[l];
  auto split_store = [&](const float (&v)[4], __bf16* hi, __bf16* lo, long long at) {
    bf16x4 h, lw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      h[i] = (__bf16)v[i];
      lw[i] = (__bf16)(v[i] - (float)h[i]);
    }
    *reinterpret_cast<bf16x4*>(hi + at) = h;
    if (a.want_lo) *reinterpret_cast<bf16x4*>(lo + at) = lw;
  };
  {
    const int k = k0 + r, j = j0 + c4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (k < L) {
      if ((L & 3) == 0 && j + 3 < L) {
        const float4 t = *reinterpret_cast<const float4*>(A + (long long)k * L + j);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (j + i < L) ? A[(long long)k * L + j + i] : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) tile[r][c4 + i] = v[i];
    split_store(v, dg_hi, dg_lo, (long long)k * Lp + j);                // data gradient: rows k, contraction j contiguous
  }
  __syncthreads();
  {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = tile[c4 + i][r];
    split_store(v, fwd_hi, fwd_lo, (long long)(j0 + r) * Lp + k0 + c4);   // forward: rows j (output column), contraction k contiguous
  }
}

inline int pad32(int v) { return (v + 31) / 32 * 32; }

// the arguments of the pack (validated by the caller); returns the number of tiles = workgroups
inline int fill_pack_args(PackArgs& a, const float* const* A, int n_layers, const int32_t* sizes, void* packed, int want_lo) {
  memset(&a, 0, sizeof(a));
  long long plane = 0;
  int tiles = 0;
  for (int l = 0; l < n_layers; ++l) {
    a.A[l] = A[l];
    a.L[l] = sizes[l];
    a.Lp[l] = pad32(sizes[l]);
    a.poff[l] = plane;
    a.tile0[l] = tiles;
    plane += (long long)a.Lp[l] * a.Lp[l];
    tiles += (a.Lp[l] / 32) * (a.Lp[l] / 32);
  }
  a.tile0[n_layers] = tiles;
  a.plane = plane;
  a.out = reinterpret_cast<__bf16*>(packed);
  a.n_layers = n_layers;
  a.want_lo = want_lo;
  return tiles;
}

// ==== upsampling net: effective (phase-form) weights (upconv_weff.hip) ====
__device__ __forceinline__ int tap_of(int a, int k) { return a == 0 ? (k == 0 ? 0 : 1) : (k == 2 ? 1 : 0); }

// one effective weight straight from the 3x3 taps: Weff[ty][tx][ci][a][b][co] = sum_{k in K(a,ty), l in K(b,tx)} W[co][ci][k][l]
__device__ __forceinline__ float weff_of(const float* __restrict__ W, int ty, int tx, int ci, int a, int b, int co) {
  const float* w = W + (co * 64 + ci) * 9;
  // (all nine taps loaded, the ones outside (a, ty) x (b, tx) dropped by a select: a branch per tap serialises the loads)
  float wv[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) wv[k] = w[k];
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int l = 0; l < 3; ++l) acc += (tap_of(a, k) == ty && tap_of(b, l) == tx) ? wv[k * 3 + l] : 0.f;
  return acc;
}

struct WeffArgs {
  const float* W1;   // [64][128][5][5]
  const float* b1;   // [64]
  const float* W2;   // [64][64][3][3]
  const float* W3;   // [16][64][3][3]
  void* weff1;       // [512][4096] bf16 or fp32
  void* b1rep;       // [4096] same type: b1 tiled over the 64 output pixels
  float* weff2;      // [2][2][64][2][2][64]
  float* weff3;      // [2][2][64][2][2][16]
  int bf16_out;
  uint4* pack;       // nullable: MFMA fragment images for the phase-conv kernels (layout: include/rcb.h)
};

template <int COUT>
__device__ __forceinline__ void build_stage(const float* __restrict__ W, float* __restrict__ out, int ci, float* w, int tid) {
  {   // (loads first, then stores: see the stage-1 branch)
    constexpr int NT = (COUT * 9 + 255) / 256;
    float t3[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const int e = tid + 256 * k;
      t3[k] = e < COUT * 9 ? W[((e / 9) * 64 + ci) * 9 + e % 9] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NT; ++k)
      if (tid + 256 * k < COUT * 9) w[tid + 256 * k] = t3[k];
  }
  __syncthreads();
  for (int e = tid; e < 16 * COUT; e += 256) {
    const int co = e % COUT, ab = (e / COUT) & 3, tt = e / (4 * COUT);
    const int a = ab >> 1, b = ab & 1, ty = tt >> 1, tx = tt & 1;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int l = 0; l < 3; ++l)
        if (tap_of(a, k) == ty && tap_of(b, l) == tx) acc += w[co * 9 + k * 3 + l];
    out[((tt * 64 + ci) * 4 + ab) * COUT + co] = acc;
  }
}

// blocks [0, 512): stage 1, one (input channel i, source pixel st) each; [512, 576): stage 2 per ci;
// [576, 640): stage 3 per ci; 640: the tiled bias; [641, 641 + 88): the packed MFMA fragments (optional)
// (workgroup `blk` of weff_build_blocks(a.pack != nullptr) workgroups of 256 threads)
__device__ __forceinline__ void weff_build_body(const WeffArgs& a, int blk) {
  __shared__ float w[64 * 25];
  const int tid = threadIdx.x;
  if (blk < 512) {
    const int i = blk >> 2, st = blk & 3, s = st >> 1, t = st & 1;
    {   // all loads first, then the stores (a load-store loop waits one memory round trip per trip: seven here)
      float t7[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const int e = tid + 256 * k;
        t7[k] = e < 64 * 25 ? a.W1[((e / 25) * 128 + i) * 25 + e % 25] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 7; ++k)
        if (tid + 256 * k < 64 * 25) w[tid + 256 * k] = t7[k];
    }
    __syncthreads();
    for (int rem = 2 * tid; rem < 4096; rem += 512) {         // two neighbouring output channels per thread: 4-byte bf16 stores
      const int y = rem >> 9, x = (rem >> 6) & 7, o = rem & 63;
      // taps whose source row y + k - 2 lies in rows [4s, 4s + 3] of the up-sampled grid (and likewise for columns)
      const int k0 = max(0, 4 * s + 2 - y), k1 = min(4, 4 * s + 5 - y);
      const int l0 = max(0, 4 * t + 2 - x), l1 = min(4, 4 * t + 5 - x);
      float acc0 = 0.f, acc1 = 0.f;
      for (int k = k0; k <= k1; ++k)
        for (int l = l0; l <= l1; ++l) {
          acc0 += w[o * 25 + k * 5 + l];
          acc1 += w[(o + 1) * 25 + k * 5 + l];
        }
      const long long idx = ((long long)st * 128 + i) * 4096 + rem;
      if (a.bf16_out) {
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        const bf16x2 pr = {(__bf16)acc0, (__bf16)acc1};
        *reinterpret_cast<bf16x2*>(reinterpret_cast<__bf16*>(a.weff1) + idx) = pr;
      } else {
        *reinterpret_cast<float2*>(reinterpret_cast<float*>(a.weff1) + idx) = make_float2(acc0, acc1);
      }
    }
  } else if (blk < 576) {
    build_stage<64>(a.W2, a.weff2, blk - 512, w, tid);
  } else if (blk < 640) {
    build_stage<16>(a.W3, a.weff3, blk - 576, w, tid);
  } else if (blk == 640) {
    for (int e = tid; e < 4096; e += 256) {
      const float v = a.b1[e & 63];
      if (a.bf16_out) reinterpret_cast<__bf16*>(a.b1rep)[e] = (__bf16)v;
      else reinterpret_cast<float*>(a.b1rep)[e] = v;
    }
  } else if (a.pack) {
    // one 16-byte fragment (8 bf16) per thread, each element summed straight from the conv taps
    const int e = (blk - 641) * 256 + tid;          // < RCB_UPCONV_PACK_UINT4
    const int lane = e & 63, q = lane & 31, h = lane >> 5;
    union { __bf16 v[8]; uint4 u; } f;
    if (e < 8192) {                                  // F2: stage-2 forward, [ph][mt][ty][tx][kb][lane]
      const int s5 = e >> 6, kb = s5 & 3, tx = (s5 >> 2) & 1, ty = (s5 >> 3) & 1, mt = (s5 >> 4) & 1, ph = s5 >> 5;
#pragma unroll
      for (int j = 0; j < 8; ++j) f.v[j] = (__bf16)weff_of(a.W2, ty, tx, 16 * kb + 8 * h + j, ph >> 1, ph & 1, 32 * mt + q);
    } else if (e < 16384) {                          // D2: stage-2 data gradient, [kh][mt][c][kb][lane]
      const int s5 = (e - 8192) >> 6, kb = s5 & 3, c = (s5 >> 2) & 7, mt = (s5 >> 5) & 1, kh = s5 >> 6;
      const int n = 8 * kh + c, ry = (n >> 2) - 1, rx = (n & 3) - 1;
      const int pa = ry & 1, ty = (ry <= 0) ? 1 : 0, pb = rx & 1, tx = (rx <= 0) ? 1 : 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) f.v[j] = (__bf16)weff_of(a.W2, ty, tx, 32 * mt + q, pa, pb, 16 * kb + 8 * h + j);
    } else if (e < 20480) {                          // F3: stage-3 forward, [pa][pb][ty][tx][kb2][lane]: A operands of
      //                                                 v_mfma_f32_16x16x32_bf16 (row co = lane & 15, ci = 32 kb2 + 8 (lane >> 4) + j);
      //                                                 the second half of the region is unused
      if (e >= 16384 + 2048) return;
      const int s5 = (e - 16384) >> 6, kb2 = s5 & 1, tx = (s5 >> 1) & 1, ty = (s5 >> 2) & 1, pb = (s5 >> 3) & 1, pa = s5 >> 4;
#pragma unroll
      for (int j = 0; j < 8; ++j) f.v[j] = (__bf16)weff_of(a.W3, ty, tx, 32 * kb2 + 8 * (lane >> 4) + j, pa, pb, lane & 15);
    } else {                                         // D3: stage-3 data gradient, [combo][mt][lane]
      const int s5 = (e - 20480) >> 6, mt = s5 & 1, n = s5 >> 1;
      const int ry = (n >> 2) - 1, rx = (n & 3) - 1;
      const int pa = ry & 1, ty = (ry <= 0) ? 1 : 0, pb = rx & 1, tx = (rx <= 0) ? 1 : 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) f.v[j] = (__bf16)weff_of(a.W3, ty, tx, 32 * mt + q, pa, pb, 8 * h + j);
    }
    a.pack[e] = f.u;
  }
}

inline int weff_build_blocks(bool frag_pack) { return frag_pack ? 641 + RCB_UPCONV_PACK_UINT4 / 256 : 641; }

}  // namespace rcb
