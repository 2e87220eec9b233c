// One wave per row: the 16-bit SIREN kernels of the narrow family (uniform hidden width 16 or 24, 1 to 4 hidden layers) and of the
// deep family (5 to 7 hidden layers of one width 16, 24 or 32), forward / backward / fused loss + backward.
//
// One WAVE (a 64-thread workgroup) per row of wvec -- an (INR, sample) -- or per pixel chunk of it.  There is no barrier across
// waves, no cross-wave reduction and no atomic: the pixel tiles of a row are summed in ascending order and the row's gradient
// leaves straight from the accumulators; which tiles a wave takes depends on P and pixel_chunks only, so the kernels are bitwise
// deterministic and batch invariant.
//
// Matrix instruction: v_mfma_f32_16x16x32_{bf16,f16}, in the transposed orientation of the other SIREN kernels
//      Z^T[out, pix] = W^T[out, in] * H^T[in, pix]        (N = 16 pixels on lane & 15, M = 16 output features, K = 32 inputs)
// A 16-feature block of a layer's output is one accumulator (lane l: features 4 (l >> 4) + 0..3 of pixel l & 15).  The next
// layer's B operand needs 8 k-values per lane at k = 8 (l >> 4) + j; the k order is free (A is built to match), so k-slot
// (g = l >> 4, j) is feature 4 g + j of block 0 for j < 4 and feature 16 + 4 g + (j - 4) of block 1 for j >= 4: the 4 + 4
// accumulator registers of a lane ARE its B operand, no data moves between lanes.  Width 16 leaves block 1 empty (zeros);
// width 24 is carried as two blocks whose padding units 24..31 have zero weights and biases, so they are exactly 0 through
// sin.  Their sines are not evaluated: the valid half-waves of block 1 of the tile's two 16-pixel halves are brought
// together by v_permlane32_swap, one sin / cos per register pair instead of two.  Width 32 is two full blocks.
// Layer 0 takes its K from both input halves at once: k-slot (g, j) of step s is Fourier feature 16 s + 8 g + j for g < 2 and
// pe feature 16 s + 8 (g - 2) + j for g >= 2 -- a lane loads 8 consecutive features (16 bytes of a 16-bit row) of its pixel.
//
// Where a row's weights live is the one thing that differs between the families, and it is a type (the weights store):
//   * RegStore (1 to 4 layers): at these depths everything a row reuses fits in the wave's registers -- the weight fragments of
//     every layer in both orientations and the biases, next to the weight-gradient accumulators of the whole row.  The row of
//     layer vectors is staged through LDS once, in the area the tile images use afterwards.
//   * LdsStore (5 to 7 layers): 7 layers of width 32 would be ~ 270 registers of weights next to the accumulators.  The fragments
//     are built once per row into LDS in lane order (slot k: 64 lanes x 16 bytes, one conflict-free ds_read_b128 per MFMA
//     operand), the biases as 16 floats per 16-unit block (read by k-group).  The row is staged one layer vector at a time (the
//     largest is 32 x 65 floats) through the image area, so that the LDS of a wave is the fragments plus the images: <= 60 KB.
// Both are addressed by the slot map of Geo, and the fragment values are built by one routine.  The kernel body only calls the
// store; a fragment is fetched once and used for both halves of the tile.
//
// Weight gradient dW^T[out, in] += dZ^T[out, pix] H[pix, in] contracts over pixels, which sit on the lanes: the tile's layer
// inputs (written in the forward pass) and its dz (written in the backward pass) go through the wave's LDS as [feature][pixel]
// 16-bit images -- a 32-pixel tile is two halves, lane l holding pixels 2 (l & 15) and 2 (l & 15) + 1, so one 4-byte store puts
// a feature's pixel pair in place -- and are read back by row (one ds_read_b128 per operand: 8 pixels of one feature, rows
// 80 bytes apart: conflict-free).  Bias gradients are the sums of the same dz operands (v_dot2 against ones).
//
// Rounding is that of the width-32 16-bit kernels: weights, layer inputs, sines and dz rounded to the operand type, fp32
// accumulation and fp32 cosines; the sine layers work in revolutions (w0 / 2 pi folded into their forward fragments and biases),
// the data-gradient fragments of the hidden and output layers carry w0, f16 scales weights and gradients by 2^10 (Op16).
// Matches prior_model.py:168-179,237 and test_model.py:347-355,625-627 like the kernels it stands beside.
#include <type_traits>

#include "siren_op16.h"

using namespace rcb;

namespace {
using namespace rcb::op16;

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename T> __device__ __forceinline__ f32x4 mfma16(typename Op16<T>::v8 a, typename Op16<T>::v8 b, f32x4 c);
template <> __device__ __forceinline__ f32x4 mfma16<__bf16>(Op16<__bf16>::v8 a, Op16<__bf16>::v8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 mfma16<_Float16>(Op16<_Float16>::v8 a, Op16<_Float16>::v8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

constexpr int IST = 40;   // row stride of the LDS images in 16-bit elements (32 pixels + 8: 80 bytes, conflict-free b128 row reads)

// KS: k-steps of layer 0 (1: F, E <= 16; 2: F, E <= 32); also the bound on the 16-wide blocks of out_dim and pe_dim
template <int NH, int HW, int KS>
struct Geo {
  static constexpr int HB = (HW + 15) / 16;        // 16-feature blocks of a hidden layer
  static constexpr int NL = NH + 1;
  static constexpr int IB0 = 2 * KS;               // 16-feature blocks of layer 0's input (at most)
  static constexpr int CB = KS, EB = KS;           // ... of out_dim, of pe_dim (at most)
  static constexpr int DZB = HB > CB ? HB : CB;
  // fragment slots (64 lanes x 8 16-bit elements each)
  static constexpr int S_F0 = 0;                   // forward, layer 0: [KS][HB]
  static constexpr int S_FH = S_F0 + KS * HB;      // forward, hidden layers 1 .. NH - 1: [NH - 1][HB]
  static constexpr int S_FO = S_FH + (NH - 1) * HB;   // forward, output layer: [CB]
  static constexpr int S_BO = S_FO + CB;           // data gradient through the output layer: [HB]
  static constexpr int S_BH = S_BO + HB;           // ... through hidden layers 1 .. NH - 1: [NH - 1][HB]
  static constexpr int S_BE = S_BH + (NH - 1) * HB;   // ... of pe through layer 0: [EB]
  static constexpr int NFRAG = S_BE + EB;
  static constexpr int NBIAS = NH * HB + CB;       // bias blocks (16 floats each): block b of layer l is l * HB + b
  // LDS image rows: layer 0's input, the inputs of layers 1 .. NH (sines), dz
  static constexpr int X_ROWS = 16 * IB0;
  static constexpr int S_ROWS = 16 * HB;
  static constexpr int ROWS = X_ROWS + NH * S_ROWS + 16 * DZB;
  static constexpr int IMG_BYTES = ROWS * IST * 2;
  // floats of the largest layer vector, bias and weights: layer 0 (32 KS inputs) or a layer of 32 KS outputs
  static constexpr int LAYER_MAX = HW * (32 * KS + 1) > 32 * KS * (HW + 1) ? HW * (32 * KS + 1) : 32 * KS * (HW + 1);
  // the input rows of the next tile are loaded during this one, except at 7 layers of width 24 / 32 with two k-steps in layer 0,
  // where their 32 registers would push the accumulators into scratch: there the tile's rows are loaded at its start
  static constexpr bool PREFETCH = !(NH == 7 && HB == 2 && KS == 2);
};

// ---- the weights stores: a row's fragments (by slot) and bias blocks; the LDS behind the fixed part is the work area, which
// holds the staged layer vectors first and the tile images afterwards ----------------------------------------------------------
template <typename T, class G>
struct RegStore {
  using v8 = typename Op16<T>::v8;
  static constexpr bool WHOLE_ROW = true;          // the row of layer vectors is staged once, then every layer is built
  static constexpr int STAGE_LOADS = 16;           // global loads a lane keeps in flight while staging
  static constexpr int FIXED_BYTES = 0;
  static size_t lds_bytes(int dnet) { return (size_t)(G::IMG_BYTES > dnet * 4 ? G::IMG_BYTES : dnet * 4); }
  // every loop over slots is fully unrolled: the indices are constants and the arrays are registers
  v8 fr[G::NFRAG];
  f32x4 bi[G::NBIAS];
  __device__ __forceinline__ RegStore(unsigned char*, int) {}
  __device__ __forceinline__ void put_frag(int slot, const v8& v) { fr[slot] = v; }
  __device__ __forceinline__ void put_bias(int blk, const f32x4& v) { bi[blk] = v; }
  __device__ __forceinline__ v8 frag(int slot) const { return fr[slot]; }
  __device__ __forceinline__ f32x4 bias(int blk) const { return bi[blk]; }
};

template <typename T, class G>
struct LdsStore {
  using v8 = typename Op16<T>::v8;
  static constexpr bool WHOLE_ROW = false;         // one layer vector at a time: stage, build, next
  static constexpr int STAGE_LOADS = 8;
  static constexpr int FRAG_BYTES = G::NFRAG * 64 * 16;
  static constexpr int FIXED_BYTES = FRAG_BYTES + G::NBIAS * 16 * 4;
  static constexpr int LDS_BYTES = FIXED_BYTES + (G::IMG_BYTES > 4 * G::LAYER_MAX ? G::IMG_BYTES : 4 * G::LAYER_MAX);
  static_assert(LDS_BYTES <= 64 * 1024, "one wave's LDS stays within the default dynamic limit");
  static size_t lds_bytes(int) { return LDS_BYTES; }
  T* const my_frag;             // this lane's 16 bytes of slot 0
  float* const my_bias;         // this lane's k-group of bias block 0
  const bool writes_bias;
  __device__ __forceinline__ LdsStore(unsigned char* smem, int lane)
      : my_frag(reinterpret_cast<T*>(smem) + lane * 8), my_bias(reinterpret_cast<float*>(smem + FRAG_BYTES) + 4 * (lane >> 4)),
        writes_bias((lane & 15) == 0) {}
  __device__ __forceinline__ void put_frag(int slot, const v8& v) { *reinterpret_cast<v8*>(my_frag + slot * 512) = v; }
  __device__ __forceinline__ void put_bias(int blk, const f32x4& v) {
    if (writes_bias) *reinterpret_cast<f32x4*>(my_bias + blk * 16) = v;
  }
  __device__ __forceinline__ v8 frag(int slot) const { return *reinterpret_cast<const v8*>(my_frag + slot * 512); }
  __device__ __forceinline__ f32x4 bias(int blk) const { return *reinterpret_cast<const f32x4*>(my_bias + blk * 16); }
};

// k-slot (g, j) of a B operand packed from accumulator blocks -> feature index
__device__ __forceinline__ int kfeat(int g, int j) { return j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4); }

template <typename T>
__device__ __forceinline__ typename Op16<T>::v8 pack_blocks(const f32x4& b0, const f32x4& b1, bool two) {
  typename Op16<T>::v8 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j] = (T)b0[j];
    o[4 + j] = two ? (T)b1[j] : (T)0.0f;
  }
  return o;
}

__device__ __forceinline__ f32x4 zero4() {
  f32x4 z;
#pragma unroll
  for (int i = 0; i < 4; ++i) z[i] = 0.f;
  return z;
}

// A dz is an fp32 product, rounded to fp32 and then to the operand type.  Left to itself the compiler merges product and
// conversion of the f16 instances into one v_fma_mixlo_f16 -- a single rounding -- but only where both land in one basic block,
// so that the rounding of a dz element depended on code placement (of the two halves of a tile, one was merged).  The product
// passes through here before its conversion and reaches it as an fp32 value.
template <typename T>
__device__ __forceinline__ float fp32_value(float x) {
  if constexpr (!Op16<T>::IS_BF16) asm("" : "+v"(x));
  return x;
}

__device__ __forceinline__ float swap_lo_hi(float& x, float y) {   // x <- [x.lo | y.lo], returns [x.hi | y.hi]
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
  x = __uint_as_float(r[0]);
  return __uint_as_float(r[1]);
}

template <typename T, int NH, int HW, int KS, bool FWD, class Store>
__global__ void __launch_bounds__(64) siren_rowwave_kernel(SirenArgs a) {
  using G = Geo<NH, HW, KS>;
  using v8 = typename Op16<T>::v8;
  using v2 = typename Op16<T>::v2;
  constexpr float GS = Op16<T>::GRAD_SCALE;
  constexpr float WS = Op16<T>::W_SCALE;
  constexpr int HB = G::HB, NL = G::NL;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x;
  const int m = lane & 15, g4 = lane >> 4;     // B / D role: pixel pair m; A role: row m.  g4: k-group / accumulator row group
  const int row = blockIdx.x % a.G, chunk = blockIdx.x / a.G;      // chunk-major: partial buffers are [chunk][row]
  const int n = row / a.S;
  const int P = a.P, F = a.F, E = a.E, C = a.C;
  const int IN0 = F + E;
  const int ib0 = (IN0 + 15) >> 4, cb_n = (C + 15) >> 4, eb_n = (E + 15) >> 4;
  const bool loss = a.sse != nullptr;          // MODE_LOSS (targets) or MODE_BWD (upstream gradient)
  const long long pe_row = pe_row_base(a, row);
  // layer vector offsets in a row of wvec: [bias | W(in, out)] per layer
  const int off1 = HW * (IN0 + 1);
  auto loff = [&](int l) { return l == 0 ? 0 : off1 + (l - 1) * HW * (HW + 1); };
  const int offo = loff(NH);

  Store W(smem_raw, lane);
  unsigned char* const work = smem_raw + Store::FIXED_BYTES;

  // ---- fragments and biases of the row, from its layer vectors staged in the work area ---------------------------------------
  const float kw = a.k_hi * WS;                // sine layers: revolutions, f16 weight scale
  {
    const float* src_row = a.wvec + (long long)row * a.w_stride;
    float* const wl = reinterpret_cast<float*>(work);
    auto stage = [&](const float* src, float* dst, int len) {
      for (int i0 = lane; i0 < len; i0 += Store::STAGE_LOADS * 64) {
        float st[Store::STAGE_LOADS];
#pragma unroll
        for (int k = 0; k < Store::STAGE_LOADS; ++k) {
          const int i = i0 + 64 * k;
          st[k] = src[i < len ? i : len - 1];
        }
#pragma unroll
        for (int k = 0; k < Store::STAGE_LOADS; ++k) {
          const int i = i0 + 64 * k;
          if (i < len) dst[i] = st[k];
        }
      }
      __syncthreads();
    };
    // an A fragment: element j of lane (m, g4) is wv[idx] * scale rounded to the operand type where at(j, idx) holds, else 0
    // (validity and index stay two values: folded into one signed index, the scalar registers of the tile loop spill twice as much)
    auto a_frag = [&](const float* wv, float scale, auto at) -> v8 {
      v8 fr;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int i;
        const bool ok = at(j, i);
        const float v = wv[ok ? i : 0];
        fr[j] = (T)(ok ? v * scale : 0.f);
      }
      return fr;
    };
    // layer l from its vector wv = [bias | W(in, out)].  Forward fragments: element j = W[in of k-slot (g4, j)][out 16 ob + m];
    // data-gradient fragments: element j = W[in 16 ib + m][out of k-slot (g4, j)]
    auto build_layer = [&](int l, const float* wv) {
      if (l == 0) {
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
          for (int ob = 0; ob < HB; ++ob)
            W.put_frag(G::S_F0 + s * HB + ob, a_frag(wv, kw, [&](int j, int& idx) {
              const int f0 = 16 * s + 8 * (g4 & 1) + j, out = 16 * ob + m;
              const bool ok_in = g4 < 2 ? f0 < F : f0 < E;
              idx = HW + (g4 < 2 ? f0 : F + f0) * HW + out;
              return ok_in && out < HW;
            }));
#pragma unroll
        for (int eb = 0; eb < G::EB; ++eb)       // pe data gradient: rows F + 16 eb + m
          W.put_frag(G::S_BE + eb, a_frag(wv, WS, [&](int j, int& idx) {
            const int kf = kfeat(g4, j), e = 16 * eb + m;
            idx = HW + (F + e) * HW + kf;
              return kf < HW && e < E;
          }));
      } else if (l < NH) {
#pragma unroll
        for (int b = 0; b < HB; ++b) {
          const int u = 16 * b + m;
          W.put_frag(G::S_FH + (l - 1) * HB + b, a_frag(wv, kw, [&](int j, int& idx) {
            const int kf = kfeat(g4, j);
            idx = HW + kf * HW + u;
              return kf < HW && u < HW;
          }));
          W.put_frag(G::S_BH + (l - 1) * HB + b, a_frag(wv, a.w0, [&](int j, int& idx) {
            const int kf = kfeat(g4, j);
            idx = HW + u * HW + kf;
              return kf < HW && u < HW;
          }));
        }
      } else {
#pragma unroll
        for (int cb = 0; cb < G::CB; ++cb)
          W.put_frag(G::S_FO + cb, a_frag(wv, WS, [&](int j, int& idx) {
            const int kf = kfeat(g4, j), out = 16 * cb + m;
            idx = C + kf * C + out;
              return kf < HW && out < C;
          }));
#pragma unroll
        for (int ib = 0; ib < HB; ++ib)
          W.put_frag(G::S_BO + ib, a_frag(wv, a.w0, [&](int j, int& idx) {
            const int kf = kfeat(g4, j), in = 16 * ib + m;
            idx = C + in * C + kf;
              return kf < C && in < HW;
          }));
      }
      // bias blocks: lane (m, g4) holds units 16 b + 4 g4 + 0..3, in revolutions for the sine layers
#pragma unroll
      for (int b = 0; b < G::DZB; ++b) {
        if (b >= (l < NH ? HB : G::CB)) continue;
        f32x4 bv;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int u = 16 * b + 4 * g4 + i;
          const bool ok = u < (l < NH ? HW : C);
          const float v = wv[ok ? u : 0];
          bv[i] = ok ? (l < NH ? v * kw : v) : 0.f;
        }
        W.put_bias(l * HB + b, bv);
      }
    };
    if constexpr (Store::WHOLE_ROW) {
      stage(src_row, wl, a.dnet);
#pragma unroll
      for (int l = 0; l < NL; ++l) build_layer(l, wl + loff(l));
      __syncthreads();        // the images below reuse the staging area
    } else {
#pragma unroll 1
      for (int l = 0; l < NL; ++l) {
        stage(src_row + loff(l), wl, l == 0 ? off1 : (l == NH ? C * (HW + 1) : HW * (HW + 1)));
        build_layer(l, wl);
        __syncthreads();      // the next layer (or the images) reuse the staging area
      }
    }
  }

  T* const img = reinterpret_cast<T*>(work);
  T* const x_img = img;                                                        // layer 0's input: rows = input features
  auto s_img = [&](int l) { return img + (G::X_ROWS + (l - 1) * G::S_ROWS) * IST; };   // input of layer l >= 1
  T* const dz_img = img + (G::X_ROWS + NH * G::S_ROWS) * IST;
  auto put_pair16 = [&](T* im, int r, T v0, T v1) {       // a feature's pixel pair (2 m, 2 m + 1) -> one 4-byte store
    v2 pr = {v0, v1};
    *reinterpret_cast<v2*>(im + r * IST + 2 * m) = pr;
  };
  auto get_row = [&](const T* im, int r) -> v8 {      // 8 pixels 8 g4 .. 8 g4 + 7 of feature row r
    union { uint4 u; v8 v; } x;
    x.u = *reinterpret_cast<const uint4*>(im + r * IST + 8 * g4);
    return x.v;
  };

  // weight-gradient accumulators: dW^T[out 16 ob + 4 g4 + i][in 16 ib + m]
  f32x4 gw0[HB][G::IB0], gwh[NH > 1 ? NH - 1 : 1][HB][HB], gwo[G::CB][HB];
  float gb[NL][G::DZB];        // bias gradients: per lane, row m of the dz operand
  float sse_local = 0.f;
  if (!FWD) {
#pragma unroll
    for (int ob = 0; ob < HB; ++ob)
#pragma unroll
      for (int ib = 0; ib < G::IB0; ++ib) gw0[ob][ib] = zero4();
#pragma unroll
    for (int l = 0; l < NH - 1; ++l)
#pragma unroll
      for (int ob = 0; ob < HB; ++ob)
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) gwh[l][ob][ib] = zero4();
#pragma unroll
    for (int cb = 0; cb < G::CB; ++cb)
#pragma unroll
      for (int ib = 0; ib < HB; ++ib) gwo[cb][ib] = zero4();
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
      for (int b = 0; b < G::DZB; ++b) gb[l][b] = 0.f;
  }

  // ---- input rows: lane (m, g4), half ph holds pixel 2 m + ph of the tile, features 16 s + 8 (g4 & 1) + 0..7 of xf (g4 < 2)
  // or pe (g4 >= 2), as 16-bit rows (xf_bf16 copy / bf16 pe) or fp32 rows ----------------------------------------------------
  const bool pe_lane = g4 >= 2;
  const bool in16 = pe_lane ? a.pe_bf16 != 0 : (a.xf16 != nullptr && a.pe_bf16 != 0);
  const int FP = (F + 7) / 8 * 8;                          // row length of the 16-bit xf copy
  const int lim = pe_lane ? E : (in16 ? FP : F);
  uint32_t raw[2][KS][8];
  const int ntiles = (P + 31) >> 5;
  auto fetch = [&](int t) {
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
      const int p = 32 * t + 2 * m + ph;
      const int pc = p < P ? p : P - 1;
      const long long pix = pe_lane ? (pe_row + pe_pix_off(a, pc)) * E
                                    : (in16 ? (long long)n * (a.xf_stride / F * FP) + (long long)pc * FP
                                            : (long long)n * a.xf_stride + (long long)pc * F);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int f0 = 16 * s + 8 * (g4 & 1);
#pragma unroll
        for (int w = 0; w < 8; ++w) raw[ph][s][w] = 0u;
        if (in16) {
          if (f0 + 8 <= lim) {
            const unsigned short* base = pe_lane ? reinterpret_cast<const unsigned short*>(a.pe)
                                                 : reinterpret_cast<const unsigned short*>(a.xf16);
            const uint4 u = *reinterpret_cast<const uint4*>(base + pix + f0);
            raw[ph][s][0] = u.x; raw[ph][s][1] = u.y; raw[ph][s][2] = u.z; raw[ph][s][3] = u.w;
          }
        } else {
          const float* base = pe_lane ? a.pe : a.xf;
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            if (f0 + 2 * jj + 2 <= lim) {
              const float2 v = *reinterpret_cast<const float2*>(base + pix + f0 + 2 * jj);
              raw[ph][s][2 * jj] = __float_as_uint(v.x);
              raw[ph][s][2 * jj + 1] = __float_as_uint(v.y);
            }
          }
        }
      }
    }
  };
  auto operand = [&](const uint32_t (&r)[8]) -> v8 {
    if (in16) return in16_operand<T>(make_uint4(r[0], r[1], r[2], r[3]), pe_lane ? 1 : 0);
    v8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (T)__uint_as_float(r[j]);
    return o;
  };
  // targets (loss) / upstream gradient (backward) of channels 16 cb + 4 g4 + i, one tile ahead
  float ynext[2][G::CB][4];
  const float* __restrict__ yrow = a.yin + (loss ? (long long)n : (long long)row) * P * C;
  auto fetch_y = [&](int t) {
    if (FWD) return;
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
      const int p = 32 * t + 2 * m + ph;
      const int pc = p < P ? p : P - 1;
#pragma unroll
      for (int cb = 0; cb < G::CB; ++cb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = 16 * cb + 4 * g4 + i;
          ynext[ph][cb][i] = 0.f;
          if (cb < cb_n) ynext[ph][cb][i] = yrow[pc * C + (c < C ? c : C - 1)];
        }
    }
  };

  const int t0 = (int)((long long)chunk * ntiles / a.chunks), t1 = (int)((long long)(chunk + 1) * ntiles / a.chunks);
  if (G::PREFETCH) fetch(t0);
  fetch_y(t0);
  for (int t = t0; t < t1; ++t) {
    if (!G::PREFETCH) fetch(t);
    bool valid[2];
    int pix[2];
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
      pix[ph] = 32 * t + 2 * m + ph;
      valid[ph] = pix[ph] < P;
    }
    v8 xb[2][KS];
#pragma unroll
    for (int ph = 0; ph < 2; ++ph)
#pragma unroll
      for (int s = 0; s < KS; ++s) xb[ph][s] = operand(raw[ph][s]);
    float yv[2][G::CB][4];
    if (!FWD) {
#pragma unroll
      for (int ph = 0; ph < 2; ++ph)
#pragma unroll
        for (int cb = 0; cb < G::CB; ++cb)
#pragma unroll
          for (int i = 0; i < 4; ++i) yv[ph][cb][i] = ynext[ph][cb][i];
    }
    if (G::PREFETCH) fetch(t + 1 < t1 ? t + 1 : t);
    fetch_y(t + 1 < t1 ? t + 1 : t);

    // ---- forward ----------------------------------------------------------------------------------------------------
    if (!FWD) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int f0 = 16 * s + 8 * (g4 & 1) + j;
          if (f0 < (pe_lane ? E : F)) put_pair16(x_img, pe_lane ? F + f0 : f0, xb[0][s][j], xb[1][s][j]);
        }
    }
    f32x4 Cf[NH][2][HB];
    v8 hb[2];                      // B operand of the next layer
#pragma unroll
    for (int l = 0; l < NH; ++l) {
      f32x4 z[2][HB];
#pragma unroll
      for (int ob = 0; ob < HB; ++ob) {
        const f32x4 b0 = W.bias(l * HB + ob);
        f32x4 acc[2] = {b0, b0};
        if (l == 0) {
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            const v8 w = W.frag(G::S_F0 + s * HB + ob);
#pragma unroll
            for (int ph = 0; ph < 2; ++ph) acc[ph] = mfma16<T>(w, xb[ph][s], acc[ph]);
          }
        } else {
          const v8 w = W.frag(G::S_FH + (l - 1) * HB + ob);
#pragma unroll
          for (int ph = 0; ph < 2; ++ph) acc[ph] = mfma16<T>(w, hb[ph], acc[ph]);
        }
#pragma unroll
        for (int ph = 0; ph < 2; ++ph)
#pragma unroll
          for (int i = 0; i < 4; ++i) z[ph][ob][i] = (WS == 1.0f) ? acc[ph][i] : acc[ph][i] * (1.0f / WS);   // revolutions
      }
      f32x4 sv[2][HB], cv[2][HB];
      constexpr int FULL = HW / 16;                  // blocks with 16 units
#pragma unroll
      for (int ph = 0; ph < 2; ++ph)
#pragma unroll
        for (int ob = 0; ob < FULL; ++ob)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sv[ph][ob][i] = __builtin_amdgcn_sinf(z[ph][ob][i]);
            if (!FWD) cv[ph][ob][i] = __builtin_amdgcn_cosf(z[ph][ob][i]);
          }
      if constexpr (HW == 24) {
        // block 1: units 16..23 sit in lanes 0..31; the two halves' valid lanes are paired in one register
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float zz = z[0][1][i];
          swap_lo_hi(zz, z[1][1][i]);              // [half 0 | half 1], units 16 + 4 g4 + i, g4 < 2
          float s0 = __builtin_amdgcn_sinf(zz);
          sv[1][1][i] = swap_lo_hi(s0, 0.f);       // back apart; the padding lanes receive 0
          sv[0][1][i] = s0;
          if (!FWD) {
            float c0 = __builtin_amdgcn_cosf(zz);
            cv[1][1][i] = swap_lo_hi(c0, 0.f);
            cv[0][1][i] = c0;
          }
        }
      }
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        hb[ph] = pack_blocks<T>(sv[ph][0], sv[ph][HB - 1], HB == 2);
        if (!FWD) {
#pragma unroll
          for (int ob = 0; ob < HB; ++ob) Cf[l][ph][ob] = cv[ph][ob];
        }
      }
      if (!FWD) {
#pragma unroll
        for (int ob = 0; ob < HB; ++ob)
#pragma unroll
          for (int i = 0; i < 4; ++i) put_pair16(s_img(l + 1), 16 * ob + 4 * g4 + i, hb[0][4 * ob + i], hb[1][4 * ob + i]);
      }
    }
    f32x4 yo[2][G::CB];
#pragma unroll
    for (int cb = 0; cb < G::CB; ++cb) {
      if (cb >= cb_n) continue;
      const v8 w = W.frag(G::S_FO + cb);
      const f32x4 bo = W.bias(NH * HB + cb);
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        const f32x4 acc = mfma16<T>(w, hb[ph], zero4());
#pragma unroll
        for (int i = 0; i < 4; ++i) yo[ph][cb][i] = ((WS == 1.0f) ? acc[i] : acc[i] * (1.0f / WS)) + bo[i];
      }
    }
    if (FWD) {
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        if (!valid[ph]) continue;
#pragma unroll
        for (int cb = 0; cb < G::CB; ++cb) {
          if (cb >= cb_n) continue;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int c = 16 * cb + 4 * g4 + i;
            if (c < C) a.yout[((long long)row * P + pix[ph]) * C + c] = yo[ph][cb][i];
          }
        }
      }
      continue;
    }

    // ---- output gradient ---------------------------------------------------------------------------------------------
    f32x4 dz[2][G::DZB];
#pragma unroll
    for (int ph = 0; ph < 2; ++ph)
#pragma unroll
      for (int b = 0; b < G::DZB; ++b) {
        dz[ph][b] = zero4();
        if (b >= G::CB || b >= cb_n) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool ok = valid[ph] && 16 * b + 4 * g4 + i < C;
          if (loss) {
            const float diff = ok ? yo[ph][b][i] - yv[ph][b][i] : 0.f;
            sse_local += diff * diff;
            dz[ph][b][i] = fp32_value<T>((2.0f * GS) * a.dy_scale * diff);
          } else {
            dz[ph][b][i] = ok ? yv[ph][b][i] * GS : 0.f;
          }
        }
      }

    // ---- backward, output layer down to layer 0 ----------------------------------------------------------------------
    v8 dzb[2];
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) dzb[ph] = pack_blocks<T>(dz[ph][0], dz[ph][G::DZB - 1], G::DZB == 2 && cb_n == 2);
#pragma unroll
    for (int l = NL - 1; l >= 0; --l) {
      const int nb = (l == NL - 1) ? cb_n : HB;           // 16-row blocks of dz_l
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
      for (int b = 0; b < G::DZB; ++b) {
        if (b >= nb) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) put_pair16(dz_img, 16 * b + 4 * g4 + i, dzb[0][4 * b + i], dzb[1][4 * b + i]);
      }
      // (1) data gradient: dH_{l-1}^T[in, pix] = W_l[in, :] dz_l  (w0 in the fragments), times the cosine of layer l - 1
      if (l > 0) {
        f32x4 dh[2][HB];
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) {
          const v8 w = W.frag(l == NL - 1 ? G::S_BO + ib : G::S_BH + (l - 1) * HB + ib);
#pragma unroll
          for (int ph = 0; ph < 2; ++ph) dh[ph][ib] = mfma16<T>(w, dzb[ph], zero4());
        }
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            dzb[ph][j] = (T)fp32_value<T>(dh[ph][0][j] * Cf[l - 1][ph][0][j]);
            dzb[ph][4 + j] = HB == 2 ? (T)fp32_value<T>(dh[ph][HB - 1][j] * Cf[l - 1][ph][HB - 1][j]) : (T)0.0f;
          }
        }
      } else if (a.dpe != nullptr) {
#pragma unroll
        for (int eb = 0; eb < G::EB; ++eb) {
          if (eb >= eb_n) continue;
          const v8 w = W.frag(G::S_BE + eb);
#pragma unroll
          for (int ph = 0; ph < 2; ++ph) {
            const f32x4 dx = mfma16<T>(w, dzb[ph], zero4());
            if (!valid[ph]) continue;
            const int e0 = 16 * eb + 4 * g4;
            const long long o = (pe_row + pe_pix_off(a, pix[ph])) * E + e0;
            constexpr float SC = 1.0f / (GS * WS);
            if (a.pe_bf16) {                 // E % 8 == 0: the four channels are all in range or all out
              if (e0 < E) {
                typename Op16<__bf16>::v4 ob = {(__bf16)(dx[0] * SC), (__bf16)(dx[1] * SC), (__bf16)(dx[2] * SC), (__bf16)(dx[3] * SC)};
                *reinterpret_cast<typename Op16<__bf16>::v4*>(reinterpret_cast<__bf16*>(a.dpe) + o) = ob;
              }
            } else if (E % 4 == 0) {
              if (e0 < E) *reinterpret_cast<float4*>(a.dpe + o) = make_float4(dx[0] * SC, dx[1] * SC, dx[2] * SC, dx[3] * SC);
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (e0 + i < E) a.dpe[o + i] = dx[i] * SC;
            }
          }
        }
      }
      // (2) weight gradient: dW_l^T += dz_l^T x input_l over the tile's 32 pixels, from the images
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      v8 av[G::DZB];
#pragma unroll
      for (int b = 0; b < G::DZB; ++b) {
        if (b >= nb) continue;
        av[b] = get_row(dz_img, 16 * b + m);
        gb[l][b] = sum8_16<T>(av[b], gb[l][b]);
      }
      if (l == 0) {
#pragma unroll
        for (int ib = 0; ib < G::IB0; ++ib) {
          if (ib >= ib0) continue;
          const v8 bv = get_row(x_img, 16 * ib + m);
#pragma unroll
          for (int ob = 0; ob < HB; ++ob) gw0[ob][ib] = mfma16<T>(av[ob], bv, gw0[ob][ib]);
        }
      } else {
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) {
          const v8 bv = get_row(s_img(l), 16 * ib + m);
          if (l == NL - 1) {
#pragma unroll
            for (int cb = 0; cb < G::CB; ++cb)
              if (cb < cb_n) gwo[cb][ib] = mfma16<T>(av[cb], bv, gwo[cb][ib]);
          } else {
#pragma unroll
            for (int ob = 0; ob < HB; ++ob) gwh[l - 1][ob][ib] = mfma16<T>(av[ob], bv, gwh[l - 1][ob][ib]);
          }
        }
      }
    }
  }
  if (FWD) return;

  // ---- the row's gradient straight from the accumulators -------------------------------------------------------------
  const long long ro = (long long)chunk * a.G + row;
  float* dst = a.dwvec != nullptr ? a.dwvec + ro * a.w_stride : nullptr;
  auto emit = [&](int idx, float acc) {
    const float v = acc * (1.0f / GS);
    if (dst != nullptr) dst[idx] = v;
    if (a.dw16 != nullptr) {
      const __bf16 hi = (__bf16)v;
      a.dw16[(long long)row * a.dw16_stride + idx] = hi;
      if (a.dwlo != nullptr) a.dwlo[(long long)row * a.dw16_stride + idx] = (__bf16)(v - (float)hi);
    }
  };
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int ob = 0; ob < HB; ++ob) {
      const int out = 16 * ob + 4 * g4 + i;
#pragma unroll
      for (int ib = 0; ib < G::IB0; ++ib) {
        const int in = 16 * ib + m;
        if (ib < ib0 && out < HW && in < IN0) emit(HW + in * HW + out, gw0[ob][ib][i]);
      }
#pragma unroll
      for (int l = 1; l < NH; ++l)
#pragma unroll
        for (int ib = 0; ib < HB; ++ib) {
          const int in = 16 * ib + m;
          if (out < HW && in < HW) emit(loff(l) + HW + in * HW + out, gwh[l - 1][ob][ib][i]);
        }
    }
#pragma unroll
    for (int cb = 0; cb < G::CB; ++cb) {
      const int out = 16 * cb + 4 * g4 + i;
#pragma unroll
      for (int ib = 0; ib < HB; ++ib) {
        const int in = 16 * ib + m;
        if (cb < cb_n && out < C && in < HW) emit(offo + C + in * C + out, gwo[cb][ib][i]);
      }
    }
  }
  // bias gradients: lane (m, g4) holds the sum over pixels 8 g4 .. 8 g4 + 7 of every tile for unit 16 b + m; the four
  // k-groups are added in a fixed order
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int no = l == NL - 1 ? C : HW;
#pragma unroll
    for (int b = 0; b < G::DZB; ++b) {
      float v = gb[l][b];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (g4 == 0 && 16 * b + m < no) emit(loff(l) + 16 * b + m, v);
    }
  }
  if (loss) {
    const float v = wave_sum(sse_local);
    if (lane == 0) a.sse[ro] = v;
  }
}

// up to 4 hidden layers keep the row's weights in registers, 5 to 7 in LDS
template <typename T, int NH, int HW, int KS>
int launch(int mode, const SirenArgs& a, hipStream_t st) {
  using G = Geo<NH, HW, KS>;
  using Store = std::conditional_t<(NH <= 4), RegStore<T, G>, LdsStore<T, G>>;
  const size_t lds = Store::lds_bytes(a.dnet);
  if (mode == MODE_FWD) return siren_launch(siren_rowwave_kernel<T, NH, HW, KS, true, Store>, a.G * a.chunks, 64, lds, 0, "siren(rowwave)", st, a);
  return siren_launch(siren_rowwave_kernel<T, NH, HW, KS, false, Store>, a.G * a.chunks, 64, lds, 0, "siren(rowwave)", st, a);
}

}  // namespace

namespace rcb {
// 16-bit modes, one width for every hidden layer: 1 .. 4 layers of width 16 / 24 (narrow), 5 .. 7 layers of width 16 / 24 / 32
// (deep): RCB_SIREN_ROWWAVE_INSTANCES; siren_route refuses what the family does not take (F, E, C above 32; clock_probe)
int siren_rowwave_launch(int mode, const rcb_siren_desc* d, const SirenRoute& r, SirenArgs& a, hipStream_t st) {
  if (mode == MODE_BWD) a.sse = nullptr;          // the kernel tells loss from backward by the sse pointer
#define RCB_CASE(NHv, HWv, KSv)                                  \
  if (r.p[0] == NHv && r.p[1] == HWv && r.p[2] == KSv)           \
    return d->precision == 2 ? launch<_Float16, NHv, HWv, KSv>(mode, a, st) : launch<__bf16, NHv, HWv, KSv>(mode, a, st);
  RCB_SIREN_ROWWAVE_INSTANCES(RCB_CASE)
#undef RCB_CASE
  return fail(RCB_ERR_UNSUPPORTED, "siren(rowwave): the route names an instance that is not built");
}
}  // namespace rcb
