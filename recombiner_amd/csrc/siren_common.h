// Declarations shared by the SIREN kernels: the kernel argument block, the pe addressing, and the one launcher.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "rcb_common.h"
#include "siren_route.h"   // HID, MAXL, MODE_*, the descriptor / layer / route rules

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace rcb {

constexpr int TS = 36;       // LDS tile row stride in floats (32 + 4 pad: conflict-free b128 reads)

struct SirenArgs {
  const float* xf;
  const float* pe;
  const float* wvec;
  const float* yin;   // MODE_LOSS: target [N,P,C];  MODE_BWD: dy [G,P,C]
  float* yout;        // MODE_FWD: [G,P,C]
  float* sse;         // MODE_LOSS: [G]
  float* dwvec;       // [G, w_stride]
  float* dpe;         // [G,P,E] or null
  long long xf_stride, w_stride;
  int G, S, P, F, E, C;
  int dnet, wt_total, tile_base, smem_floats;
  float k_hi, k_lo;   // w0 / (2 pi) split in two floats
  float w0, dy_scale;
  int pe_bf16;        // pe / dpe hold bf16 elements (16-bit kernels only)
  __bf16* dw16;       // nullable: bf16 copy of dwvec, rows dw16_stride elements apart (rcb_siren_desc.dw_bf16)
  __bf16* dwlo;       // nullable (with dw16): the low plane bf16(dwvec - dw16), same layout; dwvec may then be NULL
  long long dw16_stride;
  int chunks;         // >= 1: workgroups per row of wvec (pixel tiles split; dwvec / sse hold per-chunk partials)
  const void* xf16;   // nullable: 16-bit copy of xf in the operand format, rows padded to 8 features (rcb_siren_desc.xf_bf16)
  unsigned long long* clock_probe;   // nullable: rcb_siren_desc.clock_probe
  // pe / dpe layout (rcb_siren_desc.pe_grid_dims): 0 = [G][P][E]; else the rows are the patches of stitched grids
  // [images][G0][G1][G2][E], G_i = pe_pn[i] * pe_ps[i] (unused leading axes are 1), image = sample * pe_ndc + datapoint
  int pe_nd, pe_ndc;
  int pe_pn[3], pe_ps[3];
  unsigned pe_m1, pe_m2;   // ceil(2^32 / pe_ps[1]), ceil(2^32 / pe_ps[2]): exact quotients for p * ps < 2^32
};

// pixel index (to be multiplied by E) of pixel 0 of row g in the pe / dpe array, and of pixel p relative to it
__device__ __forceinline__ long long pe_row_base(const SirenArgs& a, int g) {
  if (a.pe_nd == 0) return (long long)g * a.P;
  const int n = g / a.S, s = g - n * a.S;
  const int np = a.pe_pn[0] * a.pe_pn[1] * a.pe_pn[2];
  const int d = n / np;
  int pl = n - d * np;
  const int c2 = pl % a.pe_pn[2];
  pl /= a.pe_pn[2];
  const int c1 = pl % a.pe_pn[1], c0 = pl / a.pe_pn[1];
  const long long img = (long long)s * a.pe_ndc + d;
  const int G0 = a.pe_pn[0] * a.pe_ps[0], G1 = a.pe_pn[1] * a.pe_ps[1], G2 = a.pe_pn[2] * a.pe_ps[2];
  return ((img * G0 + c0 * a.pe_ps[0]) * G1 + c1 * a.pe_ps[1]) * G2 + c2 * a.pe_ps[2];
}
__device__ __forceinline__ int pe_pix_off(const SirenArgs& a, int p) {
  if (a.pe_nd == 0) return p;
  // (an axis of one pixel has no 32-bit reciprocal: its quotient is the dividend)
  const unsigned t = a.pe_ps[2] == 1 ? (unsigned)p : __umulhi((unsigned)p, a.pe_m2), y2 = (unsigned)p - t * (unsigned)a.pe_ps[2];
  const unsigned y0 = a.pe_ps[1] == 1 ? t : __umulhi(t, a.pe_m1), y1 = t - y0 * (unsigned)a.pe_ps[1];
  const int G1 = a.pe_pn[1] * a.pe_ps[1], G2 = a.pe_pn[2] * a.pe_ps[2];
  return (int)((y0 * G1 + y1) * G2 + y2);
}

// row of accumulator register r for lane half h (32x32 MFMA C/D layout)
__device__ __forceinline__ constexpr int rho(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 mfma2(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}


// ---- launching (the route: siren_route.h; the one entry body that routes and calls these: siren_mlp.hip) ------------------
// one launcher per family, in its kernel file: the instance the route names with that family's grid and LDS bytes, nothing else
using SirenLaunch = int(int mode, const rcb_siren_desc* d, const SirenRoute& r, SirenArgs& a, hipStream_t st);
SirenLaunch siren_fp32_launch, siren_generic_launch, siren_bf16_launch, siren_wave_launch, siren_wide_launch, siren_rowwave_launch;
int& siren_wave_tiles();      // 1: one wave per row where instantiated, 0: the workgroup kernel everywhere (rcb_debug_siren_wave_tiles)

constexpr int SIREN_LDS_MAX = 160 * 1024;

// Set the LDS limit (attr_bytes > 0; per launch: the attribute belongs to the (function, device) pair, a process may drive
// several devices or call from several threads, and the call is a table write), launch, check.
template <class K, class... A>
int siren_launch(K kernel, unsigned grid, unsigned block, size_t lds_bytes, int attr_bytes, const char* tag, hipStream_t st,
                 const A&... args) {
  if (attr_bytes > 0) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, attr_bytes);
    if (e != hipSuccess) return fail((int)e, "%s: hipFuncSetAttribute: %s", tag, hipGetErrorString(e));
  }
  kernel<<<grid, block, lds_bytes, st>>>(args...);
  RCB_LAUNCH_CHECK();
  return RCB_OK;
}

// The instances of one geometry of the workgroup and wide families: forward, backward, loss, and the loss with both input
// halves as 16-bit rows (siren_can16; route.in16).  launch(mode_c, in16_c) launches the instance of those two constants.
template <int E, class L>
int siren_launch_mode(int mode, bool in16, L&& launch) {
  constexpr bool can16 = siren_can16(E);
  if (can16 && in16 && mode == MODE_LOSS) return launch(std::integral_constant<int, MODE_LOSS>{}, std::integral_constant<bool, can16>{});
  if (mode == MODE_FWD) return launch(std::integral_constant<int, MODE_FWD>{}, std::false_type{});
  if (mode == MODE_BWD) return launch(std::integral_constant<int, MODE_BWD>{}, std::false_type{});
  return launch(std::integral_constant<int, MODE_LOSS>{}, std::false_type{});
}

// compute units of the current device (cached per device: a process may drive several)
inline int cu_count() {
  static int n_cu[64];
  int dev_id = 0;
  if (hipGetDevice(&dev_id) != hipSuccess || dev_id < 0 || dev_id >= 64) dev_id = 0;
  if (n_cu[dev_id] == 0) {
    hipDeviceProp_t prop;
    n_cu[dev_id] = (hipGetDeviceProperties(&prop, dev_id) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
  }
  return n_cu[dev_id];
}

}  // namespace rcb
