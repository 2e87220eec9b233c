// Host side of the SIREN kernels, the part that needs no HIP: which descriptors are accepted (siren_check_desc), how large a row
// of layer vectors is (siren_layers), which kernel instances exist (the RCB_SIREN_*_INSTANCES lists) and which of them runs a
// descriptor (siren_route).  Plain C++ over include/rcb.h: the host compiler builds it alone (tests/siren_route_sweep.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/rcb.h"

namespace rcb {

int fail(int code, const char* fmt, ...);   // rcb_common.h; a stand-alone program supplies its own
#ifndef RCB_REQUIRE
#define RCB_REQUIRE(cond, code, ...)            \
  do {                                          \
    if (!(cond)) return rcb::fail((code), __VA_ARGS__); \
  } while (0)
#endif

constexpr int HID = 32;      // hidden width of the matrix-core fp32 kernel and of the workgroup / wave 16-bit kernels
constexpr int MAXL = 5;      // linear layers up to which per-layer widths exist
constexpr int SIREN_MAX_LAYERS = 8;   // linear layers (7 hidden: the A transform's limit)
constexpr int SIREN_MAX_WIDTH = 64;   // hidden width limit

enum { MODE_FWD = 0, MODE_BWD = 1, MODE_LOSS = 2 };

// ---- the layer rule -----------------------------------------------------------------------------------------------------
// linear layer l maps in[l] to out[l] features; its vector [bias(out) | W(in, out)] starts at off[l] of a row of dnet elements
// holding wt weights.  hidden_dims, where given, names the hidden widths one by one.
struct SirenLayers {
  int nl;
  long long in[SIREN_MAX_LAYERS], out[SIREN_MAX_LAYERS], off[SIREN_MAX_LAYERS];
  long long dnet, wt;
};

inline SirenLayers siren_layers(const rcb_siren_desc* d) {   // needs 1 <= n_hidden <= 7
  SirenLayers L;
  L.nl = d->n_hidden + 1;
  L.dnet = L.wt = 0;
  const bool listed = d->hidden_dims[0] != 0;
  for (int l = 0; l < L.nl; ++l) {
    L.in[l] = l == 0 ? d->fourier_dim + d->pe_dim : L.out[l - 1];
    L.out[l] = l == L.nl - 1 ? d->out_dim : (listed && l < 4 ? d->hidden_dims[l] : d->hidden);
    L.off[l] = L.dnet;
    L.dnet += L.out[l] * (L.in[l] + 1);
    L.wt += L.out[l] * L.in[l];
  }
  return L;
}

// ---- the descriptor rule ------------------------------------------------------------------------------------------------
// pe / dpe as patches of stitched grids (rcb_siren_desc.pe_grid_dims): patch counts and sizes right-aligned in three axes
// (unused leading axes are 1), np patches of pp pixels per datapoint
struct SirenPeGrid {
  int pn[3], ps[3];
  long long np, pp;
};

inline SirenPeGrid siren_pe_grid(const rcb_siren_desc* d) {   // needs 1 <= pe_grid_dims <= 3
  SirenPeGrid g;
  g.np = g.pp = 1;
  const int nd = d->pe_grid_dims;
  for (int i = 0; i < 3; ++i) g.pn[i] = g.ps[i] = 1;
  for (int i = 0; i < nd; ++i) {
    g.pn[3 - nd + i] = d->pe_patch_nums[i];
    g.ps[3 - nd + i] = d->pe_patch_size[i];
    g.np *= d->pe_patch_nums[i];
    g.pp *= d->pe_patch_size[i];
  }
  return g;
}

inline int siren_check_desc(const rcb_siren_desc* d, SirenLayers& L) {   // L: siren_layers(d) of an accepted d
  RCB_REQUIRE(d, RCB_ERR_ARG, "siren: null descriptor");
  RCB_REQUIRE(d->hidden == HID || (d->precision >= 1 && (d->hidden == 16 || d->hidden == 24 || d->hidden == 48 || d->hidden == 64)) ||
                  (d->precision == 0 && d->hidden >= 1 && d->hidden <= 64),
              RCB_ERR_UNSUPPORTED, "siren: hidden width %d (fp32 mode: up to 64; 16-bit modes: 16, 24, 32, 48, 64)", d->hidden);
  RCB_REQUIRE(d->n_hidden >= 1 && d->n_hidden <= 7, RCB_ERR_UNSUPPORTED,
              "siren: n_hidden=%d (1..7 hidden layers: the A transform takes up to 8 linear layers)", d->n_hidden);
  RCB_REQUIRE(d->n_hidden <= 4 || d->hidden_dims[0] == 0, RCB_ERR_UNSUPPORTED,
              "siren: per-layer hidden widths exist for 1..4 hidden layers only (5..7 layers take one width)");
  RCB_REQUIRE(d->n_hidden <= 4 || d->precision == 0 || d->hidden == 16 || d->hidden == 24 || d->hidden == HID, RCB_ERR_UNSUPPORTED,
              "siren: hidden width %d at %d hidden layers (16-bit modes: 16, 24 or 32 beyond 4 layers)", d->hidden, d->n_hidden);
  RCB_REQUIRE(d->hidden_dims[0] == 0 || d->precision == 0, RCB_ERR_UNSUPPORTED,
              "siren: per-layer hidden widths exist in the fp32 mode only (the 16-bit kernels take one width: 16, 24, 32, 48 or 64)");
  RCB_REQUIRE(d->out_dim >= 1 && d->out_dim <= 32, RCB_ERR_UNSUPPORTED, "siren: out_dim=%d", d->out_dim);
  RCB_REQUIRE(d->fourier_dim >= 1 && d->pe_dim >= 0 && d->fourier_dim + d->pe_dim <= 64, RCB_ERR_UNSUPPORTED,
              "siren: F=%d E=%d", d->fourier_dim, d->pe_dim);
  RCB_REQUIRE(d->fourier_dim % 2 == 0 && d->pe_dim % 2 == 0, RCB_ERR_UNSUPPORTED, "siren: odd feature dims");
  RCB_REQUIRE(d->n_rows > 0 && d->samples > 0 && d->n_pix > 0 && d->n_rows % d->samples == 0, RCB_ERR_SHAPE,
              "siren: rows=%d samples=%d pix=%d", d->n_rows, d->samples, d->n_pix);
  RCB_REQUIRE(d->precision >= 0 && d->precision <= 2, RCB_ERR_UNSUPPORTED, "siren: precision %d not built", d->precision);
  RCB_REQUIRE((long long)d->n_pix * d->out_dim < (1ll << 31), RCB_ERR_SHAPE, "siren: n_pix x out_dim = %lld elements per row of targets (32-bit offsets inside a row)",
              (long long)d->n_pix * d->out_dim);
  RCB_REQUIRE(d->pe_bf16 == 0 || (d->pe_bf16 == 1 && d->precision >= 1 && d->pe_dim % 8 == 0), RCB_ERR_UNSUPPORTED,
              "siren: bf16 pe storage needs a 16-bit precision mode and pe_dim %% 8 == 0 (precision=%d, E=%d)", d->precision,
              d->pe_dim);
  RCB_REQUIRE(d->dw_bf16 == nullptr || d->precision >= 1, RCB_ERR_UNSUPPORTED,
              "siren: the bf16 copy of the gradient exists in the 16-bit kernels only");
  RCB_REQUIRE(d->dw_lo == nullptr || d->dw_bf16 != nullptr, RCB_ERR_ARG, "siren: dw_lo (low plane) comes with dw_bf16 (high plane)");
  const long long dn = (L = siren_layers(d)).dnet;
  RCB_REQUIRE(d->w_row_stride >= dn, RCB_ERR_SHAPE, "siren: w_row_stride %lld below the %lld elements of a row of layer vectors",
              (long long)d->w_row_stride, dn);
  // (a C caller that sets dw_bf16 but leaves the stride field zero would make every row of the copy overlap)
  RCB_REQUIRE(d->dw_bf16 == nullptr || d->dw_bf16_stride >= dn, RCB_ERR_SHAPE,
              "siren: dw_bf16_stride %lld below the %lld elements of a row of layer vectors", (long long)d->dw_bf16_stride, dn);
  const int chunks = d->pixel_chunks > 1 ? d->pixel_chunks : 1;
  RCB_REQUIRE(chunks == 1 || (d->precision >= 1 && chunks <= (d->n_pix + 31) / 32 && d->dw_bf16 == nullptr &&
                              (long long)d->n_rows * chunks < (1ll << 30)),
              RCB_ERR_UNSUPPORTED,
              "siren: pixel_chunks=%d needs a 16-bit precision mode, at most one chunk per 32-pixel tile and dw_bf16 == NULL "
              "(rcb_siren_reduce_chunks emits it)", d->pixel_chunks);
  if (d->pe_grid_dims != 0) {
    const int nd = d->pe_grid_dims;
    RCB_REQUIRE(nd >= 1 && nd <= 3 && d->precision >= 1 && d->pe_dim > 0, RCB_ERR_UNSUPPORTED,
                "siren: pe_grid_dims=%d (1..3, 16-bit kernels, pe_dim > 0)", nd);
    for (int i = 0; i < nd; ++i)
      RCB_REQUIRE(d->pe_patch_nums[i] >= 1 && d->pe_patch_size[i] >= 1, RCB_ERR_SHAPE, "siren: stitched pe axis %d: %d x %d", i,
                  d->pe_patch_nums[i], d->pe_patch_size[i]);
    const SirenPeGrid g = siren_pe_grid(d);
    RCB_REQUIRE(g.pp == d->n_pix && (d->n_rows / d->samples) % g.np == 0 && g.pp * 4096 < (1ll << 32) && g.ps[1] <= 4096 &&
                    g.ps[2] <= 4096,
                RCB_ERR_SHAPE, "siren: stitched pe layout: patch of %lld pixels for n_pix=%d, %lld patches per datapoint for %d INRs",
                g.pp, d->n_pix, g.np, d->n_rows / d->samples);
  }
  return RCB_OK;
}

// ---- the instances ------------------------------------------------------------------------------------------------------
// fp32 on the matrix cores, width 32 (siren_mlp.hip): X(NH, KS, NB) runs NH hidden layers with max(F, E) <= KS and
// ceil((F + E) / 32) == NB; the first match in this order
#define RCB_SIREN_FP32_INSTANCES(X) X(3, 16, 1) X(2, 16, 1) X(3, 18, 2) X(1, 16, 1) X(4, 16, 1) X(3, 32, 2)
// 16-bit, width 32, one workgroup per row (siren_mlp_bf16.hip): X(NH, F, E, C) -- cifar / kodak / protein, audio, video, and the
// first at 2 hidden layers
#define RCB_SIREN_WG_INSTANCES(X) X(3, 16, 16, 3) X(3, 16, 16, 1) X(3, 18, 16, 3) X(2, 16, 16, 3)
// 16-bit, width 32, loss / backward, one wave per row (siren_mlp_wave.hip): X(NH, F, E, C)
#define RCB_SIREN_WAVE_INSTANCES(X) X(3, 16, 16, 3)
// 16-bit, dealt gradient tiles (siren_mlp_wide.hip): X(NH, F, E, C, W)
#ifdef RCB_SIREN_DEALT32
// width 32 on this kernel (wave l owns layer l's gradient tile, three workgroups per CU): measured 0.284 ms against the
// 0.25 ms of siren_mlp_bf16.hip in the same back-to-back loop (4096 x 1024 px) -- eight barriers per pass are too many for
// its short layers -- so these instances are only built on request (-DRCB_SIREN_DEALT32, selected by RCB_SIREN_W32_DEALT=1)
#define RCB_SIREN_WIDE_DEALT32(X) X(3, 16, 16, 3, 32) X(3, 16, 16, 1, 32) X(3, 18, 16, 3, 32) X(2, 16, 16, 3, 32)
#else
#define RCB_SIREN_WIDE_DEALT32(X)
#endif
// kodak / cifar / protein geometry at width 48 and 64, video and audio geometry at width 64
#define RCB_SIREN_WIDE_INSTANCES(X) \
  RCB_SIREN_WIDE_DEALT32(X) X(3, 16, 16, 3, 48) X(3, 16, 16, 3, 64) X(3, 18, 16, 3, 64) X(3, 16, 16, 1, 64)
// 16-bit, one wave per row at one width for every hidden layer (siren_mlp_rowwave.hip): X(NH, HW, KS) -- 1 .. 4 layers of
// width 16 / 24 (1 .. 4 layers of width 32 belong to the workgroup and wave families), 5 .. 7 layers of width 16 / 24 / 32;
// KS = 1 while F, E and C are at most 16 each, 2 up to 32
#define RCB_SIREN_ROWWAVE_KS(X, KS)                                                                                          \
  X(1, 16, KS) X(2, 16, KS) X(3, 16, KS) X(4, 16, KS) X(5, 16, KS) X(6, 16, KS) X(7, 16, KS) X(1, 24, KS) X(2, 24, KS)       \
  X(3, 24, KS) X(4, 24, KS) X(5, 24, KS) X(6, 24, KS) X(7, 24, KS) X(5, 32, KS) X(6, 32, KS) X(7, 32, KS)
#define RCB_SIREN_ROWWAVE_INSTANCES(X) RCB_SIREN_ROWWAVE_KS(X, 1) RCB_SIREN_ROWWAVE_KS(X, 2)

// both input halves as 16-bit rows (kernel template argument IN16): the fused loss only, pe stored as bf16, a 16-bit copy of xf
// supplied, and a pe half of whole 8-feature groups
constexpr bool siren_can16(int E) { return E % 8 == 0 && E > 0; }

// ---- the route ----------------------------------------------------------------------------------------------------------
enum SirenFamily {
  SIREN_REFUSED = 0,   // code / text
  SIREN_FP32,          // p = NH, KS, NB
  SIREN_GENERIC,       // p = ML: the layer capacity of the instance (MAXL or SIREN_MAX_LAYERS)
  SIREN_WG,            // p = NH, F, E, C; in16
  SIREN_WAVE,          // p = NH, F, E, C; dpe
  SIREN_WIDE,          // p = NH, F, E, C, W; in16
  SIREN_ROWWAVE,       // p = NH, HW, KS
};

struct SirenRoute {
  int family;
  int p[5], n_cu;
  bool in16, dpe;
  int code;
  char text[224];
};

// The kernel that runs a descriptor siren_check_desc accepted.  in16_rows: pe is bf16 and a 16-bit copy of xf is given;
// wave_variant: rcb_debug_siren_wave_tiles; n_cu: compute units of the device; dealt32: RCB_SIREN_W32_DEALT in a
// -DRCB_SIREN_DEALT32 build (ignored otherwise)
inline SirenRoute siren_route(const rcb_siren_desc* d, int mode, bool has_dpe, bool in16_rows, int wave_variant, int n_cu,
                              [[maybe_unused]] bool dealt32 = false) {
  SirenRoute r;
  r.family = SIREN_REFUSED, r.in16 = r.dpe = false, r.code = RCB_ERR_UNSUPPORTED, r.n_cu = n_cu, r.text[0] = 0;
  r.p[0] = r.p[1] = r.p[2] = r.p[3] = r.p[4] = 0;
  const int nh = d->n_hidden, hw = d->hidden, F = d->fourier_dim, E = d->pe_dim, C = d->out_dim;
  auto named = [&r](int family, int p0, int p1, int p2, int p3, int p4) {
    r.family = family;
    r.p[0] = p0, r.p[1] = p1, r.p[2] = p2, r.p[3] = p3, r.p[4] = p4;
  };
#define RCB_REFUSE(...) snprintf(r.text, sizeof(r.text), __VA_ARGS__)

  // 16-bit modes, one wave per row: uniform hidden width 16 or 24 at 1 .. 4 hidden layers, and every descriptor of 5 .. 7
  if (d->precision >= 1 && (nh >= 5 || ((hw == 16 || hw == 24) && d->hidden_dims[0] == 0))) {
    const char* fam = nh >= 5 ? "deep" : "narrow";
    if (!(F <= 32 && E <= 32 && C <= 32))
      RCB_REFUSE("siren(%s): F=%d E=%d C=%d (the one-wave-per-row kernels take up to 32 features from each input half and 32 outputs)",
                 fam, F, E, C);
    else if (d->clock_probe != nullptr)
      RCB_REFUSE("siren(%s): clock_probe exists in the width-32 kernel of 1..4 layers only", fam);
    else
      named(SIREN_ROWWAVE, nh, hw, (F <= 16 && E <= 16 && C <= 16) ? 1 : 2, 0, 0);
    return r;
  }

  if (d->precision >= 1) {
    bool wide = hw > HID;
#ifdef RCB_SIREN_DEALT32
    wide = wide || (dealt32 && mode != MODE_FWD);
#endif
    r.in16 = siren_can16(E) && in16_rows && mode == MODE_LOSS;
    if (wide) {
#define RCB_X(NHv, Fv, Ev, Cv, Wv) \
  if (nh == NHv && F == Fv && E == Ev && C == Cv && hw == Wv) return named(SIREN_WIDE, NHv, Fv, Ev, Cv, Wv), r;
      RCB_SIREN_WIDE_INSTANCES(RCB_X)
#undef RCB_X
      RCB_REFUSE("siren(wide): geometry n_hidden=%d F=%d E=%d C=%d width=%d is not instantiated", nh, F, E, C, hw);
      return r;
    }
    if (wave_variant > 0 && mode != MODE_FWD && d->precision == 1 && in16_rows && hw == HID && (d->n_pix & 31) == 0 &&
        d->pe_grid_dims == 0) {
      // A wave walks whole rows: the launch is as long as the wave with the most rows.  Unless the (row, chunk) units fill the
      // resident waves (two 4-wave workgroups per CU) to 90 % in the last round, the workgroup family -- four waves per row,
      // any number of rows -- is the better fit (the test-time batches: 500 images x 5 samples = 2500 rows on 2048 waves).
      const long long units = (long long)d->n_rows * (d->pixel_chunks > 1 ? d->pixel_chunks : 1), waves = 8ll * n_cu;
      const long long rounds = (units + waves - 1) / waves;
      if (wave_variant == 2 || units * 10 >= rounds * waves * 9) {      // (2: forced, tests)
#define RCB_X(NHv, Fv, Ev, Cv) \
  if (nh == NHv && F == Fv && E == Ev && C == Cv) return r.in16 = false, r.dpe = has_dpe, named(SIREN_WAVE, NHv, Fv, Ev, Cv, 0), r;
        RCB_SIREN_WAVE_INSTANCES(RCB_X)
#undef RCB_X
      }
    }
#define RCB_X(NHv, Fv, Ev, Cv) \
  if (nh == NHv && F == Fv && E == Ev && C == Cv) return named(SIREN_WG, NHv, Fv, Ev, Cv, 0), r;
    RCB_SIREN_WG_INSTANCES(RCB_X)
#undef RCB_X
    RCB_REFUSE("siren(bf16): geometry n_hidden=%d F=%d E=%d C=%d is not instantiated", nh, F, E, C);
    return r;
  }

  // fp32: width 32 of 1 .. 4 layers on the matrix cores; other widths, per-layer widths and 5 .. 7 layers on the plain-FMA kernel
  if (hw != HID || d->hidden_dims[0] != 0 || nh > 4) {
    const SirenLayers L = siren_layers(d);
    for (int l = 0; l < nh; ++l)
      if (!(L.out[l] >= 1 && L.out[l] <= SIREN_MAX_WIDTH)) {
        RCB_REFUSE("siren(generic fp32): hidden layer %d is %d wide (1..%d)", l, (int)L.out[l], SIREN_MAX_WIDTH);
        return r;
      }
    named(SIREN_GENERIC, nh + 1 > MAXL ? SIREN_MAX_LAYERS : MAXL, 0, 0, 0, 0);
    return r;
  }
  const int ks = F > E ? F : E, nb0 = (F + E + 31) / 32;
#define RCB_X(NHv, KSv, NBv) \
  if (nh == NHv && ks <= KSv && nb0 == NBv) return named(SIREN_FP32, NHv, KSv, NBv, 0, 0), r;
  RCB_SIREN_FP32_INSTANCES(RCB_X)
#undef RCB_X
  RCB_REFUSE("siren: no kernel for n_hidden=%d, F=%d, E=%d", nh, F, E);
  return r;
#undef RCB_REFUSE
}

}  // namespace rcb
