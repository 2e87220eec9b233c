// N4: the one index rule of the whole-signal entries (recon.hip: rcb_recon_finish and its _crop / _fmt / _ragged forms; signal.hip:
// rcb_signal_patch and its _pad / _fmt / _ragged forms; recon_regions.hip: rcb_recon_regions, which goes the other way, from a grid
// position to its run).  A signal lies on the grid G_i = pn[i] * ps[i]; its y [per][P][C] holds patch after patch
// (b0 b1 b2 row-major), each patch pixel after pixel (p0 p1 p2 row-major), so the R = ps[2] * C elements of a patch row are
// contiguous: a run.  Run number r of a signal counts (b0, b1, b2, p0, p1) row-major and lies at grid position g_i = b_i * ps_i + p_i,
// its element `off` at e = b2 * R + off of the grid row (g0, g1).  Both files cut a signal into chunks of kChunk elements, one
// workgroup each, thread t owning the quads t, t + 256, ... of its chunk.
#pragma once
#include "rcb_common.h"

namespace rcb {

constexpr int kThreads = 256;
constexpr int kQuadsPerThread = 8;
constexpr int kChunk = kThreads * 4 * kQuadsPerThread;      // 8192 elements of one signal per workgroup

struct PatchGeo {
  int pn[3], ps[3];       // patches per axis / pixels per axis of a patch, right-aligned (leading axes 1)
  int C;                  // channels
  int R;                  // elements of one run: ps[2] * C
  int E;                  // elements of one signal on the grid
  int n_chunks;           // ceil(E / kChunk)
  // the signal's own extent inside the grid (the _pad / _crop entries; the others never read it)
  int sz[3];              // positions per axis, right-aligned (leading axes 1)
  int L;                  // existing elements of one grid row: sz[2] * C
};

// run `run` of a signal -> its grid row (g0, g1) and its patch b2 along the last axis.  CLIP: the row the edge-padded signal
// takes it from, min(g_i, sz[i] - 1).
template <bool CLIP>
__device__ __forceinline__ void decode_run(const PatchGeo& g, int run, int& g0, int& g1, int& b2) {
  int r = run;
  const int p1 = r % g.ps[1]; r /= g.ps[1];
  const int p0 = r % g.ps[0]; r /= g.ps[0];
  b2 = r % g.pn[2]; r /= g.pn[2];
  const int b1 = r % g.pn[1];
  const int b0 = r / g.pn[1];
  g0 = b0 * g.ps[0] + p0;
  g1 = b1 * g.ps[1] + p1;
  if (CLIP) {
    g0 = min(g0, g.sz[0] - 1);
    g1 = min(g1, g.sz[1] - 1);
  }
}

// The inverse (recon_regions.hip, which walks boxes of the signal and gathers from y): the grid row (g0, g1) and the patch b2
// along the last axis -> the run that decode_run<false> maps there.  Element e = b2 * R + off of that grid row lies at
// encode_run(g, g0, g1, e / R) * R + e % R of the signal's y; a run number is below E / R, so it fits an int.
__device__ __forceinline__ int encode_run(const PatchGeo& g, int g0, int g1, int b2) {
  const int b0 = g0 / g.ps[0], p0 = g0 % g.ps[0];
  const int b1 = g1 / g.ps[1], p1 = g1 % g.ps[1];
  return (((b0 * g.pn[1] + b1) * g.pn[2] + b2) * g.ps[0] + p0) * g.ps[1] + p1;
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// The axes of g from the caller's arrays of nd entries, validated axis by axis; per = prod(patch_nums), P = prod(patch_size).
// `size` null: the extent is the grid.  axis_stride (the signal entries; null for the recon entries) is only checked here, and
// selects how the 2^31 limit is worded: per signal, or per factor with the product left to the caller's own checks.
inline int grid_axes(const char* who, int nd, const int32_t* patch_nums, const int32_t* patch_size, const int32_t* size,
                     const int64_t* axis_stride, PatchGeo& g, long long& per, long long& P) {
  per = P = 1;
  for (int i = 0; i < 3; ++i) g.pn[i] = g.ps[i] = g.sz[i] = 1;
  for (int i = 0; i < nd; ++i) {
    RCB_REQUIRE(patch_nums[i] > 0 && patch_size[i] > 0, RCB_ERR_SHAPE, "%s: axis %d has %d patches of %d pixels", who, i,
                patch_nums[i], patch_size[i]);
    if (axis_stride)
      RCB_REQUIRE(axis_stride[i] >= 0, RCB_ERR_ARG, "%s: negative stride %lld of axis %d", who, (long long)axis_stride[i], i);
    g.pn[3 - nd + i] = patch_nums[i];
    g.ps[3 - nd + i] = patch_size[i];
    const long long G = (long long)patch_nums[i] * patch_size[i], pix = per * P;
    per *= patch_nums[i];
    P *= patch_size[i];
    if (axis_stride)
      RCB_REQUIRE(G <= 0x7fffffffLL && pix * G <= 0x7fffffffLL, RCB_ERR_UNSUPPORTED,
                  "%s: more than 2^31 - 1 elements per signal", who);          // (pix, G < 2^31: the product fits 64 bits)
    else
      RCB_REQUIRE(per <= 0x7fffffffLL && P <= 0x7fffffffLL, RCB_ERR_SHAPE, "%s: patch geometry overflows", who);
    RCB_REQUIRE(!size || (size[i] >= 1 && size[i] <= G), RCB_ERR_SHAPE, "%s: axis %d of the signal has %d positions (1 .. %lld)", who,
                i, size ? size[i] : 0, G);
    g.sz[3 - nd + i] = size ? size[i] : (int)G;
  }
  return RCB_OK;
}

// the element counts of g, once the caller has held E = per * P * channels to 2^31 - 1 in its own words
inline void grid_elems(PatchGeo& g, int channels, long long E) {
  g.C = channels;
  g.R = g.ps[2] * channels;
  g.E = (int)E;
  g.n_chunks = (int)((E + kChunk - 1) / kChunk);
  g.L = g.sz[2] * channels;
}

// ---- the per-signal ("ragged") entries (rcb_signal_patch_ragged, rcb_recon_finish_ragged) ---------------------------------
// One row of the device table per signal: where the by-value geometry of the other entries holds one extent (sz, L) and one set of
// strides for the whole launch, a workgroup of these entries takes them from the row of its signal.
struct RaggedRow {
  long long off;          // the signal's first element, from the base pointer of the call
  long long as[3];        // strides of the axes in elements, right-aligned (leading 0)
  int sz[3];              // positions per axis, right-aligned (leading 1)
  int flags;              // kRagged*: the memory path of this signal, decided by the host entry
};
constexpr int kRaggedQuad = 1;    // a quad inside the extent is 4 consecutive, aligned elements on the signal's side: one load / store
constexpr int kRaggedDense = 2;   // (recon) the last axis is the innermost one: element e of a grid row lies e elements on

// the geometry of one signal: g with the row's extent
__device__ __forceinline__ PatchGeo ragged_geo(const PatchGeo& g, const RaggedRow& r) {
  PatchGeo o = g;
  o.sz[0] = r.sz[0]; o.sz[1] = r.sz[1]; o.sz[2] = r.sz[2];
  o.L = r.sz[2] * g.C;
  return o;
}

// The host tables -> rows (no flags yet), validated: `sizes` [n_data][3] against the grid of g, `spans` [n_data][4] non-negative.
// reach[d]: offset of the farthest element of signal d with channel stride cs.
inline int ragged_rows(const char* who, long long n_data, int nd, const PatchGeo& g, int channels, long long cs, const int32_t* sizes,
                       const int64_t* spans, RaggedRow* rows, long long* reach) {
  for (long long d = 0; d < n_data; ++d) {
    RaggedRow& r = rows[d];
    r.off = spans[4 * d];
    r.flags = 0;
    RCB_REQUIRE(r.off >= 0, RCB_ERR_ARG, "%s: signal %lld has the negative offset %lld", who, d, r.off);
    long long far = r.off;
    bool fits = true;
    for (int i = 0; i < 3; ++i) {
      const int a = i - (3 - nd);                            // the caller's axis, or < 0: a leading axis of one position
      r.sz[i] = a < 0 ? 1 : sizes[3 * d + a];
      r.as[i] = a < 0 ? 0 : spans[4 * d + 1 + a];
      const long long G = (long long)g.pn[i] * g.ps[i];
      RCB_REQUIRE(r.sz[i] >= 1 && r.sz[i] <= G, RCB_ERR_SHAPE, "%s: axis %d of signal %lld has %d positions (1 .. %lld)", who, a, d,
                  r.sz[i], G);
      RCB_REQUIRE(r.as[i] >= 0, RCB_ERR_ARG, "%s: negative stride %lld of axis %d of signal %lld", who, r.as[i], a, d);
      // (sz - 1) * stride + far without overflow: a reach beyond 2^62 fits no buffer
      if (r.sz[i] > 1 && r.as[i] > ((1LL << 62) - far) / (r.sz[i] - 1)) fits = false;
      else far += (r.sz[i] - 1) * r.as[i];
    }
    if (channels > 1 && cs > ((1LL << 62) - far) / (channels - 1)) fits = false;
    else far += (channels - 1) * cs;
    reach[d] = fits ? far : (1LL << 62);
  }
  return RCB_OK;
}

// the rows -> the device table, on `st`, which is synchronised: the host rows may be freed on return
inline int ragged_upload(const char* who, const RaggedRow* rows, long long n_data, void* table, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(table, rows, (size_t)n_data * sizeof(RaggedRow), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail((int)e, "%s: table upload failed: %s", who, hipGetErrorString(e));
  return RCB_OK;
}

}  // namespace rcb
