// N4 (417): the distortion figure by REGION -- per frame, per patch, per tile -- on the device.  rcb_recon_regions reads what
// rcb_recon_finish_fmt reads, the reconstruction y [N][P][C] in patch order and its target, and writes per datapoint and per box of
// the signal's extent the fp64 sum of squared errors and the count of non-finite elements; nothing else.
//
// Regions tile the EXTENT sz (not the grid): nr[i] = ceil(sz[i] / region[i]) boxes per axis, box r_i = [r_i * region[i],
// min((r_i + 1) * region[i], sz[i])), the region index row-major over (r0, r1, r2).  A box on the far edge is smaller; padding
// belongs to no box and is never loaded.  The elements of a box are its positions row-major with the channels innermost -- the
// order of the whole signal, not the patch order of y -- s = ((p0 * box1 + p1) * box2 + p2) * C + c, n_r of them.
//
// The sum of a box is rcb_recon_finish's sum of a datapoint of n_r elements, addition for addition: chunks of kChunk elements, one
// workgroup each; thread t owns the quads t, t + 256, ... of its chunk in element order; block_sum; then the chunk partials as
// recon_reduce_kernel adds them (thread t: partials t, t + 256, ..., block_sum).  What an element is and what it adds are
// recon_elem.h's, the source recon.hip compiles.  So sse_r[d][r] is bitwise the sse of rcb_recon_finish_fmt (nd = 0) on the box's
// values copied out contiguously, whatever the batch, the launch or the memory path.
//
// Launch: one workgroup per (datapoint, region, chunk), max_chunks = the chunks of the largest box of the call; the surplus
// workgroups of a smaller box exit before they load or write anything, and the reduce kernel reads each box's own chunk count.
// Datapoint, region and chunk come from blockIdx alone, so the box, its origin and every divisor below are workgroup-uniform.
//
// Memory: a quad is 4 consecutive box elements.  When box rows, the origins of the boxes and the runs of y all fall on 4-element
// boundaries -- min(region, sz)[last] * C, sz[last] * C and R = patch_size[last] * C multiples of 4 -- and both pointers are 16-byte
// aligned, a quad lies inside one run of y: one 16-byte load per input and ONE position -> (patch, pixel) inversion
// (patch_grid.h: encode_run) per quad.  Otherwise the same quads go element by element.  The kernel is a gather bounded by the
// bytes of y and target inside the extent; the only LDS is block_sum's, no scratch, no atomics.
#include <algorithm>

#include "recon_elem.h"

#pragma clang fp contract(off)

using namespace rcb;

namespace {

struct RegionGeo {
  PatchGeo g;
  int mode;
  SampleRule16 rule;      // modes 2 and 3
  int reg[3];             // positions per axis of a full box: min(region[i], sz[i]), right-aligned (leading axes 1)
  int nr[3];              // boxes per axis
  int n_regions;          // their product
  int max_chunks;         // chunks of the largest box: the workgroups every (datapoint, region) has
};

// box `r` of the extent: its origin o and its size b per axis -> its elements n_r (<= E)
__device__ __forceinline__ int region_box(const RegionGeo& x, int r, int (&o)[3], int (&b)[3]) {
  const int r2 = r % x.nr[2];
  r /= x.nr[2];
  const int ri[3] = {r / x.nr[1], r % x.nr[1], r2};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o[i] = ri[i] * x.reg[i];                               // (< sz[i])
    b[i] = min(x.reg[i], x.g.sz[i] - o[i]);
  }
  return b[0] * b[1] * b[2] * x.g.C;
}

// element s of the box (o, b), Lr = b[2] * C of them per box row -> its offset inside the signal's y
__device__ __forceinline__ int box_offset(const PatchGeo& g, const int (&o)[3], const int (&b)[3], int Lr, int s) {
  const int row = s / Lr;
  const int e = o[2] * g.C + s % Lr;                       // element of the grid row (g0, g1)
  const int g0 = o[0] + row / b[1], g1 = o[1] + row % b[1];
  return encode_run(g, g0, g1, e / g.R) * g.R + e % g.R;   // (< E)
}

template <bool VEC, bool W16>
__global__ void __launch_bounds__(kThreads) regions_kernel(const float* __restrict__ y, const float* __restrict__ target,
                                                           double* __restrict__ part_sse, int* __restrict__ part_bad, RegionGeo x) {
  const long long blk = blockIdx.x;
  const int chunk = (int)(blk % x.max_chunks);
  const long long dr = blk / x.max_chunks;
  const int r = (int)(dr % x.n_regions);
  const long long d = dr / x.n_regions;
  int o[3], b[3];
  const int n_r = region_box(x, r, o, b);
  if ((long long)chunk * kChunk >= n_r) return;            // a smaller box has fewer chunks (uniform: the whole workgroup leaves)
  const PatchGeo& g = x.g;
  const long long base = d * (long long)g.E;
  const float* yd = y + base;
  const float* td = target ? target + base : nullptr;
  const int Lr = b[2] * g.C;
  double acc = 0.0;
  int bad = 0;
  for (int it = 0; it < kQuadsPerThread; ++it) {
    const long long s0l = (long long)chunk * kChunk + ((long long)it * kThreads + threadIdx.x) * 4;
    if (s0l >= n_r) break;
    const int s0 = (int)s0l;
    float xs[4], t[4] = {0.f, 0.f, 0.f, 0.f};
    int n = 4;
    if (VEC) {                                             // n_r % 4 == 0 and the quad lies inside one run of y
      const int off = box_offset(g, o, b, Lr, s0);
      const float4 xv = *reinterpret_cast<const float4*>(yd + off);
      xs[0] = xv.x; xs[1] = xv.y; xs[2] = xv.z; xs[3] = xv.w;
      if (td) {
        const float4 tv = *reinterpret_cast<const float4*>(td + off);
        t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
      }
    } else {
      n = n_r - s0 < 4 ? n_r - s0 : 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int off = k < n ? box_offset(g, o, b, Lr, s0 + k) : 0;
        xs[k] = k < n ? yd[off] : 0.0f;
        if (td) t[k] = k < n ? td[off] : 0.0f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const Elem e = W16 ? finish16(xs[k], x.rule.scale, x.rule.cap, x.rule.bias) : finish(xs[k], x.mode);
      if (k < n) RCB_RECON_ADD_TERM(e, t[k], true, acc, bad);
    }
  }
  if (block_sum(acc, bad)) {
    part_sse[blk] = acc;
    part_bad[blk] = bad;
  }
}

// one workgroup per (datapoint, region): the box's own chunk partials in recon_reduce_kernel's order
__global__ void __launch_bounds__(kThreads) regions_reduce_kernel(const double* __restrict__ part_sse,
                                                                  const int* __restrict__ part_bad, RegionGeo x,
                                                                  double* __restrict__ sse_r, int* __restrict__ n_bad_r) {
  const long long dr = blockIdx.x;
  int o[3], b[3];
  const int n_r = region_box(x, (int)(dr % x.n_regions), o, b);
  const int n_chunks = (int)(((long long)n_r + kChunk - 1) / kChunk);
  double acc = 0.0;
  int bad = 0;
  for (int c = threadIdx.x; c < n_chunks; c += kThreads) {
    acc += part_sse[dr * x.max_chunks + c];
    bad += part_bad[dr * x.max_chunks + c];
  }
  if (block_sum(acc, bad)) {
    if (sse_r) sse_r[dr] = bad ? __builtin_nan("") : acc;
    if (n_bad_r) n_bad_r[dr] = bad;
  }
}

using RegionsKernel = void (*)(const float*, const float*, double*, int*, RegionGeo);

static RegionsKernel regions_kernel_of(bool vec, bool w16) {
  if (w16) return vec ? regions_kernel<true, true> : regions_kernel<false, true>;
  return vec ? regions_kernel<true, false> : regions_kernel<false, false>;
}

}  // namespace

extern "C" int64_t rcb_recon_regions_workspace_bytes(int64_t n_data, int64_t n_regions, int64_t max_region_elems) {
  if (n_data <= 0 || n_regions <= 0 || n_regions > 0x7fffffffLL || max_region_elems <= 0 || max_region_elems > 0x7fffffffLL)
    return -1;
  const int64_t max_chunks = (max_region_elems + kChunk - 1) / kChunk;
  if (n_regions > 0x7fffffffLL / max_chunks) return -1;
  const int64_t per_data = n_regions * max_chunks;
  if (n_data > 0x7fffffffLL / per_data) return -1;
  return n_data * per_data * (int64_t)(sizeof(double) + sizeof(int));
}

extern "C" int rcb_recon_regions(const float* y, const float* target, int64_t n_rows, int32_t n_pix, int32_t channels, int32_t nd,
                                 const int32_t* patch_nums, const int32_t* patch_size, const int32_t* size, const int32_t* region,
                                 int32_t mode, int32_t depth, double* sse_r, int32_t* n_bad_r, void* workspace,
                                 int64_t workspace_bytes, rcb_stream_t stream) {
  const char* who = "recon_regions";
  RCB_REQUIRE(y && workspace, RCB_ERR_ARG, "%s: null y or workspace", who);
  RCB_REQUIRE(sse_r || n_bad_r, RCB_ERR_ARG, "%s: null sse_r and n_bad_r (nothing to write)", who);
  if (const int err = check_mode_fmt(who, mode, depth)) return err;
  RCB_REQUIRE(nd >= 1 && nd <= 3, RCB_ERR_UNSUPPORTED, "%s: %d grid dimensions (1 .. 3)", who, nd);
  RCB_REQUIRE(patch_nums && patch_size && region, RCB_ERR_ARG, "%s: null patch geometry or region", who);
  RCB_REQUIRE(channels >= 1 && channels <= 32, RCB_ERR_SHAPE, "%s: %d channels (1 .. 32)", who, channels);
  RCB_REQUIRE(n_rows > 0 && n_pix > 0, RCB_ERR_SHAPE, "%s: %lld rows of %d pixels", who, (long long)n_rows, n_pix);
  RCB_REQUIRE(!(sse_r && !target), RCB_ERR_ARG, "%s: sse_r needs a target", who);
  for (int i = 0; i < nd; ++i)
    RCB_REQUIRE(region[i] >= 1, RCB_ERR_SHAPE, "%s: axis %d of a region has %d positions (at least 1)", who, i, region[i]);
  RegionGeo x;
  PatchGeo& g = x.g;
  long long per, P;
  if (const int err = grid_axes(who, nd, patch_nums, patch_size, size, nullptr, g, per, P)) return err;
  RCB_REQUIRE(P == n_pix, RCB_ERR_SHAPE, "%s: the patch has %lld pixels, the rows %d", who, P, n_pix);
  RCB_REQUIRE(n_rows % per == 0, RCB_ERR_SHAPE, "%s: %lld rows are no whole number of datapoints of %lld patches", who,
              (long long)n_rows, per);
  RCB_REQUIRE(per * P <= 0x7fffffffLL, RCB_ERR_UNSUPPORTED, "%s: %lld pixels per datapoint (elements: up to 2^31 - 1)", who,
              per * P);                                      // (per, P < 2^31: the product fits 64 bits)
  const long long E = per * P * channels;
  RCB_REQUIRE(E <= 0x7fffffffLL, RCB_ERR_UNSUPPORTED, "%s: %lld elements per datapoint (up to 2^31 - 1)", who, E);
  grid_elems(g, channels, E);
  const long long n_data = n_rows / per;
  long long n_regions = 1, max_elems = channels;             // (both <= prod(sz) * C <= E)
  for (int i = 0; i < 3; ++i) {
    const int a = i - (3 - nd);                              // the caller's axis, or < 0: a leading axis of one position
    x.reg[i] = a < 0 ? 1 : std::min(region[a], g.sz[i]);
    x.nr[i] = (g.sz[i] + x.reg[i] - 1) / x.reg[i];
    n_regions *= x.nr[i];
    max_elems *= x.reg[i];
  }
  const int64_t need = rcb_recon_regions_workspace_bytes(n_data, n_regions, max_elems);
  RCB_REQUIRE(need > 0, RCB_ERR_UNSUPPORTED,
              "%s: %lld datapoints of %lld regions of up to %lld elements need more than 2^31 - 1 workgroups", who, n_data, n_regions,
              max_elems);
  RCB_REQUIRE(workspace_bytes >= need && aligned(workspace, 8), RCB_ERR_SHAPE,
              "%s: workspace of %lld bytes (8-byte aligned), %lld needed", who, (long long)workspace_bytes, (long long)need);
  x.n_regions = (int)n_regions;
  x.max_chunks = (int)((max_elems + kChunk - 1) / kChunk);
  x.mode = mode;
  x.rule = sample_rule16(mode, depth);
  const long long blocks = n_data * n_regions * x.max_chunks;
  double* part_sse = static_cast<double*>(workspace);
  int* part_bad = reinterpret_cast<int*>(part_sse + blocks);
  hipStream_t st = (hipStream_t)stream;
  // whole quads inside one run of y: every box row, every box origin and every run start on a 4-element boundary
  const bool vec = (x.reg[2] * channels) % 4 == 0 && g.L % 4 == 0 && g.R % 4 == 0 && aligned(y, 16) && (!target || aligned(target, 16));
  regions_kernel_of(vec, mode >= 2)<<<(unsigned)blocks, kThreads, 0, st>>>(y, target, part_sse, part_bad, x);
  RCB_LAUNCH_CHECK();
  regions_reduce_kernel<<<(unsigned)(n_data * n_regions), kThreads, 0, st>>>(part_sse, part_bad, x, sse_r, n_bad_r);
  RCB_LAUNCH_CHECK();
  return RCB_OK;
}
