// N4: the decoder's last step and the distortion figure on the device (reference: utils.py:200-260 rounds the reconstruction to
// 8 bits and forms the squared error in numpy on the host, main_compression.py:154-167 calls it on the whole batch).
//
// rcb_recon_finish reads the reconstruction y [N][P][C] (fp32; the rows are datapoints, or the patches of stitched signals as in
// rcb_siren_desc.pe_grid_dims) once and writes, each optional: the 8-bit whole signals, the fp32 whole signals of the rounded (mode
// 0) or raw (mode 1) values, per datapoint the fp64 sum of squared errors against `target`, and the count of non-finite inputs.
//
//   mode 0:  q = rintf(fminf(fmaxf(x, 0), 1) * 255.0f)      (fp32 multiply, round half to even: np.round)
//            v = q / 255.0f                                  (IEEE fp32 division: numpy's)
//   mode 1:  v = x
//   sse   =  sum of (double)d * (double)d,  d = t - v in fp32 (the difference numpy forms elementwise)
//
// Reduction (no floating-point atomics, no workgroup hand-off): a datapoint's E = rows * P * C elements are contiguous in y; they
// are cut into chunks of kChunk elements, one workgroup each.  Thread t of a workgroup owns the quads t, t + 256, ... of its chunk
// and adds their terms in element order; the 64 lanes of a wave are combined by the xor butterfly, the four waves in wave order;
// a second kernel adds a datapoint's chunk partials (thread t: partials t, t + 256, ... in order, then the same butterfly).  Every
// step is a function of E alone -- not of n_data, the CU count, the launch, or whether the 16-byte path below is taken -- so a
// datapoint's sse is bitwise the same alone and inside any batch, and from run to run.
//
// Memory: a quad is 4 consecutive source elements.  When the contiguous run of a patch row, R = patch_size[last] * C floats (the
// whole datapoint for nd = 0), is a multiple of 4 and the pointers are 16-byte aligned, a quad never straddles a run: one 16-byte
// load per input, one 16-byte store to `whole`, one 4-byte store to `u8`, coalesced along C x pixels of the patch row.  Otherwise the
// same quads are moved element by element.  HBM-bound: bytes = y + target + outputs.
#include "rcb_common.h"

#pragma clang fp contract(off)

using namespace rcb;

namespace {

constexpr int kThreads = 256;
constexpr int kQuadsPerThread = 8;
constexpr int kChunk = kThreads * 4 * kQuadsPerThread;      // 8192 elements of one datapoint per workgroup

struct ReconGeo {
  int pn[3], ps[3];       // patches per axis / pixels per axis of a patch, right-aligned (leading axes 1)
  int C;                  // channels
  int R;                  // floats of one contiguous run: ps[2] * C
  int E;                  // elements of one datapoint
  int n_chunks;           // ceil(E / kChunk)
  int mode;
};

// offset of source element s (a multiple of R plus `off` < R) of a datapoint inside its stitched signal
__device__ __forceinline__ int whole_offset(const ReconGeo& g, int run, int off) {
  int r = run;
  const int p1 = r % g.ps[1]; r /= g.ps[1];
  const int p0 = r % g.ps[0]; r /= g.ps[0];
  const int b2 = r % g.pn[2]; r /= g.pn[2];
  const int b1 = r % g.pn[1];
  const int b0 = r / g.pn[1];
  const int g0 = b0 * g.ps[0] + p0, g1 = b1 * g.ps[1] + p1;
  // ((g0 * G1 + g1) * G2 + b2 * ps2) * C + off, with G2 * C = pn2 * R and ps2 * C = R
  return ((g0 * (g.pn[1] * g.ps[1]) + g1) * g.pn[2] + b2) * g.R + off;
}

struct Elem {
  float v;
  unsigned q;
  bool bad;
};

__device__ __forceinline__ Elem finish(float x, int mode) {
  Elem e;
  e.bad = !(fabsf(x) < __builtin_inff());
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

template <bool VEC>
__global__ void __launch_bounds__(kThreads) recon_kernel(const float* __restrict__ y, const float* __restrict__ target,
                                                         uint8_t* __restrict__ u8, float* __restrict__ whole,
                                                         double* __restrict__ part_sse, int* __restrict__ part_bad, ReconGeo g) {
  const long long blk = blockIdx.x;
  const long long d = blk / g.n_chunks;
  const int chunk = (int)(blk % g.n_chunks);
  const long long base = d * (long long)g.E;
  const float* yd = y + base;
  const float* td = target ? target + base : nullptr;
  double acc = 0.0;
  int bad = 0;
  for (int it = 0; it < kQuadsPerThread; ++it) {
    const long long s0l = (long long)chunk * kChunk + ((long long)it * kThreads + threadIdx.x) * 4;
    if (s0l >= g.E) break;
    const int s0 = (int)s0l;
    float x[4], t[4] = {0.f, 0.f, 0.f, 0.f};
    int n = 4;
    if (VEC) {                                           // E % 4 == 0: whole quads only
      const float4 xv = *reinterpret_cast<const float4*>(yd + s0);
      x[0] = xv.x; x[1] = xv.y; x[2] = xv.z; x[3] = xv.w;
      if (td) {
        const float4 tv = *reinterpret_cast<const float4*>(td + s0);
        t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
      }
    } else {
      n = g.E - s0 < 4 ? g.E - s0 : 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        x[k] = k < n ? yd[s0 + k] : 0.0f;
        if (td) t[k] = k < n ? td[s0 + k] : 0.0f;
      }
    }
    Elem e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      e[k] = finish(x[k], g.mode);
      if (k < n) {
        const bool b = e[k].bad || !(fabsf(t[k]) < __builtin_inff());
        bad += (int)e[k].bad + (int)!(fabsf(t[k]) < __builtin_inff());
        const float df = t[k] - e[k].v;
        const double dd = (double)df;
        acc += b ? 0.0 : dd * dd;                        // (a bad element makes the datapoint's sse NaN in the second kernel)
      }
    }
    if (u8 || whole) {
      if (VEC) {
        const long long o = base + whole_offset(g, s0 / g.R, s0 % g.R);
        if (whole) *reinterpret_cast<float4*>(whole + o) = make_float4(e[0].v, e[1].v, e[2].v, e[3].v);
        if (u8) *reinterpret_cast<unsigned*>(u8 + o) = e[0].q | (e[1].q << 8) | (e[2].q << 16) | (e[3].q << 24);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < n) {
            const long long o = base + whole_offset(g, (s0 + k) / g.R, (s0 + k) % g.R);
            if (whole) whole[o] = e[k].v;
            if (u8) u8[o] = (uint8_t)e[k].q;
          }
        }
      }
    }
  }
  if (block_sum(acc, bad)) {
    part_sse[blk] = acc;
    part_bad[blk] = bad;
  }
}

// one workgroup per datapoint: its chunk partials in a fixed order
__global__ void __launch_bounds__(kThreads) recon_reduce_kernel(const double* __restrict__ part_sse, const int* __restrict__ part_bad,
                                                                int n_chunks, double* __restrict__ sse, int* __restrict__ n_bad) {
  const long long d = blockIdx.x;
  double acc = 0.0;
  int bad = 0;
  for (int c = threadIdx.x; c < n_chunks; c += kThreads) {
    acc += part_sse[d * n_chunks + c];
    bad += part_bad[d * n_chunks + c];
  }
  if (block_sum(acc, bad)) {
    if (sse) sse[d] = bad ? __builtin_nan("") : acc;
    if (n_bad) n_bad[d] = bad;
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int64_t rcb_recon_workspace_bytes(int64_t n_data, int64_t elems_per_datapoint) {
  if (n_data <= 0 || elems_per_datapoint <= 0 || elems_per_datapoint > 0x7fffffffLL) return -1;
  const int64_t n_chunks = (elems_per_datapoint + kChunk - 1) / kChunk;
  if (n_data > 0x7fffffffLL / n_chunks) return -1;
  return n_data * n_chunks * (int64_t)(sizeof(double) + sizeof(int));
}

extern "C" int rcb_recon_finish(const float* y, const float* target, int64_t n_rows, int32_t n_pix, int32_t channels, int32_t nd,
                                const int32_t* patch_nums, const int32_t* patch_size, int32_t mode, uint8_t* u8, float* whole,
                                double* sse, int32_t* n_bad, void* workspace, int64_t workspace_bytes, rcb_stream_t stream) {
  RCB_REQUIRE(y && workspace, RCB_ERR_ARG, "recon_finish: null y or workspace");
  RCB_REQUIRE(mode == 0 || mode == 1, RCB_ERR_ARG, "recon_finish: mode %d (0 = 8-bit, 1 = raw)", mode);
  RCB_REQUIRE(nd >= 0 && nd <= 3, RCB_ERR_UNSUPPORTED, "recon_finish: %d grid dimensions (0 .. 3)", nd);
  RCB_REQUIRE(nd == 0 || (patch_nums && patch_size), RCB_ERR_ARG, "recon_finish: null patch geometry");
  RCB_REQUIRE(channels >= 1 && channels <= 32, RCB_ERR_SHAPE, "recon_finish: %d channels (1 .. 32)", channels);
  RCB_REQUIRE(n_rows > 0 && n_pix > 0, RCB_ERR_SHAPE, "recon_finish: %lld rows of %d pixels", (long long)n_rows, n_pix);
  RCB_REQUIRE(!(u8 && mode == 1), RCB_ERR_ARG, "recon_finish: the raw mode has no 8-bit output");
  RCB_REQUIRE(!(sse && !target), RCB_ERR_ARG, "recon_finish: sse needs a target");
  ReconGeo g;
  long long per = 1, P = 1;
  for (int i = 0; i < 3; ++i) g.pn[i] = g.ps[i] = 1;
  for (int i = 0; i < nd; ++i) {
    RCB_REQUIRE(patch_nums[i] > 0 && patch_size[i] > 0, RCB_ERR_SHAPE, "recon_finish: axis %d has %d patches of %d pixels", i,
                patch_nums[i], patch_size[i]);
    g.pn[3 - nd + i] = patch_nums[i];
    g.ps[3 - nd + i] = patch_size[i];
    per *= patch_nums[i];
    P *= patch_size[i];
    RCB_REQUIRE(per <= 0x7fffffffLL && P <= 0x7fffffffLL, RCB_ERR_SHAPE, "recon_finish: patch geometry overflows");
  }
  if (nd == 0) g.ps[2] = n_pix, P = n_pix;
  RCB_REQUIRE(P == n_pix, RCB_ERR_SHAPE, "recon_finish: the patch has %lld pixels, the rows %d", P, n_pix);
  RCB_REQUIRE(n_rows % per == 0, RCB_ERR_SHAPE, "recon_finish: %lld rows are no whole number of datapoints of %lld patches",
              (long long)n_rows, per);
  RCB_REQUIRE(per * P <= 0x7fffffffLL, RCB_ERR_UNSUPPORTED, "recon_finish: %lld pixels per datapoint (elements: up to 2^31 - 1)",
              per * P);                                      // (per, P < 2^31: the product fits 64 bits)
  const long long E = per * P * channels;
  RCB_REQUIRE(E <= 0x7fffffffLL, RCB_ERR_UNSUPPORTED, "recon_finish: %lld elements per datapoint (up to 2^31 - 1)", E);
  const long long n_data = n_rows / per;
  const int64_t need = rcb_recon_workspace_bytes(n_data, E);
  RCB_REQUIRE(need > 0, RCB_ERR_UNSUPPORTED, "recon_finish: %lld datapoints of %lld elements need more than 2^31 - 1 workgroups",
              n_data, E);
  RCB_REQUIRE(workspace_bytes >= need && aligned(workspace, 8), RCB_ERR_SHAPE,
              "recon_finish: workspace of %lld bytes (8-byte aligned), %lld needed", (long long)workspace_bytes, (long long)need);
  g.C = channels;
  g.R = g.ps[2] * channels;
  g.E = (int)E;
  g.n_chunks = (int)((E + kChunk - 1) / kChunk);
  g.mode = mode;
  const long long blocks = n_data * g.n_chunks;
  double* part_sse = static_cast<double*>(workspace);
  int* part_bad = reinterpret_cast<int*>(part_sse + blocks);
  const bool vec = g.R % 4 == 0 && aligned(y, 16) && (!target || aligned(target, 16)) && (!whole || aligned(whole, 16)) &&
                   (!u8 || aligned(u8, 4));
  if (vec)
    recon_kernel<true><<<(unsigned)blocks, kThreads, 0, (hipStream_t)stream>>>(y, target, u8, whole, part_sse, part_bad, g);
  else
    recon_kernel<false><<<(unsigned)blocks, kThreads, 0, (hipStream_t)stream>>>(y, target, u8, whole, part_sse, part_bad, g);
  RCB_LAUNCH_CHECK();
  if (sse || n_bad) {
    recon_reduce_kernel<<<(unsigned)n_data, kThreads, 0, (hipStream_t)stream>>>(part_sse, part_bad, g.n_chunks, sse, n_bad);
    RCB_LAUNCH_CHECK();
  }
  return RCB_OK;
}
