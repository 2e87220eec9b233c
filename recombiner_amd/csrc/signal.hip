// N4, the encoder's first step: whole signals -> the patch targets y [N][P][C] the kernels train on (reference: data/image.py:30-46,
// data/video.py:54-73 and data/audio.py:125-140 cut each patch out with a slice on the host, ToTensor / `video / 255` divide by 255).
//
// rcb_signal_patch reads n_data signals on the grid G_i = patch_nums[i] * patch_size[i] through ONE addressing rule -- element
// (d, g_0 .. g_nd-1, c) at src + d * data_stride + sum g_i * axis_stride[i] + c * channel_stride, strides in elements, >= 0 -- and
// writes y contiguous in the row order rcb_recon_finish reads: row n is patch n % prod(patch_nums) (row-major) of signal
// n / prod(patch_nums), its pixel p the row-major position inside the patch.  The index arithmetic is recon.hip's whole_offset with
// the strides of the source in place of the contiguous whole signal.
//
//   src_kind 0 (uint8):  y = (float)q / 255.0f         (one IEEE fp32 division: ToTensor's and numpy's)
//   src_kind 1 (fp32):   the 32 bits of the source, unchanged (moved as integers: NaN payloads, -0, denormals keep their bits)
//
// Memory: a quad is 4 consecutive DESTINATION elements of one signal.  When the source is channel-last and dense along the last axis
// (channel_stride = 1, axis_stride[last] = channels), the run R = patch_size[last] * channels is a multiple of 4 and every run starts
// on a 4-element boundary of an aligned base, a quad is 4 consecutive source elements too and never straddles a run: one 4-byte
// (uint8) or 16-byte (fp32) load and one 16-byte store.  Otherwise the same quads are moved element by element.  The host entry
// decides; both paths give the same bits.  Pure data movement: bytes = src + y.  No LDS, no atomics.
#include "rcb_common.h"

#pragma clang fp contract(off)

using namespace rcb;

namespace {

constexpr int kThreads = 256;
constexpr int kQuadsPerThread = 8;
constexpr int kChunk = kThreads * 4 * kQuadsPerThread;      // 8192 elements of one signal per workgroup

struct SignalGeo {
  int pn[3], ps[3];           // patches per axis / pixels per axis of a patch, right-aligned (leading axes 1)
  int C;                      // channels
  int R;                      // elements of one run of y: ps[2] * C
  int E;                      // elements of one signal
  int n_chunks;               // ceil(E / kChunk)
  long long ds, as[3], cs;    // source strides in elements: signal, axes (right-aligned, leading 0), channel
};

// source offset of pixel 0, channel 0 of run `run` of a signal's y: the run order is that of recon.hip's whole_offset
// (patch b0 b1 b2 row-major, then the patch's rows p0 p1), the grid position g_i = b_i * ps_i + p_i
__device__ __forceinline__ long long run_offset(const SignalGeo& g, int run) {
  int r = run;
  const int p1 = r % g.ps[1]; r /= g.ps[1];
  const int p0 = r % g.ps[0]; r /= g.ps[0];
  const int b2 = r % g.pn[2]; r /= g.pn[2];
  const int b1 = r % g.pn[1];
  const int b0 = r / g.pn[1];
  const long long g0 = (long long)b0 * g.ps[0] + p0, g1 = (long long)b1 * g.ps[1] + p1, g2 = (long long)b2 * g.ps[2];
  return g0 * g.as[0] + g1 * g.as[1] + g2 * g.as[2];
}

__device__ __forceinline__ unsigned unit8(unsigned q) { return __float_as_uint((float)q / 255.0f); }

template <int KIND, bool VEC>
__global__ void __launch_bounds__(kThreads) signal_patch_kernel(const void* __restrict__ src, unsigned* __restrict__ y, SignalGeo g) {
  const long long blk = blockIdx.x;
  const long long d = blk / g.n_chunks;
  const int chunk = (int)(blk % g.n_chunks);
  const uint8_t* s8 = static_cast<const uint8_t*>(src) + d * g.ds;
  const unsigned* s32 = static_cast<const unsigned*>(src) + d * g.ds;
  unsigned* yd = y + d * (long long)g.E;
  for (int it = 0; it < kQuadsPerThread; ++it) {
    const long long s0l = (long long)chunk * kChunk + ((long long)it * kThreads + threadIdx.x) * 4;
    if (s0l >= g.E) break;
    const int s0 = (int)s0l;
    if (VEC) {                                           // R % 4 == 0: whole quads inside one run, 4 consecutive source elements
      const long long o = run_offset(g, s0 / g.R) + s0 % g.R;
      uint4 v;
      if (KIND == 0) {
        const unsigned w = *reinterpret_cast<const unsigned*>(s8 + o);
        v = make_uint4(unit8(w & 0xffu), unit8((w >> 8) & 0xffu), unit8((w >> 16) & 0xffu), unit8(w >> 24));
      } else {
        v = *reinterpret_cast<const uint4*>(s32 + o);
      }
      *reinterpret_cast<uint4*>(yd + s0) = v;
    } else {
      const int n = g.E - s0 < 4 ? g.E - s0 : 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < n) {
          const int s = s0 + k, off = s % g.R;
          const long long o = run_offset(g, s / g.R) + (long long)(off / g.C) * g.as[2] + (long long)(off % g.C) * g.cs;
          yd[s] = KIND == 0 ? unit8(s8[o]) : s32[o];
        }
      }
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int rcb_signal_patch(const void* src, int32_t src_kind, int64_t n_data, int32_t nd, const int32_t* patch_nums,
                                const int32_t* patch_size, int32_t channels, int64_t data_stride, const int64_t* axis_stride,
                                int64_t channel_stride, float* y, rcb_stream_t stream) {
  RCB_REQUIRE(src_kind == 0 || src_kind == 1, RCB_ERR_ARG, "signal_patch: source kind %d (0 = uint8, 1 = fp32)", src_kind);
  RCB_REQUIRE(nd >= 1 && nd <= 3, RCB_ERR_UNSUPPORTED, "signal_patch: %d grid dimensions (1 .. 3)", nd);
  RCB_REQUIRE(patch_nums && patch_size && axis_stride, RCB_ERR_ARG, "signal_patch: null patch geometry or strides");
  RCB_REQUIRE(channels >= 1 && channels <= 32, RCB_ERR_SHAPE, "signal_patch: %d channels (1 .. 32)", channels);
  RCB_REQUIRE(n_data >= 0, RCB_ERR_SHAPE, "signal_patch: %lld signals", (long long)n_data);
  SignalGeo g;
  long long pix = 1;
  for (int i = 0; i < 3; ++i) g.pn[i] = g.ps[i] = 1, g.as[i] = 0;
  for (int i = 0; i < nd; ++i) {
    RCB_REQUIRE(patch_nums[i] > 0 && patch_size[i] > 0, RCB_ERR_SHAPE, "signal_patch: axis %d has %d patches of %d pixels", i,
                patch_nums[i], patch_size[i]);
    RCB_REQUIRE(axis_stride[i] >= 0, RCB_ERR_ARG, "signal_patch: negative stride %lld of axis %d", (long long)axis_stride[i], i);
    g.pn[3 - nd + i] = patch_nums[i];
    g.ps[3 - nd + i] = patch_size[i];
    g.as[3 - nd + i] = axis_stride[i];
    const long long G = (long long)patch_nums[i] * patch_size[i];
    RCB_REQUIRE(G <= 0x7fffffffLL && pix * G <= 0x7fffffffLL, RCB_ERR_UNSUPPORTED,
                "signal_patch: more than 2^31 - 1 elements per signal");     // (pix, G < 2^31: the product fits 64 bits)
    pix *= G;
  }
  RCB_REQUIRE(data_stride >= 0 && channel_stride >= 0, RCB_ERR_ARG, "signal_patch: negative stride (signal %lld, channel %lld)",
              (long long)data_stride, (long long)channel_stride);
  const long long E = pix * channels;
  RCB_REQUIRE(E <= 0x7fffffffLL, RCB_ERR_UNSUPPORTED, "signal_patch: %lld elements per signal (up to 2^31 - 1)", E);
  if (n_data == 0) return RCB_OK;
  RCB_REQUIRE(src && y, RCB_ERR_ARG, "signal_patch: null src or y");
  g.C = channels;
  g.R = g.ps[2] * channels;
  g.E = (int)E;
  g.n_chunks = (int)((E + kChunk - 1) / kChunk);
  g.ds = data_stride;
  g.cs = channel_stride;
  RCB_REQUIRE(n_data <= 0x7fffffffLL / g.n_chunks, RCB_ERR_UNSUPPORTED,
              "signal_patch: %lld signals of %lld elements need more than 2^31 - 1 workgroups", (long long)n_data, E);
  // the 16-byte path: channel-last, dense last axis, and every run start -- base, signal, outer grid positions; b2 * R by R % 4 -- a
  // multiple of 4 elements (a stride only counts where its index can be non-zero)
  bool vec = (channels == 1 || channel_stride == 1) && (g.pn[2] * g.ps[2] == 1 || g.as[2] == channels) && g.R % 4 == 0 &&
             aligned(y, 16) && aligned(src, src_kind == 0 ? 4 : 16);
  vec = vec && (n_data == 1 || data_stride % 4 == 0);
  for (int i = 0; i < 2; ++i) vec = vec && (g.pn[i] * g.ps[i] == 1 || g.as[i] % 4 == 0);
  const unsigned blocks = (unsigned)(n_data * g.n_chunks);
  unsigned* yo = reinterpret_cast<unsigned*>(y);
  hipStream_t st = (hipStream_t)stream;
  if (src_kind == 0) {
    if (vec) signal_patch_kernel<0, true><<<blocks, kThreads, 0, st>>>(src, yo, g);
    else signal_patch_kernel<0, false><<<blocks, kThreads, 0, st>>>(src, yo, g);
  } else {
    if (vec) signal_patch_kernel<1, true><<<blocks, kThreads, 0, st>>>(src, yo, g);
    else signal_patch_kernel<1, false><<<blocks, kThreads, 0, st>>>(src, yo, g);
  }
  RCB_LAUNCH_CHECK();
  return RCB_OK;
}
