// N4, the encoder's first step: whole signals -> the patch targets y [N][P][C] the kernels train on (reference: data/image.py:30-46,
// data/video.py:54-73 and data/audio.py:125-140 cut each patch out with a slice on the host, ToTensor / `video / 255` divide by 255).
//
// rcb_signal_patch reads n_data signals on the grid G_i = patch_nums[i] * patch_size[i] through ONE addressing rule -- element
// (d, g_0 .. g_nd-1, c) at src + d * data_stride + sum g_i * axis_stride[i] + c * channel_stride, strides in elements, >= 0 -- and
// writes y contiguous in the row order rcb_recon_finish reads: row n is patch n % prod(patch_nums) (row-major) of signal
// n / prod(patch_nums), its pixel p the row-major position inside the patch.  Which grid row a run of y comes from is
// patch_grid.h's decode_run, shared with recon.hip; here the strides of the source stand in place of the contiguous whole signal.
//
//   src_kind 0 (uint8):  y = (float)q / 255.0f         (one IEEE fp32 division: ToTensor's and numpy's)
//   src_kind 1 (fp32):   the 32 bits of the source, unchanged (moved as integers: NaN payloads, -0, denormals keep their bits)
//   src_kind 2 (u16 at depth b, rcb_signal_patch_fmt only):  y = (float)q / (float)(2^b - 1), one IEEE fp32 division; a stored
//                        value above 2^b - 1 is not clamped (y > 1)
//   src_kind 3 (s16, rcb_signal_patch_fmt only):  y = ((float)q + 32768.0f) / 65536.0f, every step exact
//
// Memory: a quad is 4 consecutive DESTINATION elements of one signal.  When the source is channel-last and dense along the last axis
// (channel_stride = 1, axis_stride[last] = channels), the run R = patch_size[last] * channels is a multiple of 4 and every run starts
// on a 4-element boundary of an aligned base, a quad is 4 consecutive source elements too and never straddles a run: one 4-byte
// (uint8), 8-byte (u16, s16) or 16-byte (fp32) load and one 16-byte store.  Otherwise the same quads are moved element by element.
// The host entry decides; both paths give the same bits.  Pure data movement: bytes = src + y.  No LDS, no atomics.
//
// rcb_signal_patch_pad (template parameter PAD) is the same cut of a signal that holds only size[i] <= G_i positions per axis:
// grid position g_i reads source position min(g_i, size[i] - 1), the edge sample replicated on the far side of every axis.  Of a
// grid row (g0, g1), numbered e = b2 * R + off, the first L = size[last] * C elements exist: with VEC (the same conditions, on the
// strides of the axes that still have more than one position) a quad whose 4 elements lie below L is 4 consecutive source elements
// on a 4-element boundary; any other quad moves element by element through the clipped index.  Every read is at a clipped
// position: inside the source.
//
// rcb_signal_patch_ragged (template parameter RAG) is the _pad cut with one extent, one offset
// and one stride set PER SIGNAL, read from row d of a device table the host entry writes (patch_grid.h: RaggedRow): signals of mixed
// sizes and orientations in one launch.  Whether a signal's quads are single loads is decided per signal on the host, by the same
// conditions, and travels in the row; the host entry also holds every signal's farthest element inside the source buffer.
#include <vector>

#include "patch_grid.h"

#pragma clang fp contract(off)

using namespace rcb;

namespace {

struct SignalGeo {
  PatchGeo g;
  long long ds, as[3], cs;    // source strides in elements: signal, axes (right-aligned, leading 0), channel
  float m;                    // KIND 2: 2^depth - 1
};

__device__ __forceinline__ unsigned unit8(unsigned q) { return __float_as_uint((float)q / 255.0f); }

// a 16-bit word of the source -> the bits of y: KIND 2 unsigned over m, KIND 3 two's complement on [0, 1)
template <int KIND>
__device__ __forceinline__ unsigned unit16(unsigned w, float m) {
  if (KIND == 2) return __float_as_uint((float)w / m);
  return __float_as_uint(((float)(int)(short)w + 32768.0f) / 65536.0f);
}

// PAD false never reads the extent (g.sz, g.L).  RAG (rcb_signal_patch_ragged; PAD): the extent, the strides
// and the place of the signal come from row d of `table` where the other entries take them from x, and VEC then says only that y
// takes whole quads (R % 4 == 0, y aligned) -- whether a quad of the SOURCE is one load is the row's kRaggedQuad, uniform over the
// workgroup.  RAG false is the code of the by-value entries and never reads `table`.
template <int KIND, bool VEC, bool PAD, bool RAG>
__global__ void __launch_bounds__(kThreads) signal_patch_kernel(const void* __restrict__ src, unsigned* __restrict__ y, SignalGeo xv,
                                                                const RaggedRow* __restrict__ table) {
  const long long blk = blockIdx.x;
  const long long d = blk / xv.g.n_chunks;
  const int chunk = (int)(blk % xv.g.n_chunks);
  SignalGeo xr;
  bool quad = true;                                          // (RAG) a quad of this signal's source is one load
  if (RAG) {
    const RaggedRow row = table[d];
    xr = xv;
    xr.g = ragged_geo(xv.g, row);
    xr.as[0] = row.as[0]; xr.as[1] = row.as[1]; xr.as[2] = row.as[2];
    xr.ds = row.off;                                         // (the signal's own offset: not a multiple of d)
    quad = (row.flags & kRaggedQuad) != 0;
  }
  const SignalGeo& x = RAG ? xr : xv;
  const PatchGeo& g = x.g;
  const uint8_t* s8 = static_cast<const uint8_t*>(src) + (RAG ? x.ds : d * x.ds);
  const unsigned* s32 = static_cast<const unsigned*>(src) + (RAG ? x.ds : d * x.ds);
  const uint16_t* s16 = static_cast<const uint16_t*>(src) + (RAG ? x.ds : d * x.ds);
  unsigned* yd = y + d * (long long)g.E;
  for (int it = 0; it < kQuadsPerThread; ++it) {
    const long long s0l = (long long)chunk * kChunk + ((long long)it * kThreads + threadIdx.x) * 4;
    if (s0l >= g.E) break;
    const int s0 = (int)s0l;
    const int n = g.E - s0 < 4 ? g.E - s0 : 4;
    int g0, g1, b2, e = 0;
    if (VEC && (!RAG || quad)) {                         // R % 4 == 0: the quad lies inside one run
      decode_run<PAD>(g, s0 / g.R, g0, g1, b2);
      e = b2 * g.R + s0 % g.R;
    }
    unsigned v[4] = {0u, 0u, 0u, 0u};
    if (VEC && (!RAG || quad) && (!PAD || e + 3 < g.L)) {  // 4 consecutive source elements (the last axis is dense: offset e)
      const long long o = g0 * x.as[0] + g1 * x.as[1] + e;
      if (KIND == 0) {
        const unsigned w = *reinterpret_cast<const unsigned*>(s8 + o);
        v[0] = unit8(w & 0xffu); v[1] = unit8((w >> 8) & 0xffu); v[2] = unit8((w >> 16) & 0xffu); v[3] = unit8(w >> 24);
      } else if (KIND == 1) {
        const uint4 q = *reinterpret_cast<const uint4*>(s32 + o);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        const uint2 q = *reinterpret_cast<const uint2*>(s16 + o);
        v[0] = unit16<KIND>(q.x & 0xffffu, x.m); v[1] = unit16<KIND>(q.x >> 16, x.m);
        v[2] = unit16<KIND>(q.y & 0xffffu, x.m); v[3] = unit16<KIND>(q.y >> 16, x.m);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < n) {
          const int s = s0 + k, off = s % g.R;
          decode_run<PAD>(g, s / g.R, g0, g1, b2);
          int g2 = b2 * g.ps[2] + off / g.C;
          if (PAD) g2 = min(g2, g.sz[2] - 1);
          const long long o = g0 * x.as[0] + g1 * x.as[1] + g2 * x.as[2] + (long long)(off % g.C) * x.cs;
          v[k] = KIND == 0 ? unit8(s8[o]) : KIND == 1 ? s32[o] : unit16<KIND>(s16[o], x.m);
        }
      }
    }
    if (VEC) {                                           // E % 4 == 0 and y 16-byte aligned
      *reinterpret_cast<uint4*>(yd + s0) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) yd[s0 + k] = v[k];
    }
  }
}

// THE dispatcher: the kernel of an entry -- by-value on the whole grid (neither), by-value padded (pad) or per-signal (rag, which
// is padded) -- for a source kind, with or without whole quads of y (vec)
using PatchKernel = void (*)(const void*, unsigned*, SignalGeo, const RaggedRow*);

template <int KIND, bool RAG>
PatchKernel patch_kernel_of(bool vec, bool pad) {
  if constexpr (RAG) {
    return vec ? signal_patch_kernel<KIND, true, true, true> : signal_patch_kernel<KIND, false, true, true>;
  } else {
    if (!pad) return vec ? signal_patch_kernel<KIND, true, false, false> : signal_patch_kernel<KIND, false, false, false>;
    return vec ? signal_patch_kernel<KIND, true, true, false> : signal_patch_kernel<KIND, false, true, false>;
  }
}

template <bool RAG>
PatchKernel patch_kernel_of(int kind, bool vec, bool pad) {
  switch (kind) {
    case 0: return patch_kernel_of<0, RAG>(vec, pad);
    case 1: return patch_kernel_of<1, RAG>(vec, pad);
    case 2: return patch_kernel_of<2, RAG>(vec, pad);
    default: return patch_kernel_of<3, RAG>(vec, pad);
  }
}

PatchKernel patch_kernel_of(int kind, bool vec, bool pad, bool rag) {
  return !rag ? patch_kernel_of<false>(kind, vec, pad) : patch_kernel_of<true>(kind, vec, pad);
}

// rcb_signal_patch_ragged: the caller's tables, the reach of the source and the device buffer the tables' copy goes to
struct RaggedArgs {
  int64_t src_elems;
  const int32_t* sizes;
  const int64_t* spans;
  void* table;
  int64_t table_bytes;
};

// all entries: `size` null is the uncropped form (every axis has its G_i positions); `fmt`: rcb_signal_patch_fmt, which alone of the
// by-value entries takes the 16-bit kinds and a depth; `rag`: rcb_signal_patch_ragged (fmt, size / data_stride / axis_stride unused:
// the extents and the strides are per signal) -- its refusals in its own words where they always differed
int patch_entry(const char* who, bool fmt, const void* src, int32_t src_kind, int32_t depth, int64_t n_data, int32_t nd,
                const int32_t* patch_nums, const int32_t* patch_size, const int32_t* size, int32_t channels, int64_t data_stride,
                const int64_t* axis_stride, int64_t channel_stride, float* y, rcb_stream_t stream, const RaggedArgs* rag = nullptr) {
  if (fmt) {
    RCB_REQUIRE(src_kind >= 0 && src_kind <= 3, RCB_ERR_ARG, "%s: source kind %d (0 = uint8, 1 = fp32, 2 = u16, 3 = s16)", who,
                src_kind);
    RCB_REQUIRE(src_kind == 2 ? (depth >= 9 && depth <= 16) : depth == 0, RCB_ERR_ARG,
                "%s: depth %d for source kind %d (9 .. 16 for u16, 0 for the others)", who, depth, src_kind);
  } else {
    RCB_REQUIRE(src_kind == 0 || src_kind == 1, RCB_ERR_ARG, "%s: source kind %d (0 = uint8, 1 = fp32)", who, src_kind);
  }
  RCB_REQUIRE(nd >= 1 && nd <= 3, RCB_ERR_UNSUPPORTED, "%s: %d grid dimensions (1 .. 3)", who, nd);
  if (rag) RCB_REQUIRE(patch_nums && patch_size, RCB_ERR_ARG, "%s: null patch geometry", who);
  else RCB_REQUIRE(patch_nums && patch_size && axis_stride, RCB_ERR_ARG, "%s: null patch geometry or strides", who);
  RCB_REQUIRE(channels >= 1 && channels <= 32, RCB_ERR_SHAPE, "%s: %d channels (1 .. 32)", who, channels);
  RCB_REQUIRE(n_data >= 0, RCB_ERR_SHAPE, "%s: %lld signals", who, (long long)n_data);
  SignalGeo x;
  PatchGeo& g = x.g;
  long long per, P;
  const int64_t no_stride[3] = {0, 0, 0};                    // (rag: selects the per-signal wording of the 2^31 limit)
  if (const int err = grid_axes(who, nd, patch_nums, patch_size, size, rag ? no_stride : axis_stride, g, per, P)) return err;
  if (rag) RCB_REQUIRE(channel_stride >= 0, RCB_ERR_ARG, "%s: negative channel stride %lld", who, (long long)channel_stride);
  else RCB_REQUIRE(data_stride >= 0 && channel_stride >= 0, RCB_ERR_ARG, "%s: negative stride (signal %lld, channel %lld)", who,
                   (long long)data_stride, (long long)channel_stride);
  const long long E = per * P * channels;
  RCB_REQUIRE(E <= 0x7fffffffLL, RCB_ERR_UNSUPPORTED, "%s: %lld elements per signal (up to 2^31 - 1)", who, E);
  if (n_data == 0) return RCB_OK;
  RCB_REQUIRE(src && y, RCB_ERR_ARG, "%s: null src or y", who);
  if (rag) {
    RCB_REQUIRE(rag->sizes && rag->spans && rag->table, RCB_ERR_ARG, "%s: null sizes, spans or table", who);
    const int64_t need = rcb_ragged_table_bytes(n_data);
    RCB_REQUIRE(need > 0 && rag->table_bytes >= need && aligned(rag->table, 8), RCB_ERR_SHAPE,
                "%s: table of %lld bytes (8-byte aligned), %lld needed", who, (long long)rag->table_bytes, (long long)need);
  }
  grid_elems(g, channels, E);
  x.ds = rag ? 0 : data_stride;
  x.cs = channel_stride;
  x.m = src_kind == 2 ? (float)((1 << depth) - 1) : 0.0f;
  for (int i = 0; i < 3; ++i) x.as[i] = rag || i < 3 - nd ? 0 : axis_stride[i - (3 - nd)];
  RCB_REQUIRE(n_data <= 0x7fffffffLL / g.n_chunks, RCB_ERR_UNSUPPORTED,
              "%s: %lld signals of %lld elements need more than 2^31 - 1 workgroups", who, (long long)n_data, E);
  hipStream_t st = (hipStream_t)stream;
  const uintptr_t esize = src_kind == 0 ? 1 : src_kind == 1 ? 4 : 2;
  // the 16-byte path (of y; the source quad is 4, 8 or 16 bytes): channel-last, dense last axis, and every run start -- base,
  // signal, outer positions; b2 * R by R % 4 -- a multiple of 4 elements (a stride only counts where its index can be non-zero: an
  // axis of more than one position)
  bool vec = g.R % 4 == 0 && aligned(y, 16);                 // y takes whole quads (E % 4 == 0 by R % 4 == 0)
  if (rag) {                                                 // ... decided per signal, on its strides and its first element's address
    std::vector<RaggedRow> rows((size_t)n_data);
    std::vector<long long> reach((size_t)n_data);
    if (const int err = ragged_rows(who, n_data, nd, g, channels, channel_stride, rag->sizes, rag->spans, rows.data(), reach.data()))
      return err;
    for (long long d = 0; d < n_data; ++d) {
      RaggedRow& r = rows[(size_t)d];
      RCB_REQUIRE(reach[(size_t)d] < rag->src_elems, RCB_ERR_SHAPE, "%s: signal %lld reaches element %lld of a source of %lld", who,
                  d, reach[(size_t)d], (long long)rag->src_elems);
      bool quad = (channels == 1 || channel_stride == 1) && (r.sz[2] == 1 || r.as[2] == channels) &&
                  ((uintptr_t)src + (uintptr_t)r.off * esize) % (4 * esize) == 0;
      for (int i = 0; i < 2; ++i) quad = quad && (r.sz[i] == 1 || r.as[i] % 4 == 0);
      r.flags = quad ? kRaggedQuad : 0;
    }
    if (const int err = ragged_upload(who, rows.data(), n_data, rag->table, st)) return err;
  } else {
    vec = vec && (channels == 1 || channel_stride == 1) && (g.sz[2] == 1 || x.as[2] == channels) && aligned(src, 4 * esize) &&
          (n_data == 1 || data_stride % 4 == 0);
    for (int i = 0; i < 2; ++i) vec = vec && (g.sz[i] == 1 || x.as[i] % 4 == 0);
  }
  patch_kernel_of(src_kind, vec, size != nullptr, rag != nullptr)<<<(unsigned)(n_data * g.n_chunks), kThreads, 0, st>>>(
      src, reinterpret_cast<unsigned*>(y), x, rag ? static_cast<const RaggedRow*>(rag->table) : nullptr);
  RCB_LAUNCH_CHECK();
  return RCB_OK;
}

}  // namespace

extern "C" int64_t rcb_ragged_table_bytes(int64_t n_data) {
  if (n_data < 0 || n_data > 0x7fffffffLL) return -1;
  return n_data * (int64_t)sizeof(RaggedRow);
}

extern "C" int rcb_signal_patch_ragged(const void* src, int64_t src_elems, int32_t src_kind, int32_t depth, int64_t n_data,
                                       int32_t nd, const int32_t* patch_nums, const int32_t* patch_size, const int32_t* sizes,
                                       const int64_t* spans, int32_t channels, int64_t channel_stride, float* y, void* table,
                                       int64_t table_bytes, rcb_stream_t stream) {
  const RaggedArgs rag = {src_elems, sizes, spans, table, table_bytes};
  return patch_entry("signal_patch_ragged", true, src, src_kind, depth, n_data, nd, patch_nums, patch_size, nullptr, channels, 0,
                     nullptr, channel_stride, y, stream, &rag);
}

extern "C" int rcb_signal_patch(const void* src, int32_t src_kind, int64_t n_data, int32_t nd, const int32_t* patch_nums,
                                const int32_t* patch_size, int32_t channels, int64_t data_stride, const int64_t* axis_stride,
                                int64_t channel_stride, float* y, rcb_stream_t stream) {
  return patch_entry("signal_patch", false, src, src_kind, 0, n_data, nd, patch_nums, patch_size, nullptr, channels, data_stride,
                     axis_stride, channel_stride, y, stream);
}

extern "C" int rcb_signal_patch_pad(const void* src, int32_t src_kind, int64_t n_data, int32_t nd, const int32_t* patch_nums,
                                    const int32_t* patch_size, const int32_t* size, int32_t channels, int64_t data_stride,
                                    const int64_t* axis_stride, int64_t channel_stride, float* y, rcb_stream_t stream) {
  RCB_REQUIRE(size, RCB_ERR_ARG, "signal_patch_pad: null size");
  return patch_entry("signal_patch_pad", false, src, src_kind, 0, n_data, nd, patch_nums, patch_size, size, channels, data_stride,
                     axis_stride, channel_stride, y, stream);
}

extern "C" int rcb_signal_patch_fmt(const void* src, int32_t src_kind, int32_t depth, int64_t n_data, int32_t nd,
                                    const int32_t* patch_nums, const int32_t* patch_size, const int32_t* size, int32_t channels,
                                    int64_t data_stride, const int64_t* axis_stride, int64_t channel_stride, float* y,
                                    rcb_stream_t stream) {
  return patch_entry("signal_patch_fmt", true, src, src_kind, depth, n_data, nd, patch_nums, patch_size, size, channels, data_stride,
                     axis_stride, channel_stride, y, stream);
}
