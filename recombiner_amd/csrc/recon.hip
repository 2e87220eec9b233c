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
//   mode 2:  (rcb_recon_finish_fmt; u16 at depth b, M = 2^b - 1)   q = rintf(c * (float)M),  v = (float)(int)q / (float)M
//   mode 3:  (rcb_recon_finish_fmt; s16)   u = fminf(rintf(c * 65536.0f), 65535.0f),  q = (int)u - 32768,  v = u / 65536.0f
//            c = NaN ? 0 : fminf(fmaxf(x, 0), 1); the integer output is 16-bit words, a quad of them one 8-byte store
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
//
// rcb_recon_finish_crop is the same kernel (template parameter CROP) for datapoints of which only a leading extent is real.
// Where a run lies in the stitched signal, the chunking and the validation of the patch grid are patch_grid.h's, shared with
// signal.hip, which cuts the signals the other way.  What an element becomes (finish, finish16), the term it adds and block_sum are
// recon_elem.h's, shared with recon_regions.hip, which sums the same terms per box of the signal.
//
// rcb_recon_finish_ragged (template parameter RAG) is the crop form with one extent and one
// output span PER SIGNAL, read from row d of a device table the host entry writes (patch_grid.h: RaggedRow): each signal's outputs
// go to its own offset of one buffer, along its own strides (a transposed delivery is only that).  The loads, the terms and the
// order of the additions do not know about it: sse[d] stays the crop entry's for that signal alone, bit for bit.
#include <algorithm>
#include <vector>

#include "recon_elem.h"                                  // the per-element arithmetic and block_sum, shared with recon_regions.hip

#pragma clang fp contract(off)

using namespace rcb;

namespace {

// rcb_recon_finish_crop: of the grid row (g0, g1) of g only the first g.L elements e = b2 * R + off exist, and only for g0 < sz[0],
// g1 < sz[1].  An element outside adds +0.0 to the sum, is never counted and is not written; the outputs are contiguous over the
// extent.
struct ReconGeo {
  PatchGeo g;
  int mode;
  int vec_out;            // crop: L % 4 == 0 and aligned outputs: a quad inside the extent is one 16-byte / 4- or 8-byte store
  long long Ec;           // crop: elements of one cropped datapoint
  // W16 (modes 2 and 3, rcb_recon_finish_fmt): u = fminf(rintf(c * scale), cap), the stored word (int)u - bias
  float scale, cap;       // u16 at depth b: M = 2^b - 1 and M (the clamp never binds); s16: 65536 and 65535
  int bias;               // u16: 0; s16: 32768
};

// offset of source element s (a multiple of R plus `off` < R) of a datapoint inside its stitched signal
__device__ __forceinline__ int whole_offset(const PatchGeo& g, int run, int off) {
  int g0, g1, b2;
  decode_run<false>(g, run, g0, g1, b2);
  // ((g0 * G1 + g1) * G2 + b2 * ps2) * C + off, with G2 * C = pn2 * R and ps2 * C = R
  return ((g0 * (g.pn[1] * g.ps[1]) + g1) * g.pn[2] + b2) * g.R + off;
}

// grid row of run `run` inside the cropped datapoint: -> offset of its element 0, or -1 when the row lies outside; e0 = b2 * R
__device__ __forceinline__ int crop_row(const PatchGeo& g, int run, int& e0) {
  int g0, g1, b2;
  decode_run<false>(g, run, g0, g1, b2);
  e0 = b2 * g.R;
  return (g0 < g.sz[0] && g1 < g.sz[1]) ? (g0 * g.sz[1] + g1) * g.L : -1;
}

// rcb_recon_finish_ragged: the same row inside signal `r`'s own span -> offset of its element 0 from the span's start, or -1
__device__ __forceinline__ long long ragged_row(const PatchGeo& g, const RaggedRow& r, int run, int& e0) {
  int g0, g1, b2;
  decode_run<false>(g, run, g0, g1, b2);
  e0 = b2 * g.R;
  return (g0 < g.sz[0] && g1 < g.sz[1]) ? g0 * r.as[0] + g1 * r.as[1] : -1;
}

// element e = pos * C + c of a grid row inside the span: e itself where the last axis is the innermost (kRaggedDense)
__device__ __forceinline__ long long ragged_elem(const PatchGeo& g, const RaggedRow& r, int e) {
  return (r.flags & kRaggedDense) ? (long long)e : (e / g.C) * r.as[2] + e % g.C;
}

// the integer output at element offset o: bytes, or (W16) 16-bit words, a quad of which is one 8-byte store
template <bool W16>
__device__ __forceinline__ void store_quad(uint8_t* out, long long o, const Elem (&e)[4]) {
  if (W16)
    *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(out) + o) = make_uint2(e[0].q | (e[1].q << 16), e[2].q | (e[3].q << 16));
  else
    *reinterpret_cast<unsigned*>(out + o) = e[0].q | (e[1].q << 8) | (e[2].q << 16) | (e[3].q << 24);
}

template <bool W16>
__device__ __forceinline__ void store_one(uint8_t* out, long long o, unsigned q) {
  if (W16) reinterpret_cast<uint16_t*>(out)[o] = (uint16_t)q;
  else out[o] = (uint8_t)q;
}

// CROP: rcb_recon_finish_crop -- the same loads, the same additions in the same order; only what an element outside the extent
// contributes (+0.0, no count) and where the outputs go differ.  W16 (rcb_recon_finish_fmt, modes 2 and 3): `u8` addresses 16-bit
// words and an element is finish16's; W16 false is the code of the 8-bit and raw modes
// RAG (rcb_recon_finish_ragged; CROP): the extent and the place of the signal's outputs come from row d of `table` -- the span's
// offset and strides instead of d * Ec and the contiguous cropped rows (x.Ec is not read, and x.vec_out says only that the output
// POINTERS take quads: the rest is the row's kRaggedQuad); what is loaded, what an element contributes and the order of the
// additions are CROP's.  RAG false is the code of the by-value entries and never reads `table`.
template <bool VEC, bool CROP, bool W16, bool RAG>
__global__ void __launch_bounds__(kThreads) recon_kernel(const float* __restrict__ y, const float* __restrict__ target,
                                                         uint8_t* __restrict__ u8, float* __restrict__ whole,
                                                         double* __restrict__ part_sse, int* __restrict__ part_bad, ReconGeo x,
                                                         const RaggedRow* __restrict__ table) {
  const long long blk = blockIdx.x;
  const long long d = blk / x.g.n_chunks;
  const int chunk = (int)(blk % x.g.n_chunks);
  PatchGeo gr;
  RaggedRow rrow;
  if (RAG) {
    rrow = table[d];
    gr = ragged_geo(x.g, rrow);
  }
  const PatchGeo& g = RAG ? gr : x.g;
  const long long base = d * (long long)g.E;
  const float* yd = y + base;
  const float* td = target ? target + base : nullptr;
  double acc = 0.0;
  int bad = 0;
  for (int it = 0; it < kQuadsPerThread; ++it) {
    const long long s0l = (long long)chunk * kChunk + ((long long)it * kThreads + threadIdx.x) * 4;
    if (s0l >= g.E) break;
    const int s0 = (int)s0l;
    float xs[4], t[4] = {0.f, 0.f, 0.f, 0.f};
    int n = 4;
    if (VEC) {                                           // E % 4 == 0: whole quads only
      const float4 xv = *reinterpret_cast<const float4*>(yd + s0);
      xs[0] = xv.x; xs[1] = xv.y; xs[2] = xv.z; xs[3] = xv.w;
      if (td) {
        const float4 tv = *reinterpret_cast<const float4*>(td + s0);
        t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
      }
    } else {
      n = g.E - s0 < 4 ? g.E - s0 : 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xs[k] = k < n ? yd[s0 + k] : 0.0f;
        if (td) t[k] = k < n ? td[s0 + k] : 0.0f;
      }
    }
    long long co[4] = {-1, -1, -1, -1};                  // CROP: offset inside the cropped datapoint, -1 outside the extent
    if (CROP) {
      if (RAG && VEC) {                                  // the quad lies inside one run: one row
        int e0;
        const long long rb = ragged_row(g, rrow, s0 / g.R, e0);
        e0 += s0 % g.R;
#pragma unroll
        for (int k = 0; k < 4; ++k) co[k] = (rb >= 0 && e0 + k < g.L) ? rb + ragged_elem(g, rrow, e0 + k) : -1;
      } else if (RAG) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < n) {
            int e0;
            const long long rb = ragged_row(g, rrow, (s0 + k) / g.R, e0);
            e0 += (s0 + k) % g.R;
            co[k] = (rb >= 0 && e0 < g.L) ? rb + ragged_elem(g, rrow, e0) : -1;
          }
        }
      } else if (VEC) {
        int e0;
        const int row = crop_row(g, s0 / g.R, e0);
        e0 += s0 % g.R;
#pragma unroll
        for (int k = 0; k < 4; ++k) co[k] = (row >= 0 && e0 + k < g.L) ? (long long)row + e0 + k : -1;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < n) {
            int e0;
            const int row = crop_row(g, (s0 + k) / g.R, e0);
            e0 += (s0 + k) % g.R;
            co[k] = (row >= 0 && e0 < g.L) ? (long long)row + e0 : -1;
          }
        }
      }
    }
    Elem e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      e[k] = W16 ? finish16(xs[k], x.scale, x.cap, x.bias) : finish(xs[k], x.mode);
      if (k < n) RCB_RECON_ADD_TERM(e[k], t[k], !CROP || co[k] >= 0, acc, bad);
    }
    if (CROP) {
      if (u8 || whole) {
        const long long cbase = RAG ? rrow.off : d * x.Ec;
        if (VEC && x.vec_out && (!RAG || (rrow.flags & kRaggedQuad) != 0) && co[0] >= 0 && co[3] >= 0) {
          const long long o = cbase + co[0];
          if (whole) *reinterpret_cast<float4*>(whole + o) = make_float4(e[0].v, e[1].v, e[2].v, e[3].v);
          if (u8) store_quad<W16>(u8, o, e);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (k < n && co[k] >= 0) {
              if (whole) whole[cbase + co[k]] = e[k].v;
              if (u8) store_one<W16>(u8, cbase + co[k], e[k].q);
            }
          }
        }
      }
    } else if (u8 || whole) {
      if (VEC) {
        const long long o = base + whole_offset(g, s0 / g.R, s0 % g.R);
        if (whole) *reinterpret_cast<float4*>(whole + o) = make_float4(e[0].v, e[1].v, e[2].v, e[3].v);
        if (u8) store_quad<W16>(u8, o, e);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < n) {
            const long long o = base + whole_offset(g, (s0 + k) / g.R, (s0 + k) % g.R);
            if (whole) whole[o] = e[k].v;
            if (u8) store_one<W16>(u8, o, e[k].q);
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

}  // namespace

extern "C" int64_t rcb_recon_workspace_bytes(int64_t n_data, int64_t elems_per_datapoint) {
  if (n_data <= 0 || elems_per_datapoint <= 0 || elems_per_datapoint > 0x7fffffffLL) return -1;
  const int64_t n_chunks = (elems_per_datapoint + kChunk - 1) / kChunk;
  if (n_data > 0x7fffffffLL / n_chunks) return -1;
  return n_data * n_chunks * (int64_t)(sizeof(double) + sizeof(int));
}

// THE dispatcher: the kernel of an entry -- by-value uncropped (neither), by-value cropped (crop) or per-signal (rag, which is
// cropped) -- for 8-bit / raw or 16-bit words (w16), with or without whole quads (vec)
using ReconKernel = void (*)(const float*, const float*, uint8_t*, float*, double*, int*, ReconGeo, const RaggedRow*);

template <bool CROP, bool W16, bool RAG>
static ReconKernel recon_kernel_of(bool vec) {
  return vec ? recon_kernel<true, CROP, W16, RAG> : recon_kernel<false, CROP, W16, RAG>;
}

static ReconKernel recon_kernel_of(bool vec, bool crop, bool w16, bool rag) {
  if (rag) return w16 ? recon_kernel_of<true, true, true>(vec) : recon_kernel_of<true, false, true>(vec);
  if (w16) return !crop ? recon_kernel_of<false, true, false>(vec) : recon_kernel_of<true, true, false>(vec);
  return !crop ? recon_kernel_of<false, false, false>(vec) : recon_kernel_of<true, false, false>(vec);
}

// rcb_recon_finish_ragged: the caller's tables and the device buffer their copy goes to (null `sizes` .. for the other entries)
struct RaggedArgs {
  const int32_t* sizes;
  const int64_t* spans;
  int64_t out_elems;
  void* table;
  int64_t table_bytes;
};

// The output spans of the rows: every signal dense with its axes in some order, the spans pairwise disjoint and inside
// [0, out_elems); sets the rows' flags (kRaggedQuad on the offsets and strides alone: the pointers' alignment is x.vec_out).
static int ragged_spans(const char* who, std::vector<RaggedRow>& rows, int channels, long long out_elems) {
  std::vector<std::pair<long long, long long>> ranges;
  ranges.reserve(rows.size());
  for (size_t d = 0; d < rows.size(); ++d) {
    RaggedRow& r = rows[d];
    int ax[3] = {0, 1, 2};
    std::sort(ax, ax + 3, [&](int a, int b) { return r.as[a] != r.as[b] ? r.as[a] < r.as[b] : a > b; });
    long long want = channels;
    for (int i = 0; i < 3; ++i) {
      const int a = ax[i];
      if (r.sz[a] == 1) continue;
      RCB_REQUIRE(r.as[a] == want, RCB_ERR_SHAPE,
                  "%s: signal %lld is not dense (a stride of %lld where %lld would continue the axes below it)", who, (long long)d,
                  r.as[a], want);
      want *= r.sz[a];                                       // (<= E * channels < 2^36)
    }
    RCB_REQUIRE(r.off <= out_elems && want <= out_elems - r.off, RCB_ERR_SHAPE,
                "%s: signal %lld spans [%lld, %lld) of an output of %lld elements", who, (long long)d, r.off, r.off + want, out_elems);
    ranges.emplace_back(r.off, r.off + want);
    const long long L = (long long)r.sz[2] * channels;
    const bool dense = r.sz[2] == 1 || r.as[2] == channels;
    bool quad = dense && L % 4 == 0 && r.off % 4 == 0;
    for (int i = 0; i < 2; ++i) quad = quad && (r.sz[i] == 1 || r.as[i] % 4 == 0);
    r.flags = (dense ? kRaggedDense : 0) | (quad ? kRaggedQuad : 0);
  }
  std::sort(ranges.begin(), ranges.end());
  for (size_t i = 1; i < ranges.size(); ++i)
    RCB_REQUIRE(ranges[i].first >= ranges[i - 1].second, RCB_ERR_SHAPE, "%s: the spans [%lld, %lld) and [%lld, %lld) overlap", who,
                ranges[i - 1].first, ranges[i - 1].second, ranges[i].first, ranges[i].second);
  return RCB_OK;
}

// all entries: `size` null is the uncropped form (every datapoint fills its grid); `fmt`: rcb_recon_finish_fmt, which alone takes
// modes 2 (u16 at `depth`) and 3 (s16), `u8` then addressing 16-bit words; `rag`: rcb_recon_finish_ragged (fmt, size null: the
// extents are per signal)
static int finish_entry(const char* who, bool fmt, const float* y, const float* target, int64_t n_rows, int32_t n_pix,
                        int32_t channels, int32_t nd, const int32_t* patch_nums, const int32_t* patch_size, const int32_t* size,
                        int32_t mode, int32_t depth, uint8_t* u8, float* whole, double* sse, int32_t* n_bad, void* workspace,
                        int64_t workspace_bytes, rcb_stream_t stream, const RaggedArgs* rag = nullptr) {
  if (rag && n_rows == 0) {                                  // no signals: nothing to validate against, nothing launched
    RCB_REQUIRE(mode >= 0 && mode <= 3, RCB_ERR_ARG, "%s: mode %d (0 = 8-bit, 1 = raw, 2 = u16, 3 = s16)", who, mode);
    return RCB_OK;
  }
  RCB_REQUIRE(y && workspace, RCB_ERR_ARG, "%s: null y or workspace", who);
  if (fmt) {
    if (const int err = check_mode_fmt(who, mode, depth)) return err;
  } else {
    RCB_REQUIRE(mode == 0 || mode == 1, RCB_ERR_ARG, "%s: mode %d (0 = 8-bit, 1 = raw)", who, mode);
  }
  RCB_REQUIRE(nd >= (size || rag ? 1 : 0) && nd <= 3, RCB_ERR_UNSUPPORTED, "%s: %d grid dimensions (%d .. 3)", who, nd,
              size || rag ? 1 : 0);
  RCB_REQUIRE(nd == 0 || (patch_nums && patch_size), RCB_ERR_ARG, "%s: null patch geometry", who);
  RCB_REQUIRE(channels >= 1 && channels <= 32, RCB_ERR_SHAPE, "%s: %d channels (1 .. 32)", who, channels);
  RCB_REQUIRE(n_rows > 0 && n_pix > 0, RCB_ERR_SHAPE, "%s: %lld rows of %d pixels", who, (long long)n_rows, n_pix);
  RCB_REQUIRE(!(u8 && mode == 1), RCB_ERR_ARG, "%s: the raw mode has no %s output", who, fmt ? "integer" : "8-bit");
  RCB_REQUIRE(!(sse && !target), RCB_ERR_ARG, "%s: sse needs a target", who);
  ReconGeo x;
  PatchGeo& g = x.g;
  long long per, P;
  if (const int err = grid_axes(who, nd, patch_nums, patch_size, size, nullptr, g, per, P)) return err;
  if (nd == 0) g.ps[2] = g.sz[2] = n_pix, P = n_pix;        // the rows are datapoints: one run each
  RCB_REQUIRE(P == n_pix, RCB_ERR_SHAPE, "%s: the patch has %lld pixels, the rows %d", who, P, n_pix);
  RCB_REQUIRE(n_rows % per == 0, RCB_ERR_SHAPE, "%s: %lld rows are no whole number of datapoints of %lld patches", who,
              (long long)n_rows, per);
  RCB_REQUIRE(per * P <= 0x7fffffffLL, RCB_ERR_UNSUPPORTED, "%s: %lld pixels per datapoint (elements: up to 2^31 - 1)", who,
              per * P);                                      // (per, P < 2^31: the product fits 64 bits)
  const long long E = per * P * channels;
  RCB_REQUIRE(E <= 0x7fffffffLL, RCB_ERR_UNSUPPORTED, "%s: %lld elements per datapoint (up to 2^31 - 1)", who, E);
  const long long n_data = n_rows / per;
  const int64_t need = rcb_recon_workspace_bytes(n_data, E);
  RCB_REQUIRE(need > 0, RCB_ERR_UNSUPPORTED, "%s: %lld datapoints of %lld elements need more than 2^31 - 1 workgroups", who,
              n_data, E);
  RCB_REQUIRE(workspace_bytes >= need && aligned(workspace, 8), RCB_ERR_SHAPE,
              "%s: workspace of %lld bytes (8-byte aligned), %lld needed", who, (long long)workspace_bytes, (long long)need);
  grid_elems(g, channels, E);
  x.mode = mode;
  const bool w16 = mode >= 2;
  const SampleRule16 rule = sample_rule16(mode, depth);
  x.scale = rule.scale, x.cap = rule.cap, x.bias = rule.bias;
  const uintptr_t q_align = w16 ? 8 : 4;                     // a quad of the integer output
  const long long blocks = n_data * g.n_chunks;
  double* part_sse = static_cast<double*>(workspace);
  int* part_bad = reinterpret_cast<int*>(part_sse + blocks);
  hipStream_t st = (hipStream_t)stream;
  // the 16-byte loads need only the inputs aligned; where the outputs are cropped the stores go by quad (vec_out), the cropped
  // rows seldom being multiples of 4 -- uncropped, a quad of the outputs is a quad of the inputs and vec covers both
  bool vec = g.R % 4 == 0 && aligned(y, 16) && (!target || aligned(target, 16));
  const bool out_aligned = (!whole || aligned(whole, 16)) && (!u8 || aligned(u8, q_align));
  const RaggedRow* table = nullptr;
  x.vec_out = 0, x.Ec = 0;
  if (rag) {
    RCB_REQUIRE(rag->sizes && rag->spans && rag->table, RCB_ERR_ARG, "%s: null sizes, spans or table", who);
    const int64_t tb = rcb_ragged_table_bytes(n_data);
    RCB_REQUIRE(tb > 0 && rag->table_bytes >= tb && aligned(rag->table, 8), RCB_ERR_SHAPE,
                "%s: table of %lld bytes (8-byte aligned), %lld needed", who, (long long)rag->table_bytes, (long long)tb);
    RCB_REQUIRE(rag->out_elems >= 0, RCB_ERR_SHAPE, "%s: an output of %lld elements", who, (long long)rag->out_elems);
    std::vector<RaggedRow> rows((size_t)n_data);
    std::vector<long long> reach((size_t)n_data);
    if (const int err = ragged_rows(who, n_data, nd, g, channels, 1, rag->sizes, rag->spans, rows.data(), reach.data())) return err;
    if (const int err = ragged_spans(who, rows, channels, rag->out_elems)) return err;
    if (const int err = ragged_upload(who, rows.data(), n_data, rag->table, st)) return err;
    x.vec_out = out_aligned;                                 // (the rest is the row's kRaggedQuad)
    table = static_cast<const RaggedRow*>(rag->table);
  } else if (size) {
    x.Ec = (long long)g.sz[0] * g.sz[1] * g.L;               // (L <= E: the products fit)
    x.vec_out = g.L % 4 == 0 && out_aligned;
  } else {
    vec = vec && out_aligned;
  }
  recon_kernel_of(vec, size || rag, w16, rag != nullptr)<<<(unsigned)blocks, kThreads, 0, st>>>(y, target, u8, whole, part_sse,
                                                                                                part_bad, x, table);
  RCB_LAUNCH_CHECK();
  if (sse || n_bad) {
    recon_reduce_kernel<<<(unsigned)n_data, kThreads, 0, st>>>(part_sse, part_bad, g.n_chunks, sse, n_bad);
    RCB_LAUNCH_CHECK();
  }
  return RCB_OK;
}

extern "C" int rcb_recon_finish(const float* y, const float* target, int64_t n_rows, int32_t n_pix, int32_t channels, int32_t nd,
                                const int32_t* patch_nums, const int32_t* patch_size, int32_t mode, uint8_t* u8, float* whole,
                                double* sse, int32_t* n_bad, void* workspace, int64_t workspace_bytes, rcb_stream_t stream) {
  return finish_entry("recon_finish", false, y, target, n_rows, n_pix, channels, nd, patch_nums, patch_size, nullptr, mode, 0, u8,
                      whole, sse, n_bad, workspace, workspace_bytes, stream);
}

extern "C" int rcb_recon_finish_crop(const float* y, const float* target, int64_t n_rows, int32_t n_pix, int32_t channels,
                                     int32_t nd, const int32_t* patch_nums, const int32_t* patch_size, const int32_t* size,
                                     int32_t mode, uint8_t* u8, float* whole, double* sse, int32_t* n_bad, void* workspace,
                                     int64_t workspace_bytes, rcb_stream_t stream) {
  RCB_REQUIRE(size, RCB_ERR_ARG, "recon_finish_crop: null size");
  return finish_entry("recon_finish_crop", false, y, target, n_rows, n_pix, channels, nd, patch_nums, patch_size, size, mode, 0, u8,
                      whole, sse, n_bad, workspace, workspace_bytes, stream);
}

extern "C" int rcb_recon_finish_fmt(const float* y, const float* target, int64_t n_rows, int32_t n_pix, int32_t channels, int32_t nd,
                                    const int32_t* patch_nums, const int32_t* patch_size, const int32_t* size, int32_t mode,
                                    int32_t depth, void* q_out, float* whole, double* sse, int32_t* n_bad, void* workspace,
                                    int64_t workspace_bytes, rcb_stream_t stream) {
  return finish_entry("recon_finish_fmt", true, y, target, n_rows, n_pix, channels, nd, patch_nums, patch_size, size, mode, depth,
                      static_cast<uint8_t*>(q_out), whole, sse, n_bad, workspace, workspace_bytes, stream);
}

extern "C" int rcb_recon_finish_ragged(const float* y, const float* target, int64_t n_rows, int32_t n_pix, int32_t channels,
                                       int32_t nd, const int32_t* patch_nums, const int32_t* patch_size, const int32_t* sizes,
                                       const int64_t* spans, int64_t out_elems, int32_t mode, int32_t depth, void* q_out,
                                       float* whole, double* sse, int32_t* n_bad, void* workspace, int64_t workspace_bytes,
                                       void* table, int64_t table_bytes, rcb_stream_t stream) {
  const RaggedArgs rag = {sizes, spans, out_elems, table, table_bytes};
  return finish_entry("recon_finish_ragged", true, y, target, n_rows, n_pix, channels, nd, patch_nums, patch_size, nullptr, mode,
                      depth, static_cast<uint8_t*>(q_out), whole, sse, n_bad, workspace, workspace_bytes, stream, &rag);
}
