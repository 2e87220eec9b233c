// N4 (414, 415): SSIM and the sums of MS-SSIM on the device, on the integers the decoder delivers against the integers of the source
// (Wang et al. 2004; the reference has no such figure: its utils.py:200-260 reports PSNR alone).
//
// rcb_ssim reads two operands [n][H][W][C] of uint8 or 16-bit unsigned samples through element strides -- rcb_signal_patch's
// addressing rule, 64-bit offsets -- and writes, per (image, scale, channel), two int64 fixed-point sums over the "valid" window
// positions: sum rint(ssim * 2^36) and sum rint(cs * 2^36); optionally the fp64 {ssim, cs} map of scale 0.
//
// The definition, fixed in include/rcb.h and restated by tests/ssim_emul.py (every product and sum one IEEE fp64 operation,
// contraction off):
//   window   11 taps w, formed by the HOST and passed in, as are C1 and C2: the device evaluates no exp and no constant of its own
//   filter   separable, the last spatial axis first, taps ascending, the first product starting the sum:
//              t(r, x) = ((w0 v(r, x) + w1 v(r, x+1)) + ...) + w10 v(r, x+10),   m(y, x) the same over t(y+i, x)
//            for v in {a, b, a a, b b, a b} (the products exact in fp64)
//   formula  maa = ma ma, mbb = mb mb, mab = ma mb;  saa = m(aa) - maa, sbb = m(bb) - mbb, sab = m(ab) - mab (not clamped)
//            cs = (2 sab + C2) / ((saa + sbb) + C2),  l = (2 mab + C1) / ((maa + mbb) + C1),  ssim = l cs
//   scales   scale s works on floor(H / 2^s) x floor(W / 2^s); a sample is the INTEGER sum of its 2^s x 2^s block (a trailing odd
//            row or column dropped at each halving), used as sum * 4^-s in fp64 -- exact, and so are its squares (< 2^48)
//
// Kernels.  ssim_kernel: one workgroup of 256 threads per tile of kT x kT = 16 x 16 window positions of one image, looping over
// the channels.  Per channel the (kT + 10)^2 halo of both operands is staged in LDS as the exact integers (block sums < 2^24);
// the row pass writes the five row-filtered maps [kT + 10][kT] to LDS as fp64; the column pass, the formula and the fixed-point
// terms follow, one position per thread.  LDS: the column pass reads 8 bytes per lane at a row pitch of kT doubles, so the 32
// lanes of a half-wave cover two rows = 64 consecutive banks: conflict-free.  The integer halo has a row pitch of 48 words
// (= 16 mod 32): the two rows a half-wave reads in the row pass lie on disjoint banks.  27 KiB of LDS per workgroup.
// The terms are integers, so their sum has no order: the 64 lanes by the xor butterfly, the four waves through LDS, then one
// 64-bit vector atomic add per workgroup, channel and sum on `sums`, which the entry zeroes first (a memset node on the stream).
// A sum is therefore bitwise the same alone, in a batch, in any batch order and from run to run.
// pool_kernel: the block sums of scale s from those of scale s - 1 (scale 0: the samples), both operands, into the workspace as
// uint32 [n][Hs][Ws][C].
//
// rcb_ssim_list (415; template parameter RAG of both kernels, as in signal.hip and recon.hip): a LIST of images of mixed sizes and
// memory layouts in one memset, scales - 1 pool launches and `scales` ssim launches, whatever the length of the list.  The host
// entry plans the list (rcb_ssim_list_plan: per scale and image the first tile, the first pooling workgroup, the workspace offset
// and the extent), validates the caller's tables and writes a device table: per scale and image one ListRow (the two operands'
// offsets and strides at that scale, the extent) and per scale two exclusive int32 prefixes of n + 1 entries, of tiles and of
// pooling workgroups.  With RAG a workgroup finds its image by a binary search of its block index in the prefix -- the index is
// uniform, so the probes are uniform loads -- takes the row, and runs the tile body below unchanged: the same halo, passes,
// butterfly and atomic.  Image k's terms are therefore the integers rcb_ssim adds for that image alone, and so is their sum.
// RAG false is the code rcb_ssim launches and never reads the table.
#include <algorithm>
#include <vector>

#include "rcb_common.h"

#pragma clang fp contract(off)

using namespace rcb;

namespace {

constexpr int kThreads = 256;
constexpr int kT = 16;                     // tile edge, both axes (tests/test_hip_ssim.py states it)
constexpr int kTaps = 11;
constexpr int kHalo = kT + kTaps - 1;      // 26
constexpr int kHaloPitch = 48;             // words per halo row: 16 mod 32 (see above)
constexpr int kMaxScales = 5;
constexpr long long kMaxPositions = 1ll << 26;

// an operand at one scale: kind 0 = uint8, 2 = 16-bit unsigned, 4 = the uint32 block sums of the workspace
struct Src {
  const void* p;
  int kind;
  long long st[4];                         // elements: image, row, column, channel
};

struct SsimArgs {
  Src a, b;
  int H, W, C;                             // this scale's extent
  int Ho, Wo;                              // window positions: H - 10, W - 10
  int tiles_x, tiles_y;
  double inv;                              // 4^-s
  double w[kTaps];
  double c1, c2;
  long long* sums;                         // this scale's [C][2] of image 0
  long long sums_image_stride;             // scales * C * 2
  double* map;                             // scale 0 only, nullable
};

struct PoolArgs {
  Src a, b;                                // the finer scale
  uint32_t* out_a;
  uint32_t* out_b;
  int Hs, Ws, C;                           // the coarser extent
  long long total;                         // n * Hs * Ws * C
};

// rcb_ssim_list: one image at one scale, as the device table holds it (offsets and strides in elements of that scale's operand:
// the caller's buffers at scale 0, the workspace above)
struct ListRow {
  long long a_off, a_st[3];                // the first element, then the row, column and channel strides
  long long b_off, b_st[3];
  int H, W;                                // this scale's extent
};

// what a RAG launch reads besides its SsimArgs / PoolArgs (RAG false: never read)
struct ListArgs {
  const ListRow* row;                      // [n] rows of this scale
  const ListRow* src;                      // (pool) [n] rows of the finer scale
  const int* first;                        // [n + 1] exclusive prefix of this launch's workgroups per image; first[n] = the grid
  int n;
};

// the image of workgroup `blk`: the k with first[k] <= blk < first[k + 1] (every image has at least one workgroup, so the prefix
// is strictly increasing).  blk is uniform over the workgroup, and so is every probe.
__device__ __forceinline__ int image_of(const int* __restrict__ first, int n, int blk) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= blk) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ unsigned load_sample(const Src& s, long long off) {
  if (s.kind == 0) return static_cast<const uint8_t*>(s.p)[off];
  if (s.kind == 2) return static_cast<const uint16_t*>(s.p)[off];
  return static_cast<const uint32_t*>(s.p)[off];
}

// RAG: workgroup blockIdx.x covers kThreads consecutive outputs of ONE image (t.first: the prefix of pooling workgroups); the finer
// scale's offsets and strides come from t.src, the places of the two outputs and the coarser extent from t.row.
template <bool RAG>
__global__ void __launch_bounds__(kThreads) pool_kernel(PoolArgs x, ListArgs t) {
  long long i = (long long)blockIdx.x * kThreads + threadIdx.x, total = x.total, step = (long long)gridDim.x * kThreads;
  int Hs = x.Hs, Ws = x.Ws;
  long long ast[3] = {x.a.st[1], x.a.st[2], x.a.st[3]}, bst[3] = {x.b.st[1], x.b.st[2], x.b.st[3]};
  long long a_off = 0, b_off = 0;
  uint32_t* out_a = x.out_a;
  uint32_t* out_b = x.out_b;
  if (RAG) {
    const int k = image_of(t.first, t.n, (int)blockIdx.x);
    const ListRow src = t.src[k];
    const ListRow dst = t.row[k];
    Hs = dst.H, Ws = dst.W;
    i = (long long)((int)blockIdx.x - t.first[k]) * kThreads + threadIdx.x;
    total = (long long)Hs * Ws * x.C;
    step = total;                                            // one pass
    a_off = src.a_off, b_off = src.b_off;
#pragma unroll
    for (int j = 0; j < 3; ++j) ast[j] = src.a_st[j], bst[j] = src.b_st[j];
    out_a += dst.a_off, out_b += dst.b_off;
  }
  for (; i < total; i += step) {
    const int c = (int)(i % x.C);
    long long r = i / x.C;
    const int px = (int)(r % Ws);
    r /= Ws;
    const int py = (int)(r % Hs);
    const long long n = r / Hs;
    const long long ia = RAG ? a_off : n * x.a.st[0], ib = RAG ? b_off : n * x.b.st[0];
    unsigned sa = 0, sb = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const long long y = 2 * py + dy, xx = 2 * px + dx;
        sa += load_sample(x.a, ia + y * ast[0] + xx * ast[1] + c * ast[2]);
        sb += load_sample(x.b, ib + y * bst[0] + xx * bst[1] + c * bst[2]);
      }
    }
    out_a[i] = sa;
    out_b[i] = sb;
  }
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// RAG: workgroup blockIdx.x is one tile of ONE image (t.first: the prefix of tiles); the extent, the offsets and the strides come
// from that image's row and x.H .. x.tiles_y, x.a.st, x.b.st are not read.  x.map is null.
template <bool RAG>
__global__ void __launch_bounds__(kThreads) ssim_kernel(SsimArgs x, ListArgs t) {
  __shared__ unsigned s_a[kHalo * kHaloPitch];
  __shared__ unsigned s_b[kHalo * kHaloPitch];
  __shared__ double s_t[5][kHalo][kT];
  __shared__ long long s_red[2][kThreads / kWave];

  const int tid = threadIdx.x;
  long long blk = blockIdx.x;
  int H = x.H, W = x.W, Ho = x.Ho, Wo = x.Wo, tx, ty;
  long long n, a_off = 0, b_off = 0;
  long long ast[3] = {x.a.st[1], x.a.st[2], x.a.st[3]}, bst[3] = {x.b.st[1], x.b.st[2], x.b.st[3]};
  if (RAG) {
    const int k = image_of(t.first, t.n, (int)blockIdx.x);
    const ListRow row = t.row[k];
    H = row.H, W = row.W;
    Ho = H - (kTaps - 1), Wo = W - (kTaps - 1);
    const int local = (int)blockIdx.x - t.first[k], tiles_x = (Wo + kT - 1) / kT;
    tx = local % tiles_x, ty = local / tiles_x;
    n = k;
    a_off = row.a_off, b_off = row.b_off;
#pragma unroll
    for (int j = 0; j < 3; ++j) ast[j] = row.a_st[j], bst[j] = row.b_st[j];
  } else {
    tx = (int)(blk % x.tiles_x);
    blk /= x.tiles_x;
    ty = (int)(blk % x.tiles_y);
    n = blk / x.tiles_y;
  }
  const long long ia = RAG ? a_off : n * x.a.st[0], ib = RAG ? b_off : n * x.b.st[0];
  const int y0 = ty * kT, x0 = tx * kT;
  const int py = tid / kT, px = tid % kT;
  const bool inside = y0 + py < Ho && x0 + px < Wo;

  for (int c = 0; c < x.C; ++c) {
    // the halo of both operands, as the exact integers; a position outside the image holds 0 and feeds masked positions only
    for (int i = tid; i < kHalo * kHalo; i += kThreads) {
      const int r = i / kHalo, q = i % kHalo;
      const long long gy = y0 + r, gx = x0 + q;
      unsigned va = 0, vb = 0;
      if (gy < H && gx < W) {
        va = load_sample(x.a, ia + gy * ast[0] + gx * ast[1] + c * ast[2]);
        vb = load_sample(x.b, ib + gy * bst[0] + gx * bst[1] + c * bst[2]);
      }
      s_a[r * kHaloPitch + q] = va;
      s_b[r * kHaloPitch + q] = vb;
    }
    __syncthreads();
    // row pass: the last spatial axis first
    for (int i = tid; i < kHalo * kT; i += kThreads) {
      const int r = i / kT, q = i % kT;
      double ta, tb, taa, tbb, tab;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        const double a = (double)s_a[r * kHaloPitch + q + k] * x.inv;
        const double b = (double)s_b[r * kHaloPitch + q + k] * x.inv;
        const double wk = x.w[k];
        const double pa = wk * a, pb = wk * b, paa = wk * (a * a), pbb = wk * (b * b), pab = wk * (a * b);
        if (k == 0) {
          ta = pa, tb = pb, taa = paa, tbb = pbb, tab = pab;
        } else {
          ta = ta + pa, tb = tb + pb, taa = taa + paa, tbb = tbb + pbb, tab = tab + pab;
        }
      }
      s_t[0][r][q] = ta;
      s_t[1][r][q] = tb;
      s_t[2][r][q] = taa;
      s_t[3][r][q] = tbb;
      s_t[4][r][q] = tab;
    }
    __syncthreads();
    // column pass, the formula and the fixed-point terms: one position per thread
    double m[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      double acc = x.w[0] * s_t[j][py][px];
#pragma unroll
      for (int k = 1; k < kTaps; ++k) acc = acc + x.w[k] * s_t[j][py + k][px];
      m[j] = acc;
    }
    const double maa = m[0] * m[0], mbb = m[1] * m[1], mab = m[0] * m[1];
    const double saa = m[2] - maa, sbb = m[3] - mbb, sab = m[4] - mab;
    const double cs = (2.0 * sab + x.c2) / ((saa + sbb) + x.c2);
    const double l = (2.0 * mab + x.c1) / ((maa + mbb) + x.c1);
    const double ssim = l * cs;
    long long f_ssim = 0, f_cs = 0;
    if (inside) {
      f_ssim = __double2ll_rn(ssim * RCB_SSIM_FX_SCALE);
      f_cs = __double2ll_rn(cs * RCB_SSIM_FX_SCALE);
      if (!RAG && x.map) {                                   // (the list form has no map)
        double* o = x.map + (((n * Ho + (y0 + py)) * Wo + (x0 + px)) * x.C + c) * 2;
        o[0] = ssim;
        o[1] = cs;
      }
    }
    f_ssim = wave_sum_i64(f_ssim);
    f_cs = wave_sum_i64(f_cs);
    if ((tid & 63) == 0) {
      s_red[0][tid >> 6] = f_ssim;
      s_red[1][tid >> 6] = f_cs;
    }
    __syncthreads();                                         // (also: s_a / s_b / s_t are free for the next channel)
    if (tid < 2) {
      long long v = s_red[tid][0];
      for (int wv = 1; wv < kThreads / kWave; ++wv) v += s_red[tid][wv];
      atomicAdd(reinterpret_cast<unsigned long long*>(x.sums + n * x.sums_image_stride + c * 2 + tid), (unsigned long long)v);
    }
    // s_red is written again only after the next channel's two barriers, which threads 0 and 1 reach after reading it
  }
}

bool is_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// elements (uint32) of one operand's block sums at scale s >= 1, rounded up to a 16-byte multiple
long long level_elems(long long n, int H, int W, int C, int s) { return (n * (H >> s) * (W >> s) * C + 3) / 4 * 4; }

// the shape rules shared by the two entries -> 0, or the code (the message names `who`)
int check_shape(const char* who, int64_t n_img, int32_t H, int32_t W, int32_t C, int32_t scales) {
  RCB_REQUIRE(n_img >= 0, RCB_ERR_SHAPE, "%s: %lld images", who, (long long)n_img);
  RCB_REQUIRE(C >= 1 && C <= 32, RCB_ERR_SHAPE, "%s: %d channels (1 .. 32)", who, C);
  RCB_REQUIRE(H >= kTaps && W >= kTaps, RCB_ERR_SHAPE, "%s: an image of %d x %d (both sides at least %d)", who, H, W, kTaps);
  RCB_REQUIRE(scales >= 1 && scales <= kMaxScales, RCB_ERR_ARG, "%s: %d scales (1 .. %d)", who, scales, kMaxScales);
  RCB_REQUIRE((H >> (scales - 1)) >= kTaps && (W >> (scales - 1)) >= kTaps, RCB_ERR_SHAPE,
              "%s: %d scales need both sides of %d x %d to be at least %d", who, scales, H, W, kTaps << (scales - 1));
  RCB_REQUIRE((long long)(H - 10) * (W - 10) <= kMaxPositions, RCB_ERR_UNSUPPORTED,
              "%s: %lld window positions per image (up to 2^26: the fixed-point sums stay below 2^62)", who,
              (long long)(H - 10) * (W - 10));
  const long long tiles = (long long)cdiv(H - 10, kT) * cdiv(W - 10, kT);
  RCB_REQUIRE(n_img == 0 || n_img <= 0x7fffffffLL / tiles, RCB_ERR_UNSUPPORTED,
              "%s: %lld images of %lld tiles need more than 2^31 - 1 workgroups", who, (long long)n_img, tiles);
  return RCB_OK;
}

// the sample formats SSIM is defined for, shared by the two entries
int check_format(const char* who, int32_t kind, int32_t depth) {
  RCB_REQUIRE(kind == 0 || kind == 2, RCB_ERR_ARG, "%s: kind %d (0 = uint8, 2 = u16; fp32 and s16 sources have no SSIM here)", who,
              kind);
  RCB_REQUIRE(kind == 2 ? (depth >= 9 && depth <= 16) : depth == 0, RCB_ERR_ARG, "%s: depth %d for kind %d (9 .. 16 for u16, 0 for uint8)",
              who, depth, kind);
  return RCB_OK;
}

// ---- rcb_ssim_list: the plan (host arithmetic) and the device table built from it --------------------------------------------------
// plan: int64 [scales][n][kPlanCols] = {first tile, first pooling workgroup, workspace offset (uint32 elements) of operand a's block
// sums -- b's follow at + level_elems(1, H, W, C, s) --, H_s, W_s}, then [scales][2] = {tiles, pooling workgroups} of the scale.
// Scale 0 pools nothing and has no workspace: its columns 1 and 2 and its second total are 0.
constexpr int kPlanCols = 5;
long long plan_ints(long long n, int scales) { return (long long)scales * (n * kPlanCols + 2); }

// device table: ListRow [scales][n], then int32 [scales][2][n + 1]: per scale the prefix of tiles and the prefix of pooling
// workgroups, each closed by its total
long long table_rows_bytes(long long n, int scales) { return (long long)scales * n * (long long)sizeof(ListRow); }
long long list_table_bytes(long long n, int scales) {
  return table_rows_bytes(n, scales) + ((long long)scales * 2 * (n + 1) * (long long)sizeof(int) + 7) / 8 * 8;
}
constexpr long long kMaxListImages = 1ll << 24;              // (the plan's length is returned as an int)

// one operand's spans of the list -> 0 or the code: non-negative, and every element of every image inside [0, elems)
int check_spans(const char* who, const char* name, long long n, const int32_t* sizes, const int64_t* spans, int C, int64_t elems) {
  for (long long k = 0; k < n; ++k) {
    const int64_t* sp = spans + 4 * k;
    for (int i = 0; i < 4; ++i)
      RCB_REQUIRE(sp[i] >= 0, RCB_ERR_ARG, "%s: image %lld: a negative %s of %s (%lld)", who, k, i == 0 ? "offset" : "stride", name,
                  (long long)sp[i]);
    // (no overflow: the extents are below 2^27 and C <= 32, so an element offset that fits a buffer is far below 2^63; a stride
    // that overflows the product is caught by the division)
    const long long dims[3] = {sizes[2 * k] - 1, sizes[2 * k + 1] - 1, C - 1};
    long long reach = sp[0];
    bool fits = reach < elems;
    for (int i = 0; i < 3 && fits; ++i) {
      fits = dims[i] == 0 || sp[i + 1] <= (elems - 1 - reach) / dims[i];
      if (fits) reach += dims[i] * sp[i + 1];
    }
    RCB_REQUIRE(fits, RCB_ERR_SHAPE, "%s: image %lld reaches past the %lld elements of %s", who, k, (long long)elems, name);
  }
  return RCB_OK;
}

int upload(const char* who, const void* host, size_t bytes, void* table, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(table, host, bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail((int)e, "%s: table upload failed: %s", who, hipGetErrorString(e));
  return RCB_OK;
}

}  // namespace

extern "C" int64_t rcb_ssim_workspace_bytes(int64_t n_img, int32_t H, int32_t W, int32_t C, int32_t scales) {
  if (check_shape("ssim_workspace_bytes", n_img, H, W, C, scales)) return -1;
  long long elems = 0;
  for (int s = 1; s < scales; ++s) elems += 2 * level_elems(n_img, H, W, C, s);      // (n * tiles < 2^31: below 2^43)
  return elems * (int64_t)sizeof(uint32_t);
}

extern "C" int rcb_ssim(const void* a, const void* b, int32_t kind, int32_t depth, int64_t n_img, int32_t H, int32_t W, int32_t C,
                        const int64_t* a_strides, const int64_t* b_strides, const double* win, double c1, double c2, int32_t scales,
                        int64_t* sums, double* map, void* workspace, int64_t workspace_bytes, rcb_stream_t stream) {
  const char* who = "ssim";
  if (const int err = check_format(who, kind, depth)) return err;
  if (const int err = check_shape(who, n_img, H, W, C, scales)) return err;
  RCB_REQUIRE(a_strides && b_strides && win, RCB_ERR_ARG, "%s: null strides or window", who);
  for (int i = 0; i < 4; ++i)
    RCB_REQUIRE(a_strides[i] >= 0 && b_strides[i] >= 0, RCB_ERR_ARG, "%s: a negative stride (%lld, %lld at entry %d)", who,
                (long long)a_strides[i], (long long)b_strides[i], i);
  if (n_img == 0) return RCB_OK;
  RCB_REQUIRE(a && b && sums, RCB_ERR_ARG, "%s: null a, b or sums", who);
  RCB_REQUIRE(is_aligned(sums, 8) && (!map || is_aligned(map, 8)), RCB_ERR_ARG, "%s: sums and map must be 8-byte aligned", who);
  const int64_t need = rcb_ssim_workspace_bytes(n_img, H, W, C, scales);
  RCB_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && is_aligned(workspace, 16)), RCB_ERR_SHAPE,
              "%s: workspace of %lld bytes (16-byte aligned), %lld needed", who, (long long)workspace_bytes, (long long)need);

  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(sums, 0, (size_t)n_img * scales * C * 2 * sizeof(int64_t), st);
  if (e != hipSuccess) return fail((int)e, "%s: clearing the sums failed: %s", who, hipGetErrorString(e));

  SsimArgs x;
  x.a.p = a, x.b.p = b;
  x.a.kind = x.b.kind = kind;
  for (int i = 0; i < 4; ++i) x.a.st[i] = a_strides[i], x.b.st[i] = b_strides[i];
  for (int k = 0; k < kTaps; ++k) x.w[k] = win[k];
  x.c1 = c1, x.c2 = c2;
  x.C = C;
  x.sums_image_stride = (long long)scales * C * 2;
  uint32_t* level = static_cast<uint32_t*>(workspace);
  for (int s = 0; s < scales; ++s) {
    const int Hs = H >> s, Ws = W >> s;
    if (s > 0) {                                             // the block sums of this scale from the scale before
      PoolArgs p;
      p.a = x.a, p.b = x.b;
      p.Hs = Hs, p.Ws = Ws, p.C = C;
      p.total = (long long)n_img * Hs * Ws * C;
      const long long le = level_elems(n_img, H, W, C, s);
      p.out_a = level, p.out_b = level + le;
      level += 2 * le;
      const long long blocks = std::min<long long>((p.total + kThreads - 1) / kThreads, 1 << 20);
      pool_kernel<false><<<(unsigned)blocks, kThreads, 0, st>>>(p, ListArgs{});
      RCB_LAUNCH_CHECK();
      x.a.p = p.out_a, x.b.p = p.out_b;
      x.a.kind = x.b.kind = 4;
      const long long dense[4] = {(long long)Hs * Ws * C, (long long)Ws * C, C, 1};
      for (int i = 0; i < 4; ++i) x.a.st[i] = x.b.st[i] = dense[i];
    }
    x.H = Hs, x.W = Ws;
    x.Ho = Hs - (kTaps - 1), x.Wo = Ws - (kTaps - 1);
    x.tiles_y = cdiv(x.Ho, kT), x.tiles_x = cdiv(x.Wo, kT);
    x.inv = 1.0 / (double)(1ll << (2 * s));
    x.sums = reinterpret_cast<long long*>(sums) + (long long)s * C * 2;
    x.map = s == 0 ? map : nullptr;
    const long long blocks = (long long)n_img * x.tiles_y * x.tiles_x;
    ssim_kernel<false><<<(unsigned)blocks, kThreads, 0, st>>>(x, ListArgs{});
    RCB_LAUNCH_CHECK();
  }
  return RCB_OK;
}

// ---- 415: lists of images of mixed sizes -------------------------------------------------------------------------------------------
namespace {

// what every list entry checks before it looks at an image
int check_list_head(const char* who, int64_t n_img, int32_t C, int32_t scales) {
  RCB_REQUIRE(n_img >= 0 && n_img <= kMaxListImages, RCB_ERR_SHAPE, "%s: %lld images (0 .. 2^24)", who, (long long)n_img);
  RCB_REQUIRE(C >= 1 && C <= 32, RCB_ERR_SHAPE, "%s: %d channels (1 .. 32)", who, C);
  RCB_REQUIRE(scales >= 1 && scales <= kMaxScales, RCB_ERR_ARG, "%s: %d scales (1 .. %d)", who, scales, kMaxScales);
  return RCB_OK;
}

// rcb_ssim's shape rules for every image of the list, the message naming the image
int check_list_shapes(const char* who, int64_t n_img, const int32_t* sizes, int32_t C, int32_t scales) {
  if (const int err = check_list_head(who, n_img, C, scales)) return err;
  RCB_REQUIRE(n_img == 0 || sizes, RCB_ERR_ARG, "%s: null sizes", who);
  for (long long k = 0; k < n_img; ++k) {
    char name[64];
    snprintf(name, sizeof name, "%s: image %lld", who, k);
    if (const int err = check_shape(name, 1, sizes[2 * k], sizes[2 * k + 1], C, scales)) return err;
  }
  return RCB_OK;
}

}  // namespace

extern "C" int64_t rcb_ssim_list_table_bytes(int64_t n_img, int32_t scales) {
  if (check_list_head("ssim_list_table_bytes", n_img, 1, scales)) return -1;
  return list_table_bytes(n_img, scales);
}

extern "C" int64_t rcb_ssim_list_workspace_bytes(int64_t n_img, const int32_t* sizes, int32_t C, int32_t scales) {
  if (check_list_shapes("ssim_list_workspace_bytes", n_img, sizes, C, scales)) return -1;
  long long bytes = 0;                                       // (2^24 images of at most 2^26 * 32 * 2 * 4 / 3 bytes: below 2^63)
  for (long long k = 0; k < n_img; ++k) bytes += rcb_ssim_workspace_bytes(1, sizes[2 * k], sizes[2 * k + 1], C, scales);
  return bytes;
}

extern "C" int rcb_ssim_list_plan(int64_t n_img, const int32_t* sizes, int32_t C, int32_t scales, int64_t* plan, int64_t max_ints) {
  const char* who = "ssim_list_plan";
  if (const int err = check_list_shapes(who, n_img, sizes, C, scales)) return err;
  const long long ints = plan_ints(n_img, scales);
  RCB_REQUIRE(plan && max_ints >= ints, RCB_ERR_SHAPE, "%s: a plan of %lld ints, %lld needed", who, (long long)max_ints, ints);
  long long tiles[kMaxScales] = {}, groups[kMaxScales] = {}, ws = 0;
  for (long long k = 0; k < n_img; ++k) {
    const int H = sizes[2 * k], W = sizes[2 * k + 1];
    for (int s = 0; s < scales; ++s) {                       // image k's block of the workspace: rcb_ssim's layout for n_img = 1
      const int Hs = H >> s, Ws = W >> s;
      int64_t* p = plan + ((long long)s * n_img + k) * kPlanCols;
      p[0] = tiles[s], p[1] = groups[s], p[2] = s ? ws : 0, p[3] = Hs, p[4] = Ws;
      tiles[s] += (long long)cdiv(Hs - (kTaps - 1), kT) * cdiv(Ws - (kTaps - 1), kT);
      if (s) {
        groups[s] += ((long long)Hs * Ws * C + kThreads - 1) / kThreads;
        ws += 2 * level_elems(1, H, W, C, s);
      }
    }
  }
  for (int s = 0; s < scales; ++s) {
    RCB_REQUIRE(tiles[s] <= 0x7fffffffLL && groups[s] <= 0x7fffffffLL, RCB_ERR_UNSUPPORTED,
                "%s: scale %d of the list needs %lld tiles and %lld pooling workgroups (up to 2^31 - 1 each)", who, s, tiles[s], groups[s]);
    plan[n_img * scales * kPlanCols + 2 * s] = tiles[s];
    plan[n_img * scales * kPlanCols + 2 * s + 1] = groups[s];
  }
  return (int)ints;
}

extern "C" int rcb_ssim_list(const void* a, int64_t a_elems, const void* b, int64_t b_elems, int32_t kind, int32_t depth,
                             int64_t n_img, const int32_t* sizes, const int64_t* a_spans, const int64_t* b_spans, int32_t C,
                             const double* win, double c1, double c2, int32_t scales, int64_t* sums, void* workspace,
                             int64_t workspace_bytes, void* table, int64_t table_bytes, rcb_stream_t stream) {
  const char* who = "ssim_list";
  if (const int err = check_format(who, kind, depth)) return err;
  if (const int err = check_list_head(who, n_img, C, scales)) return err;
  RCB_REQUIRE(win, RCB_ERR_ARG, "%s: null window", who);
  if (n_img == 0) return RCB_OK;
  RCB_REQUIRE(sizes && a_spans && b_spans && table, RCB_ERR_ARG, "%s: null sizes, spans or table", who);
  RCB_REQUIRE(a && b && sums, RCB_ERR_ARG, "%s: null a, b or sums", who);
  RCB_REQUIRE(is_aligned(sums, 8), RCB_ERR_ARG, "%s: sums must be 8-byte aligned", who);
  const long long n = n_img;
  std::vector<int64_t> plan((size_t)plan_ints(n, scales));
  const int planned = rcb_ssim_list_plan(n, sizes, C, scales, plan.data(), (int64_t)plan.size());
  if (planned < 0) return planned;
  const long long need_table = list_table_bytes(n, scales);
  RCB_REQUIRE(table_bytes >= need_table && is_aligned(table, 8), RCB_ERR_SHAPE, "%s: table of %lld bytes (8-byte aligned), %lld needed",
              who, (long long)table_bytes, need_table);
  const int64_t need = rcb_ssim_list_workspace_bytes(n, sizes, C, scales);
  RCB_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && is_aligned(workspace, 16)), RCB_ERR_SHAPE,
              "%s: workspace of %lld bytes (16-byte aligned), %lld needed", who, (long long)workspace_bytes, (long long)need);
  if (const int err = check_spans(who, "a", n, sizes, a_spans, C, a_elems)) return err;
  if (const int err = check_spans(who, "b", n, sizes, b_spans, C, b_elems)) return err;

  // the device table from the plan and the spans
  std::vector<int64_t> host((size_t)need_table / 8);
  ListRow* rows = reinterpret_cast<ListRow*>(host.data());
  int* first = reinterpret_cast<int*>(reinterpret_cast<char*>(host.data()) + table_rows_bytes(n, scales));
  const int64_t* totals = plan.data() + n * scales * kPlanCols;
  for (int s = 0; s < scales; ++s) {
    int* first_tile = first + (long long)s * 2 * (n + 1);
    int* first_group = first_tile + (n + 1);
    for (long long k = 0; k < n; ++k) {
      const int64_t* p = plan.data() + ((long long)s * n + k) * kPlanCols;
      ListRow& r = rows[(long long)s * n + k];
      r.H = (int)p[3], r.W = (int)p[4];
      if (s == 0) {
        r.a_off = a_spans[4 * k], r.b_off = b_spans[4 * k];
        for (int i = 0; i < 3; ++i) r.a_st[i] = a_spans[4 * k + 1 + i], r.b_st[i] = b_spans[4 * k + 1 + i];
      } else {                                               // dense block sums in the workspace, a's then b's
        r.a_off = p[2], r.b_off = p[2] + level_elems(1, sizes[2 * k], sizes[2 * k + 1], C, s);
        r.a_st[0] = r.b_st[0] = (long long)r.W * C, r.a_st[1] = r.b_st[1] = C, r.a_st[2] = r.b_st[2] = 1;
      }
      first_tile[k] = (int)p[0], first_group[k] = (int)p[1];
    }
    first_tile[n] = (int)totals[2 * s], first_group[n] = (int)totals[2 * s + 1];
  }
  hipStream_t st = (hipStream_t)stream;
  if (const int err = upload(who, host.data(), (size_t)need_table, table, st)) return err;
  const hipError_t e = hipMemsetAsync(sums, 0, (size_t)n * scales * C * 2 * sizeof(int64_t), st);
  if (e != hipSuccess) return fail((int)e, "%s: clearing the sums failed: %s", who, hipGetErrorString(e));

  const ListRow* d_rows = static_cast<const ListRow*>(table);
  const int* d_first = reinterpret_cast<const int*>(static_cast<const char*>(table) + table_rows_bytes(n, scales));
  SsimArgs x = {};
  for (int k = 0; k < kTaps; ++k) x.w[k] = win[k];
  x.c1 = c1, x.c2 = c2;
  x.C = C;
  x.sums_image_stride = (long long)scales * C * 2;
  x.a.p = a, x.b.p = b;
  x.a.kind = x.b.kind = kind;
  for (int s = 0; s < scales; ++s) {
    ListArgs t;
    t.row = d_rows + (long long)s * n;
    t.src = s ? d_rows + (long long)(s - 1) * n : nullptr;
    t.n = (int)n;
    if (s > 0) {                                             // the block sums of this scale from the scale before
      PoolArgs p = {};
      p.a = x.a, p.b = x.b;
      p.C = C;
      p.out_a = p.out_b = static_cast<uint32_t*>(workspace);
      t.first = d_first + ((long long)s * 2 + 1) * (n + 1);
      pool_kernel<true><<<(unsigned)totals[2 * s + 1], kThreads, 0, st>>>(p, t);
      RCB_LAUNCH_CHECK();
      x.a.p = x.b.p = workspace;
      x.a.kind = x.b.kind = 4;
    }
    x.inv = 1.0 / (double)(1ll << (2 * s));
    x.sums = reinterpret_cast<long long*>(sums) + (long long)s * C * 2;
    t.first = d_first + (long long)s * 2 * (n + 1);
    ssim_kernel<true><<<(unsigned)totals[2 * s], kThreads, 0, st>>>(x, t);
    RCB_LAUNCH_CHECK();
  }
  return RCB_OK;
}
