// N4 (418): Y'CbCr on the device -- planar 4:4:4 / 4:2:2 / 4:2:0 sources in (rcb_ycc_to_rgb), the planes of an RGB signal out
// (rcb_rgb_to_ycc), and the per-plane squared error of two RGB signals in Y'CbCr (rcb_ycc_sse): what PSNR-Y and the
// (6 Y + Cb + Cr) / 8 figure of the video codec comparisons are formed from.
//
// The definition is fixed in include/rcb.h and restated by tests/ycc_emul.py; in short, every step one IEEE fp64 operation,
// contraction off (the pragma below; the 8-bit cube test tells a contracted build apart):
//   forward   p_k = (m[k][0] r + m[k][1] g) + m[k][2] b;  Y = Q(p_0 + off[0]);  chroma 4:4:4 = Q(p_k + off[k]);
//             4:2:2 = Q((p(y, x0) + p(y, x1)) * 0.5 + off[k]);  4:2:0 = Q(((p00 + p01) + (p10 + p11)) * 0.25 + off[k]), the far row and
//             column clipped to the extent;  Q(v) = (int)rint(fmin(fmax(v, 0), L)), the ONE rounding
//   inverse   v_k = (n[k][0] (Y - o[0]) + n[k][1] (Cb - o[1])) + n[k][2] (Cr - o[2]);  q = Q(v_k);  chroma read at (y >> 1, x >> 1)
// The device evaluates no colour constant: m / off (n / o) are the caller's (utils.ycc_matrix).
//
// Kernels.  A thread owns a tile of kTH x kTW = 2 x 4 positions -- whole chroma blocks at every subsampling, so no mean crosses
// threads -- and a workgroup of 256 threads (32 across, 8 down) 16 x 128 positions of one frame.  A tile on the far edge reads the
// clipped row / column again, which IS the definition's edge replication; what lies outside the extent is neither stored nor
// summed.  No LDS but the 96 bytes of the sse reduction, no scratch.
// Memory paths.  Element by element through the strides (any layout), or -- uint8, channel stride 1, column stride 3, every row
// on a 4-byte boundary -- the 12 bytes of a tile row as three dwords (forward: loads; inverse: the stores of dst, W a multiple of
// 4).  A tile that crosses the right edge goes element by element on either path.  Only the loads and stores differ: the bits
// are the same, and the entry decides.
// rcb_ycc_sse: the integers both operands would deliver, differenced and squared as integers (a term < 2^32), summed per thread,
// per wave (xor butterfly), per workgroup (LDS), then ONE 64-bit integer atomic per workgroup and plane onto the memset row of the
// frame.  Integer sums have no order: a frame's row is bitwise the same alone, in any batch and from run to run.
#include "rcb_common.h"

#pragma clang fp contract(off)

using namespace rcb;

namespace {

constexpr int kThreads = 256;
constexpr int kTW = 4, kTH = 2;              // positions per thread: across, down (tests/test_hip_ycc.py states the tile)
constexpr int kWX = 32, kWY = 8;             // threads per workgroup: across, down -> 128 x 16 positions
constexpr long long kMaxPositions = 1ll << 26;

struct Consts {
  double m[9], off[3], L;                    // forward: m, off; inverse: n, o
};

struct RgbSrc {
  const void* p;
  long long off, st[5];                      // elements: the first sample; signal, frame, row, column, channel
};

struct Plane {
  const void* p;
  long long st[4];                           // elements: signal, frame, row, column
};

struct Geo {
  int T, H, W, Hc, Wc, ss, wgx, wgy;
};

struct TileQ {
  int y[kTH * kTW], c[2][kTH * kTW];       // c[0] Cb, c[1] Cr: chroma (ci, cj) at [ci * kTW + cj]; 4:2:2 uses cj < 2, 4:2:0 ci = 0 as well
};

template <int KIND>
__device__ __forceinline__ double load_sample(const void* p, long long o) {
  if (KIND == 0) return (double)static_cast<const uint8_t*>(p)[o];
  return (double)static_cast<const uint16_t*>(p)[o];
}

template <int KIND>
__device__ __forceinline__ void store_sample(void* p, long long o, int q) {
  if (KIND == 0) static_cast<uint8_t*>(p)[o] = (uint8_t)q;
  else static_cast<uint16_t*>(p)[o] = (uint16_t)q;
}

__device__ __forceinline__ int quantise(double v, double L) { return (int)rint(fmin(fmax(v, 0.0), L)); }

// workgroup -> (frame, y0, x0) of this thread's tile; false: the tile lies outside the extent
__device__ __forceinline__ bool tile_of(const Geo& g, long long& frame, int& y0, int& x0) {
  long long blk = blockIdx.x;
  const int bx = (int)(blk % g.wgx);
  blk /= g.wgx;
  const int by = (int)(blk % g.wgy);
  frame = blk / g.wgy;                                       // n * T + t
  x0 = (bx * kWX + (int)threadIdx.x % kWX) * kTW;
  y0 = (by * kWY + (int)threadIdx.x / kWX) * kTH;
  return y0 < g.H && x0 < g.W;
}

// the first chroma sample of a tile, and how many the tile holds down and across
__device__ __forceinline__ void chroma_of(const Geo& g, int y0, int x0, int& cy0, int& cx0, int& rows, int& cols) {
  cy0 = g.ss == 2 ? y0 >> 1 : y0, cx0 = g.ss ? x0 >> 1 : x0;
  rows = g.ss == 2 ? 1 : kTH, cols = g.ss ? kTW / 2 : kTW;
}

// The integers rcb_rgb_to_ycc delivers for one tile (y0 < H, x0 < W).  Positions outside the extent read the clipped row / column:
// their luma and whole chroma samples outside Hc x Wc are formed but are the caller's to leave out.
template <int KIND, bool FAST>
__device__ __forceinline__ void forward_tile(const RgbSrc& s, const Consts& c, const Geo& g, long long frame, int y0, int x0, TileQ& q) {
  double p[3][kTH][kTW];
  const long long base = s.off + (frame / g.T) * s.st[0] + (frame % g.T) * s.st[1];
#pragma unroll
  for (int i = 0; i < kTH; ++i) {
    const long long row = base + (long long)min(y0 + i, g.H - 1) * s.st[2];
    double r[kTW], gg[kTW], b[kTW];
    if (FAST && x0 + kTW <= g.W) {                           // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
      const uint32_t* w = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(s.p) + row + 3ll * x0);
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
      r[0] = (double)(w0 & 255u), gg[0] = (double)((w0 >> 8) & 255u), b[0] = (double)((w0 >> 16) & 255u);
      r[1] = (double)(w0 >> 24), gg[1] = (double)(w1 & 255u), b[1] = (double)((w1 >> 8) & 255u);
      r[2] = (double)((w1 >> 16) & 255u), gg[2] = (double)(w1 >> 24), b[2] = (double)(w2 & 255u);
      r[3] = (double)((w2 >> 8) & 255u), gg[3] = (double)((w2 >> 16) & 255u), b[3] = (double)(w2 >> 24);
    } else {
#pragma unroll
      for (int j = 0; j < kTW; ++j) {
        const long long o = row + (long long)min(x0 + j, g.W - 1) * s.st[3];
        r[j] = load_sample<KIND>(s.p, o);
        gg[j] = load_sample<KIND>(s.p, o + s.st[4]);
        b[j] = load_sample<KIND>(s.p, o + 2 * s.st[4]);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < kTW; ++j) p[k][i][j] = (c.m[3 * k] * r[j] + c.m[3 * k + 1] * gg[j]) + c.m[3 * k + 2] * b[j];
  }
#pragma unroll
  for (int i = 0; i < kTH; ++i)
#pragma unroll
    for (int j = 0; j < kTW; ++j) q.y[i * kTW + j] = quantise(p[0][i][j] + c.off[0], c.L);
#pragma unroll
  for (int k = 1; k < 3; ++k) {
    int* qc = q.c[k - 1];
#pragma unroll
    for (int e = 0; e < kTH * kTW; ++e) qc[e] = 0;
    if (g.ss == 0) {
#pragma unroll
      for (int i = 0; i < kTH; ++i)
#pragma unroll
        for (int j = 0; j < kTW; ++j) qc[i * kTW + j] = quantise(p[k][i][j] + c.off[k], c.L);
    } else if (g.ss == 1) {
#pragma unroll
      for (int i = 0; i < kTH; ++i)
#pragma unroll
        for (int j = 0; j < kTW / 2; ++j) qc[i * kTW + j] = quantise((p[k][i][2 * j] + p[k][i][2 * j + 1]) * 0.5 + c.off[k], c.L);
    } else {
#pragma unroll
      for (int j = 0; j < kTW / 2; ++j)
        qc[j] = quantise(((p[k][0][2 * j] + p[k][0][2 * j + 1]) + (p[k][1][2 * j] + p[k][1][2 * j + 1])) * 0.25 + c.off[k], c.L);
    }
  }
}

// pack_y: uint8, W a multiple of 4 and oy on a 4-byte boundary -- the four luma bytes of a tile row as one dword
template <int KIND, bool FAST>
__global__ void __launch_bounds__(kThreads) rgb_to_ycc_kernel(RgbSrc s, Consts c, Geo g, void* oy, void* ocb, void* ocr, int pack_y) {
  long long frame;
  int y0, x0;
  if (!tile_of(g, frame, y0, x0)) return;
  TileQ q;
  forward_tile<KIND, FAST>(s, c, g, frame, y0, x0, q);
  if (oy) {
#pragma unroll
    for (int i = 0; i < kTH; ++i) {
      const long long o = (frame * g.H + (y0 + i)) * g.W + x0;
      if (y0 + i >= g.H) {
      } else if (KIND == 0 && pack_y) {
        const uint32_t w = (uint32_t)q.y[i * kTW] | (uint32_t)q.y[i * kTW + 1] << 8 | (uint32_t)q.y[i * kTW + 2] << 16 |
                           (uint32_t)q.y[i * kTW + 3] << 24;
        *reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(oy) + o) = w;
      } else {
#pragma unroll
        for (int j = 0; j < kTW; ++j)
          if (x0 + j < g.W) store_sample<KIND>(oy, o + j, q.y[i * kTW + j]);
      }
    }
  }
  int cy0, cx0, rows, cols;
  chroma_of(g, y0, x0, cy0, cx0, rows, cols);
#pragma unroll
  for (int k = 1; k < 3; ++k) {
    void* oc = k == 1 ? ocb : ocr;
    const int* qc = q.c[k - 1];
#pragma unroll
    for (int i = 0; i < kTH; ++i)
#pragma unroll
      for (int j = 0; j < kTW; ++j)
        if (oc && i < rows && j < cols && cy0 + i < g.Hc && cx0 + j < g.Wc)
          store_sample<KIND>(oc, (frame * g.Hc + (cy0 + i)) * g.Wc + (cx0 + j), qc[i * kTW + j]);
  }
}

template <int KIND, bool FAST>
__global__ void __launch_bounds__(kThreads) ycc_sse_kernel(RgbSrc a, RgbSrc b, Consts c, Geo g, long long* sse) {
  __shared__ long long s_red[3][kThreads / kWave];
  long long frame;
  int y0, x0;
  const bool active = tile_of(g, frame, y0, x0);             // (frame is uniform over the workgroup)
  long long acc[3] = {0, 0, 0};
  if (active) {
    TileQ qa, qb;
    forward_tile<KIND, FAST>(a, c, g, frame, y0, x0, qa);
    forward_tile<KIND, FAST>(b, c, g, frame, y0, x0, qb);
    int cy0, cx0, rows, cols;
    chroma_of(g, y0, x0, cy0, cx0, rows, cols);
#pragma unroll
    for (int i = 0; i < kTH; ++i)
#pragma unroll
      for (int j = 0; j < kTW; ++j) {
        const int e = i * kTW + j;
        if (y0 + i < g.H && x0 + j < g.W) {
          const long long d = qa.y[e] - qb.y[e];
          acc[0] += d * d;
        }
        if (i < rows && j < cols && cy0 + i < g.Hc && cx0 + j < g.Wc) {
          const long long db = qa.c[0][e] - qb.c[0][e], dr = qa.c[1][e] - qb.c[1][e];
          acc[1] += db * db;
          acc[2] += dr * dr;
        }
      }
  }
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    long long v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((tid & 63) == 0) s_red[k][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < 3) {
    long long v = s_red[tid][0];
    for (int wv = 1; wv < kThreads / kWave; ++wv) v += s_red[tid][wv];
    atomicAdd(reinterpret_cast<unsigned long long*>(sse + frame * 3 + tid), (unsigned long long)v);
  }
}

// FAST: uint8, W a multiple of 4, dst on a 4-byte boundary -- the 12 bytes of a tile row as three dword stores
template <int KIND, bool FAST>
__global__ void __launch_bounds__(kThreads) ycc_to_rgb_kernel(Plane py, Plane pcb, Plane pcr, Consts c, Geo g, void* dst) {
  long long frame;
  int y0, x0;
  if (!tile_of(g, frame, y0, x0)) return;
  const long long sig = frame / g.T, fr = frame % g.T;
  const long long by = sig * py.st[0] + fr * py.st[1], bcb = sig * pcb.st[0] + fr * pcb.st[1], bcr = sig * pcr.st[0] + fr * pcr.st[1];
#pragma unroll
  for (int i = 0; i < kTH; ++i) {
    const int yy = min(y0 + i, g.H - 1);                     // (a row outside the extent is formed again, never stored)
    const int cy = g.ss == 2 ? yy >> 1 : yy;
    int q[kTW][3];
#pragma unroll
    for (int j = 0; j < kTW; ++j) {
      const int xx = min(x0 + j, g.W - 1);                   // (a position outside the extent is formed again, never stored)
      const int cx = g.ss ? xx >> 1 : xx;
      const double Y = load_sample<KIND>(py.p, by + (long long)yy * py.st[2] + (long long)xx * py.st[3]) - c.off[0];
      const double Cb = load_sample<KIND>(pcb.p, bcb + (long long)cy * pcb.st[2] + (long long)cx * pcb.st[3]) - c.off[1];
      const double Cr = load_sample<KIND>(pcr.p, bcr + (long long)cy * pcr.st[2] + (long long)cx * pcr.st[3]) - c.off[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) q[j][k] = quantise((c.m[3 * k] * Y + c.m[3 * k + 1] * Cb) + c.m[3 * k + 2] * Cr, c.L);
    }
    const long long o = ((frame * g.H + yy) * g.W + x0) * 3;
    if (y0 + i >= g.H) {
    } else if (FAST && x0 + kTW <= g.W) {
      uint32_t* w = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(dst) + o);
      w[0] = (uint32_t)q[0][0] | (uint32_t)q[0][1] << 8 | (uint32_t)q[0][2] << 16 | (uint32_t)q[1][0] << 24;
      w[1] = (uint32_t)q[1][1] | (uint32_t)q[1][2] << 8 | (uint32_t)q[2][0] << 16 | (uint32_t)q[2][1] << 24;
      w[2] = (uint32_t)q[2][2] | (uint32_t)q[3][0] << 8 | (uint32_t)q[3][1] << 16 | (uint32_t)q[3][2] << 24;
    } else {
#pragma unroll
      for (int j = 0; j < kTW; ++j)
        if (x0 + j < g.W) {
#pragma unroll
          for (int k = 0; k < 3; ++k) store_sample<KIND>(dst, o + 3 * j + k, q[j][k]);
        }
    }
  }
}

bool is_aligned(const void* p, uintptr_t al) { return ((uintptr_t)p & (al - 1)) == 0; }

// what the three entries share: the sample format, the subsampling and the extent -> the geometry and L
int check_common(const char* who, int32_t kind, int32_t depth, int32_t ss, int64_t n, int32_t T, int32_t H, int32_t W, Geo& g, double& L) {
  RCB_REQUIRE(kind == 0 || kind == 2, RCB_ERR_ARG, "%s: kind %d (0 = uint8, 2 = u16; fp32 and s16 samples have no Y'CbCr here)", who, kind);
  RCB_REQUIRE(kind == 2 ? (depth >= 9 && depth <= 16) : depth == 0, RCB_ERR_ARG, "%s: depth %d for kind %d (9 .. 16 for u16, 0 for uint8)",
              who, depth, kind);
  RCB_REQUIRE(ss >= 0 && ss <= 2, RCB_ERR_ARG, "%s: subsampling %d (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0)", who, ss);
  RCB_REQUIRE(n >= 0 && T >= 1, RCB_ERR_SHAPE, "%s: %lld signals of %d frames", who, (long long)n, T);
  RCB_REQUIRE(H >= 1 && W >= 1, RCB_ERR_SHAPE, "%s: frames of %d x %d positions (at least 1 x 1)", who, H, W);
  RCB_REQUIRE((long long)H * W <= kMaxPositions, RCB_ERR_UNSUPPORTED, "%s: frames of %d x %d positions (up to 2^26 per frame)", who, H, W);
  g.T = T, g.H = H, g.W = W, g.ss = ss;
  g.Hc = ss == 2 ? (H + 1) / 2 : H, g.Wc = ss ? (W + 1) / 2 : W;
  g.wgx = cdiv(cdiv(W, kTW), kWX), g.wgy = cdiv(cdiv(H, kTH), kWY);
  L = kind == 0 ? 255.0 : (double)((1 << depth) - 1);
  return RCB_OK;
}

int check_strides(const char* who, const char* what, const int64_t* st, int count) {
  RCB_REQUIRE(st, RCB_ERR_ARG, "%s: null strides of %s", who, what);
  for (int i = 0; i < count; ++i)
    RCB_REQUIRE(st[i] >= 0, RCB_ERR_ARG, "%s: a negative stride of %s (%lld at entry %d)", who, what, (long long)st[i], i);
  return RCB_OK;
}

// the farthest element read lies below `elems` (a stride that would overflow the product is caught by the division)
int check_reach(const char* who, const char* what, long long offset, const long long* dims, const int64_t* st, int count, int64_t elems) {
  long long reach = offset;
  bool fits = reach < elems;
  for (int i = 0; i < count && fits; ++i) {
    fits = dims[i] == 0 || st[i] <= (elems - 1 - reach) / dims[i];
    if (fits) reach += dims[i] * st[i];
  }
  RCB_REQUIRE(fits, RCB_ERR_SHAPE, "%s: %s reaches past its %lld elements", who, what, (long long)elems);
  return RCB_OK;
}

int check_blocks(const char* who, int64_t n, const Geo& g) {
  const long long per = (long long)g.wgx * g.wgy;
  RCB_REQUIRE(g.T <= 0x7fffffffLL / per && n <= 0x7fffffffLL / (per * g.T), RCB_ERR_UNSUPPORTED,
              "%s: %lld signals of %d frames of %lld workgroups need more than 2^31 - 1 workgroups", who, (long long)n, g.T, per);
  return RCB_OK;
}

int check_rgb(const char* who, const char* what, const void* p, int64_t elems, const int64_t* st, int64_t offset, int64_t n, const Geo& g,
              RgbSrc& s) {
  RCB_REQUIRE(p, RCB_ERR_ARG, "%s: null %s", who, what);
  const long long dims[5] = {n - 1, g.T - 1, g.H - 1, g.W - 1, 2};
  if (const int err = check_reach(who, what, offset, dims, st, 5, elems)) return err;
  s.p = p, s.off = offset;
  for (int i = 0; i < 5; ++i) s.st[i] = st[i];
  return RCB_OK;
}

// uint8 RGB rows as dwords: channel stride 1, column stride 3, the first sample and every signal, frame and row step on 4 bytes
bool rgb_rows_as_dwords(int32_t kind, const RgbSrc& s) {
  return kind == 0 && s.st[4] == 1 && s.st[3] == 3 && is_aligned(static_cast<const uint8_t*>(s.p) + s.off, 4) && s.st[0] % 4 == 0 &&
         s.st[1] % 4 == 0 && s.st[2] % 4 == 0;
}

void fill_consts(Consts& c, const double* m, const double* off, double L) {
  for (int i = 0; i < 9; ++i) c.m[i] = m[i];
  for (int i = 0; i < 3; ++i) c.off[i] = off[i];
  c.L = L;
}

}  // namespace

extern "C" int rcb_ycc_to_rgb(const void* py, const void* pcb, const void* pcr, const int64_t* elems, const int64_t* y_strides,
                              const int64_t* cb_strides, const int64_t* cr_strides, int32_t kind, int32_t depth, int32_t ss, int64_t n,
                              int32_t T, int32_t H, int32_t W, const double* inv, const double* o, void* dst, rcb_stream_t stream) {
  const char* who = "ycc_to_rgb";
  Geo g;
  double L;
  if (const int err = check_common(who, kind, depth, ss, n, T, H, W, g, L)) return err;
  if (const int err = check_strides(who, "the Y plane", y_strides, 4)) return err;
  if (const int err = check_strides(who, "the Cb plane", cb_strides, 4)) return err;
  if (const int err = check_strides(who, "the Cr plane", cr_strides, 4)) return err;
  RCB_REQUIRE(inv && o, RCB_ERR_ARG, "%s: null matrix or offsets", who);
  RCB_REQUIRE(elems, RCB_ERR_ARG, "%s: null element counts", who);
  if (n == 0) return RCB_OK;
  RCB_REQUIRE(py && pcb && pcr && dst, RCB_ERR_ARG, "%s: null py, pcb, pcr or dst", who);
  const long long dy[4] = {n - 1, T - 1, H - 1, W - 1}, dc[4] = {n - 1, T - 1, g.Hc - 1, g.Wc - 1};
  if (const int err = check_reach(who, "the Y plane", 0, dy, y_strides, 4, elems[0])) return err;
  if (const int err = check_reach(who, "the Cb plane", 0, dc, cb_strides, 4, elems[1])) return err;
  if (const int err = check_reach(who, "the Cr plane", 0, dc, cr_strides, 4, elems[2])) return err;
  if (const int err = check_blocks(who, n, g)) return err;

  Plane a, b, c;
  a.p = py, b.p = pcb, c.p = pcr;
  for (int i = 0; i < 4; ++i) a.st[i] = y_strides[i], b.st[i] = cb_strides[i], c.st[i] = cr_strides[i];
  Consts k;
  fill_consts(k, inv, o, L);
  const unsigned blocks = (unsigned)(n * T * g.wgx * g.wgy);
  hipStream_t st = (hipStream_t)stream;
  if (kind == 2) ycc_to_rgb_kernel<2, false><<<blocks, kThreads, 0, st>>>(a, b, c, k, g, dst);
  else if (W % 4 == 0 && is_aligned(dst, 4)) ycc_to_rgb_kernel<0, true><<<blocks, kThreads, 0, st>>>(a, b, c, k, g, dst);
  else ycc_to_rgb_kernel<0, false><<<blocks, kThreads, 0, st>>>(a, b, c, k, g, dst);
  RCB_LAUNCH_CHECK();
  return RCB_OK;
}

extern "C" int rcb_rgb_to_ycc(const void* src, int64_t src_elems, const int64_t* strides, int64_t offset, int32_t kind, int32_t depth,
                              int32_t ss, int64_t n, int32_t T, int32_t H, int32_t W, const double* m, const double* off, void* oy,
                              void* ocb, void* ocr, rcb_stream_t stream) {
  const char* who = "rgb_to_ycc";
  Geo g;
  double L;
  if (const int err = check_common(who, kind, depth, ss, n, T, H, W, g, L)) return err;
  if (const int err = check_strides(who, "src", strides, 5)) return err;
  RCB_REQUIRE(offset >= 0, RCB_ERR_ARG, "%s: a negative offset (%lld)", who, (long long)offset);
  RCB_REQUIRE(m && off, RCB_ERR_ARG, "%s: null matrix or offsets", who);
  RCB_REQUIRE(oy || ocb || ocr, RCB_ERR_ARG, "%s: oy, ocb and ocr are all null (at least one plane is wanted)", who);
  if (n == 0) return RCB_OK;
  RgbSrc s;
  if (const int err = check_rgb(who, "src", src, src_elems, strides, offset, n, g, s)) return err;
  if (const int err = check_blocks(who, n, g)) return err;

  Consts k;
  fill_consts(k, m, off, L);
  const unsigned blocks = (unsigned)(n * T * g.wgx * g.wgy);
  const int pack_y = kind == 0 && W % 4 == 0 && oy && is_aligned(oy, 4);
  hipStream_t st = (hipStream_t)stream;
  if (kind == 2) rgb_to_ycc_kernel<2, false><<<blocks, kThreads, 0, st>>>(s, k, g, oy, ocb, ocr, 0);
  else if (rgb_rows_as_dwords(kind, s)) rgb_to_ycc_kernel<0, true><<<blocks, kThreads, 0, st>>>(s, k, g, oy, ocb, ocr, pack_y);
  else rgb_to_ycc_kernel<0, false><<<blocks, kThreads, 0, st>>>(s, k, g, oy, ocb, ocr, pack_y);
  RCB_LAUNCH_CHECK();
  return RCB_OK;
}

extern "C" int rcb_ycc_sse(const void* a, int64_t a_elems, const int64_t* a_strides, int64_t a_offset, const void* b, int64_t b_elems,
                           const int64_t* b_strides, int64_t b_offset, int32_t kind, int32_t depth, int32_t ss, int64_t n, int32_t T,
                           int32_t H, int32_t W, const double* m, const double* off, int64_t* sse, rcb_stream_t stream) {
  const char* who = "ycc_sse";
  Geo g;
  double L;
  if (const int err = check_common(who, kind, depth, ss, n, T, H, W, g, L)) return err;
  if (const int err = check_strides(who, "a", a_strides, 5)) return err;
  if (const int err = check_strides(who, "b", b_strides, 5)) return err;
  RCB_REQUIRE(a_offset >= 0 && b_offset >= 0, RCB_ERR_ARG, "%s: a negative offset (%lld, %lld)", who, (long long)a_offset,
              (long long)b_offset);
  RCB_REQUIRE(m && off, RCB_ERR_ARG, "%s: null matrix or offsets", who);
  if (n == 0) return RCB_OK;
  RCB_REQUIRE(sse, RCB_ERR_ARG, "%s: null sse", who);
  RgbSrc sa, sb;
  if (const int err = check_rgb(who, "a", a, a_elems, a_strides, a_offset, n, g, sa)) return err;
  if (const int err = check_rgb(who, "b", b, b_elems, b_strides, b_offset, n, g, sb)) return err;
  if (const int err = check_blocks(who, n, g)) return err;

  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(sse, 0, (size_t)n * T * 3 * sizeof(int64_t), st);
  if (e != hipSuccess) return fail((int)e, "%s: clearing the sums failed: %s", who, hipGetErrorString(e));
  Consts k;
  fill_consts(k, m, off, L);
  const unsigned blocks = (unsigned)(n * T * g.wgx * g.wgy);
  if (kind == 2) ycc_sse_kernel<2, false><<<blocks, kThreads, 0, st>>>(sa, sb, k, g, (long long*)sse);
  else if (rgb_rows_as_dwords(kind, sa) && rgb_rows_as_dwords(kind, sb)) ycc_sse_kernel<0, true><<<blocks, kThreads, 0, st>>>(sa, sb, k, g, (long long*)sse);
  else ycc_sse_kernel<0, false><<<blocks, kThreads, 0, st>>>(sa, sb, k, g, (long long*)sse);
  RCB_LAUNCH_CHECK();
  return RCB_OK;
}
