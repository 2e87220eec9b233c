// N4 (416): resize image and video sources on the device -- the step the reference's video loader makes before anything else
// (data/video.py:26-31: the first 24 frames, centre-cropped to 240 x 240, resized to 128 x 128 by torchvision's antialiased bilinear
// Resize) and every codec comparison at a reduced resolution starts with.  The centre crop is a view (utils.center_crop); this file
// is the filter.
//
// rcb_resize reads n signals of T frames [H_in][W_in][C] of uint8, fp32 or 16-bit unsigned samples through element strides
// {signal, frame, row, column, channel} and an element offset -- rcb_signal_patch's addressing rule, 64-bit offsets -- and writes
// dst contiguous [n][T][H_out][W_out][C] of the source's type.
//
// The definition, fixed in include/rcb.h and restated by tests/resize_emul.py (every step one IEEE fp64 operation, contraction off):
//   taps     per axis, formed by the HOST (rcb_resize_taps) and uploaded: for output i the first input position, the number of taps
//            and the normalised triangle weights -- support max(scale, 1), half-pixel centres.  The device evaluates no weight.
//   filter   separable, the last spatial axis first, taps ascending, the first product starting the sum:
//              t(r, x) = ((w0 v(r, f) + w1 v(r, f+1)) + ...),   a(y, x) = ((u0 t(g, x) + u1 t(g+1, x)) + ...)
//            v the sample as an exact fp64 value, t never rounded below fp64
//   output   integers: (int)rint(fmin(fmax(a, 0), L)), ONE rounding, half to even; fp32: (float)a, no clamp
//
// Kernel.  One workgroup of 256 threads per tile of kTY x kTX = 8 x 32 output positions of one frame, looping over the channels.
// The input rows a tile needs, [first_y(y0), first_y(y1) + count_y(y1)) (both non-decreasing in y), are taken in consecutive chunks
// of kRows = 32: the row pass writes t [kRows][kTX] to LDS as fp64 (it never goes through HBM), the column pass adds the taps that
// fall into the chunk to the accumulator each thread carries in a register.  Chunks ascend and taps ascend inside a chunk, so the
// additions are the definition's, one by one, whatever the chunking: 16 : 1 on the row axis (7 * 16 + 32 = 144 rows) takes five chunks
// of the same 8 KiB.
// LDS.  t has a row pitch of kTX = 32 doubles = 256 bytes = all 64 banks.  A half-wave of the column pass is ONE output row (32
// consecutive x), so its 32 lanes read 32 consecutive doubles of ONE row of t: every bank twice over two dwords of one 8-byte read,
// conflict-free whichever row each output row's taps ask for (a [*][16] pitch, two output rows per half-wave, is conflict-free only
// when the two rows differ in parity, as SSIM's always do and a resize's do not).  The row pass writes the same 32 consecutive
// doubles per half-wave.  The x-tap rows of the tile are staged at a pitch of RCB_RESIZE_MAX_TAPS = 33 doubles: lane x reads dword
// 66 x + 2 j = 2 (x + j) mod 64, 32 distinct even banks.  The y-tap row is the same address for the whole half-wave: a broadcast.
// 8 KiB + 8.25 KiB + 2.06 KiB = 18.3 KiB per workgroup; no scratch.
#include <algorithm>
#include <vector>

#include "rcb_common.h"

#pragma clang fp contract(off)

using namespace rcb;

namespace {

constexpr int kThreads = 256;
constexpr int kTX = 32;                    // tile width: one half-wave per output row (tests/test_hip_resize.py states both)
constexpr int kTY = 8;                     // tile height
constexpr int kRows = 32;                  // input rows per LDS chunk
constexpr int kMaxTaps = RCB_RESIZE_MAX_TAPS;
constexpr int kMaxSide = 1 << 24;          // per axis, in and out: the tables stay small and every index an int

struct ResizeArgs {
  const void* src;
  void* dst;
  long long off, st[5];                    // elements: the first sample; signal, frame, row, column, channel
  int T, C, H_out, W_out, tiles_x, tiles_y;
  int ky, kx;                              // the pitch of wy and wx: the longest tap row of the axis
  const int* fy;                           // [H_out] first input row, cy [H_out] taps, wy [H_out][ky]
  const int* cy;
  const double* wy;
  const int* fx;                           // the same of the last axis
  const int* cx;
  const double* wx;
  double L;                                // integer kinds: the largest value
};

template <int KIND>
__device__ __forceinline__ double load_sample(const void* p, long long o) {
  if (KIND == 0) return (double)static_cast<const uint8_t*>(p)[o];
  if (KIND == 2) return (double)static_cast<const uint16_t*>(p)[o];
  return (double)static_cast<const float*>(p)[o];
}

template <int KIND>
__device__ __forceinline__ void store_sample(void* p, long long o, double a, double L) {
  if (KIND == 1) {
    static_cast<float*>(p)[o] = (float)a;
    return;
  }
  const int q = (int)rint(fmin(fmax(a, 0.0), L));
  if (KIND == 0) static_cast<uint8_t*>(p)[o] = (uint8_t)q;
  else static_cast<uint16_t*>(p)[o] = (uint16_t)q;
}

template <int KIND>
__global__ void __launch_bounds__(kThreads) resize_kernel(ResizeArgs a) {
  __shared__ double s_t[kRows][kTX];
  __shared__ double s_wx[kTX][kMaxTaps];
  __shared__ double s_wy[kTY][kMaxTaps];

  const int tid = threadIdx.x;
  long long blk = blockIdx.x;
  const int tx = (int)(blk % a.tiles_x);
  blk /= a.tiles_x;
  const int ty = (int)(blk % a.tiles_y);
  const long long frame = blk / a.tiles_y;                   // n * T + t
  const int x0 = tx * kTX, y0 = ty * kTY;
  const int px = tid % kTX, py = tid / kTX;
  const int ox = x0 + px, oy = y0 + py;
  const bool xin = ox < a.W_out, yin = oy < a.H_out;

  // the tap rows of the tile: uniform per output column (row pass) and per output row (column pass)
  for (int i = tid; i < kTX * a.kx; i += kThreads) {
    const int x = i / a.kx, j = i % a.kx;
    if (x0 + x < a.W_out) s_wx[x][j] = a.wx[(long long)(x0 + x) * a.kx + j];
  }
  for (int i = tid; i < kTY * a.ky; i += kThreads) {
    const int y = i / a.ky, j = i % a.ky;
    if (y0 + y < a.H_out) s_wy[y][j] = a.wy[(long long)(y0 + y) * a.ky + j];
  }
  const int fxx = xin ? a.fx[ox] : 0, cxx = xin ? a.cx[ox] : 0;
  const int fyy = yin ? a.fy[oy] : 0, cyy = yin ? a.cy[oy] : 0;
  const int y1 = min(y0 + kTY, a.H_out) - 1;
  const int rlo = a.fy[y0], rhi = a.fy[y1] + a.cy[y1];       // the input rows of the tile (first and first + count ascend with y)
  __syncthreads();

  const long long in0 = a.off + (frame / a.T) * a.st[0] + (frame % a.T) * a.st[1] + (long long)fxx * a.st[3];
  const long long out0 = ((frame * a.H_out + oy) * a.W_out + ox) * a.C;
  for (int c = 0; c < a.C; ++c) {
    double acc = 0.0;
    for (int base = rlo; base < rhi; base += kRows) {        // (uniform over the workgroup)
      // row pass: the last spatial axis first; thread (py, px) forms column px of rows py, py + 8, ... of the chunk
      if (xin) {
        for (int r = py; r < kRows && base + r < rhi; r += kTY) {
          const long long o = in0 + (long long)(base + r) * a.st[2] + c * a.st[4];
          double t = s_wx[px][0] * load_sample<KIND>(a.src, o);
          for (int j = 1; j < cxx; ++j) t = t + s_wx[px][j] * load_sample<KIND>(a.src, o + j * a.st[3]);
          s_t[r][px] = t;
        }
      }
      __syncthreads();
      // column pass: the taps of this output row that lie in the chunk, ascending; tap 0 starts the sum
      if (xin && yin) {
        const int jlo = max(0, base - fyy), jhi = min(cyy, base + kRows - fyy);
        for (int j = jlo; j < jhi; ++j) {
          const double p = s_wy[py][j] * s_t[fyy + j - base][px];
          acc = j == 0 ? p : acc + p;
        }
      }
      __syncthreads();                                       // (s_t is free for the next chunk, or the next channel)
    }
    if (xin && yin) store_sample<KIND>(a.dst, out0 + c, acc, a.L);
  }
}

bool is_aligned(const void* p, uintptr_t al) { return ((uintptr_t)p & (al - 1)) == 0; }

// one axis: the rule of the header -> the first position and the number of taps of output i
inline void tap_range(int n_in, double scale, double support, int i, int& first, int& count) {
  if (scale == 1.0) {                                        // n_in == n_out: the one tap of 1.0 (the formulas add a tap of weight 0)
    first = i, count = 1;
    return;
  }
  const double center = scale * ((double)i + 0.5);
  first = std::max((int)((center - support) + 0.5), 0);
  const int last = std::min((int)((center + support) + 0.5), n_in);
  count = last - first;
}

int check_axis(const char* who, int32_t n_in, int32_t n_out) {
  RCB_REQUIRE(n_in >= 1 && n_out >= 1, RCB_ERR_SHAPE, "%s: an axis of %d -> %d positions (at least 1 each)", who, n_in, n_out);
  RCB_REQUIRE(n_in <= kMaxSide && n_out <= kMaxSide, RCB_ERR_UNSUPPORTED, "%s: an axis of %d -> %d positions (up to 2^24 each)", who,
              n_in, n_out);
  RCB_REQUIRE(n_in <= 16ll * n_out, RCB_ERR_UNSUPPORTED, "%s: %d -> %d positions is more than 16 : 1 (%d taps at the most)", who, n_in,
              n_out, kMaxTaps);
  return RCB_OK;
}

// the longest tap row of an axis (check_axis holds)
int longest_count(int n_in, int n_out) {
  const double scale = (double)n_in / (double)n_out, support = scale >= 1.0 ? scale : 1.0;
  int longest = 0, first, count;
  for (int i = 0; i < n_out; ++i) {
    tap_range(n_in, scale, support, i, first, count);
    longest = std::max(longest, count);
  }
  return longest;
}

// device table: int32 fy [H_out], cy [H_out], fx [W_out], cx [W_out] (8 (H_out + W_out) bytes), then double wy [H_out][ky],
// wx [W_out][kx], ky / kx the longest tap row of the axis
long long table_bytes_of(int H_out, int W_out, int ky, int kx) {
  return 8ll * (H_out + W_out) + 8ll * ((long long)H_out * ky + (long long)W_out * kx);
}

}  // namespace

extern "C" int rcb_resize_taps(int32_t n_in, int32_t n_out, int32_t* first, int32_t* count, double* w, int32_t max_taps) {
  const char* who = "resize_taps";
  if (const int err = check_axis(who, n_in, n_out)) return err;
  RCB_REQUIRE(first && count && w, RCB_ERR_ARG, "%s: null first, count or w", who);
  const int longest = longest_count(n_in, n_out);
  RCB_REQUIRE(max_taps >= longest, RCB_ERR_SHAPE, "%s: rows of %d taps, %d -> %d needs %d", who, max_taps, n_in, n_out, longest);
  const double scale = (double)n_in / (double)n_out;
  const double support = scale >= 1.0 ? scale : 1.0, inv = scale >= 1.0 ? 1.0 / scale : 1.0;
  for (int i = 0; i < n_out; ++i) {
    int f, n;
    tap_range(n_in, scale, support, i, f, n);
    const double center = scale * ((double)i + 0.5);
    double* row = w + (long long)i * max_taps;
    double total = 0.0;
    for (int j = 0; j < n; ++j) {
      const double g = std::max(0.0, 1.0 - std::fabs((((double)(f + j) - center) + 0.5) * inv));
      row[j] = g;
      total = j == 0 ? g : total + g;
    }
    for (int j = 0; j < n; ++j) row[j] = row[j] / total;
    for (int j = n; j < max_taps; ++j) row[j] = 0.0;
    first[i] = f, count[i] = n;
  }
  return longest;
}

extern "C" int64_t rcb_resize_table_bytes(int32_t H_in, int32_t W_in, int32_t H_out, int32_t W_out) {
  if (check_axis("resize_table_bytes", H_in, H_out) || check_axis("resize_table_bytes", W_in, W_out)) return -1;
  return table_bytes_of(H_out, W_out, longest_count(H_in, H_out), longest_count(W_in, W_out));
}

extern "C" int rcb_resize(const void* src, int64_t src_elems, int32_t kind, int32_t depth, int64_t n, int32_t T, int32_t H_in,
                          int32_t W_in, int32_t C, const int64_t* strides, int64_t offset, int32_t H_out, int32_t W_out, void* dst,
                          void* table, int64_t table_bytes, rcb_stream_t stream) {
  const char* who = "resize";
  RCB_REQUIRE(kind == 0 || kind == 1 || kind == 2, RCB_ERR_ARG,
              "%s: kind %d (0 = uint8, 1 = fp32, 2 = u16; s16 audio is a different filter question)", who, kind);
  RCB_REQUIRE(kind == 2 ? (depth >= 9 && depth <= 16) : depth == 0, RCB_ERR_ARG, "%s: depth %d for kind %d (9 .. 16 for u16, 0 for the others)",
              who, depth, kind);
  RCB_REQUIRE(C >= 1 && C <= 32, RCB_ERR_SHAPE, "%s: %d channels (1 .. 32)", who, C);
  RCB_REQUIRE(n >= 0 && T >= 1, RCB_ERR_SHAPE, "%s: %lld signals of %d frames", who, (long long)n, T);
  if (const int err = check_axis(who, H_in, H_out)) return err;
  if (const int err = check_axis(who, W_in, W_out)) return err;
  RCB_REQUIRE(strides, RCB_ERR_ARG, "%s: null strides", who);
  for (int i = 0; i < 5; ++i)
    RCB_REQUIRE(strides[i] >= 0, RCB_ERR_ARG, "%s: a negative stride (%lld at entry %d)", who, (long long)strides[i], i);
  RCB_REQUIRE(offset >= 0, RCB_ERR_ARG, "%s: a negative offset (%lld)", who, (long long)offset);
  if (n == 0) return RCB_OK;
  RCB_REQUIRE(src && dst && table, RCB_ERR_ARG, "%s: null src, dst or table", who);
  const int ky = longest_count(H_in, H_out), kx = longest_count(W_in, W_out);
  const long long need = table_bytes_of(H_out, W_out, ky, kx);
  RCB_REQUIRE(table_bytes >= need && is_aligned(table, 8), RCB_ERR_SHAPE, "%s: table of %lld bytes (8-byte aligned), %lld needed", who,
              (long long)table_bytes, need);
  // the farthest element read lies below src_elems (a stride that would overflow the product is caught by the division)
  {
    const long long dims[5] = {n - 1, T - 1, H_in - 1, W_in - 1, C - 1};
    long long reach = offset;
    bool fits = reach < src_elems;
    for (int i = 0; i < 5 && fits; ++i) {
      fits = dims[i] == 0 || strides[i] <= (src_elems - 1 - reach) / dims[i];
      if (fits) reach += dims[i] * strides[i];
    }
    RCB_REQUIRE(fits, RCB_ERR_SHAPE, "%s: the signals reach past the %lld elements of the source", who, (long long)src_elems);
  }
  const int tiles_y = cdiv(H_out, kTY), tiles_x = cdiv(W_out, kTX);
  const long long tiles = (long long)tiles_y * tiles_x;
  RCB_REQUIRE(T <= 0x7fffffffLL / tiles && n <= 0x7fffffffLL / (tiles * T), RCB_ERR_UNSUPPORTED,
              "%s: %lld signals of %d frames of %lld tiles need more than 2^31 - 1 workgroups", who, (long long)n, T, tiles);

  // both tap tables through the planner, packed to the pitch of each axis
  std::vector<int64_t> host((size_t)need / 8);
  int* ints = reinterpret_cast<int*>(host.data());
  double* wy = reinterpret_cast<double*>(host.data()) + (H_out + W_out);
  double* wx = wy + (long long)H_out * ky;
  {
    std::vector<double> w((size_t)std::max(H_out, W_out) * kMaxTaps);
    int got = rcb_resize_taps(H_in, H_out, ints, ints + H_out, w.data(), kMaxTaps);
    if (got < 0) return got;
    for (int i = 0; i < H_out; ++i) std::copy_n(w.data() + (long long)i * kMaxTaps, ky, wy + (long long)i * ky);
    got = rcb_resize_taps(W_in, W_out, ints + 2 * H_out, ints + 2 * H_out + W_out, w.data(), kMaxTaps);
    if (got < 0) return got;
    for (int i = 0; i < W_out; ++i) std::copy_n(w.data() + (long long)i * kMaxTaps, kx, wx + (long long)i * kx);
  }
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(table, host.data(), (size_t)need, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail((int)e, "%s: table upload failed: %s", who, hipGetErrorString(e));

  ResizeArgs a;
  a.src = src, a.dst = dst;
  a.off = offset;
  for (int i = 0; i < 5; ++i) a.st[i] = strides[i];
  a.T = T, a.C = C, a.H_out = H_out, a.W_out = W_out;
  a.tiles_x = tiles_x, a.tiles_y = tiles_y;
  a.ky = ky, a.kx = kx;
  const int* d_ints = static_cast<const int*>(table);
  a.fy = d_ints, a.cy = d_ints + H_out, a.fx = d_ints + 2 * H_out, a.cx = d_ints + 2 * H_out + W_out;
  a.wy = static_cast<const double*>(table) + (H_out + W_out);
  a.wx = a.wy + (long long)H_out * ky;
  a.L = kind == 0 ? 255.0 : kind == 2 ? (double)((1 << depth) - 1) : 0.0;
  const unsigned blocks = (unsigned)(n * T * tiles);
  if (kind == 0) resize_kernel<0><<<blocks, kThreads, 0, st>>>(a);
  else if (kind == 1) resize_kernel<1><<<blocks, kThreads, 0, st>>>(a);
  else resize_kernel<2><<<blocks, kThreads, 0, st>>>(a);
  RCB_LAUNCH_CHECK();
  return RCB_OK;
}
