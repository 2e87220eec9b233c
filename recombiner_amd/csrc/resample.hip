// N4 (419): resample PCM audio to the preset's rate on the device -- the audio preset is a 16 kHz preset (data/audio.py:39-46
// hard-codes LibriSpeech's rate; 48 000 samples are "3 s at 16 kHz"), audio elsewhere is 44.1 or 48 kHz and often stereo.
//
// rcb_resample reads n_sig signals of L_in samples and C channels of int16 PCM or fp32 through element strides {signal, sample,
// channel} and an element offset -- rcb_resize's addressing rule -- and writes dst contiguous [n_sig][length_out][C_out] of the
// source's type, C_out = C, or 1 with a channel mix.
//
// The definition, fixed in include/rcb.h and restated by tests/resample_emul.py (every step one IEEE fp64 operation, contraction off):
//   taps     the polyphase Hann-windowed sinc of torchaudio.functional.resample at its defaults, formed by the HOST
//            (rcb_resample_taps) and uploaded: per phase p = i mod n the first offset, the number of taps and the weights.  The
//            device evaluates no weight.
//   filter   output i = q n + p:  a = ((w_0 v(m_0) + w_1 v(m_0 + 1)) + ...), m_0 = q o + first[p], taps ascending, the first product
//            starting the sum; v(m) = +0.0 outside [0, L_in), multiplied and added like any other sample
//   mix      v(m) = ((g_0 x_0(m) + g_1 x_1(m)) + ...) in fp64 before the filter
//   output   a' = a * gain + bias unless gain == 1 and bias == 0;  s16: (int)rint(fmin(fmax(a', -32768), 32767));  fp32: (float)a'
//
// Kernel.  One workgroup of 256 threads per tile of kTile = 256 consecutive outputs of one signal, looping over the output channels.
// m_0(i) and m_0(i) + count(i) do not decrease with i (the host proves it for the table it uploads), so the input span of a tile is
// [m_0(first output), m_0(last output) + count(last output)): at most ceil(256 o / n) + 97 samples, which the host also proves
// against kSpan before it launches.  The span is staged ONCE into LDS as fp64 after the channel mix -- the mix and the integer ->
// double conversion happen once per sample, not once per tap -- and each thread then runs its phase's taps ascending.
// Tap table.  Consecutive lanes are consecutive outputs, hence consecutive phases mod n: the device table is w [tap][phase], so
// that tap j of a wave is one run of 64 consecutive doubles (two when the phase wraps) -- 512 bytes, four full 128-byte lines.
// [phase][tap] would put the lanes K doubles apart: one line per lane and tap.  With n = 1 (3 : 1, 8 : 1) all lanes read one address.
// LDS.  ds_read_b64 is served per 32-lane half over 64 dword banks: lanes d doubles apart hit dword banks 2 d l mod 64, which are
// distinct for 32 lanes exactly when d is odd.  3 : 1 (d = 3) is conflict-free; 2 : 1, 4 : 1, 6 : 1 and 8 : 1 are 2-, 4-, 2- and
// 8-way, and 8 : 1, the legal worst case, would pay eight LDS cycles per read where the two fp64 operations of a tap take about as
// long as one.  For the even whole ratios d = 2^a m (m odd) the span is therefore stored at idx + (idx >> a): lane l's sample
// d l + c moves to (d + m) l + c + (c >> a), a lane distance of m (2^a + 1) doubles, which is odd -- conflict-free for 2, 4, 6
// and 8 : 1 at the cost of one shift and one add per tap and of span >> a more doubles of LDS.  Other ratios keep the plain index
// (a shift by 31): a fractional ratio such as 441 : 160 mixes lane distances of 2 and 3 doubles and is 2-way on nearly every read,
// which no fixed padding mends.  tools/resample_lds_banks.py counts all of this by the bank rule; its table is in
// profiles/r25_resample_resources.txt.
// kSpanLds * 8 = 20 KiB per workgroup; no scratch.
#include <algorithm>
#include <cmath>
#include <vector>

#include "rcb_common.h"

#pragma clang fp contract(off)

using namespace rcb;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 256;                 // outputs per workgroup (tests/test_hip_resample.py states it)
constexpr int kMaxTaps = RCB_RESAMPLE_MAX_TAPS;
constexpr int kSpan = 2176;                // samples a tile may need: ceil(256 * 8) + 97, rounded up to a multiple of 64
constexpr int kSpanLds = 2560;             // the padded span: 2176 * 9 / 8 at 8 : 1, (6 * 256 + 100) * 3 / 2 at 6 : 1
constexpr int kMaxC = 8;
constexpr int kMaxN = 1024, kMaxO = 8192;
constexpr double kPi = 3.14159265358979323846;

struct ResampleArgs {
  const void* src;
  void* dst;
  long long off, st[3];                    // elements: the first sample; signal, sample, channel
  int L_in, C, C_out, length_out, tiles;
  int o, n;
  int pad_shift;                           // a: the span at idx + (idx >> a); 31: at idx
  int has_mix, affine;
  const int* first;                        // [n] first offset of the phase, count [n] taps, w [K][n]
  const int* count;
  const double* w;
  double mix[kMaxC];
  double gain, bias;
};

template <int KIND>
__device__ __forceinline__ double load_sample(const void* p, long long o) {
  if (KIND == 3) return (double)static_cast<const int16_t*>(p)[o];
  return (double)static_cast<const float*>(p)[o];
}

template <int KIND>
__device__ __forceinline__ void store_sample(void* p, long long o, double a) {
  if (KIND == 1) {
    static_cast<float*>(p)[o] = (float)a;
    return;
  }
  static_cast<int16_t*>(p)[o] = (int16_t)(int)rint(fmin(fmax(a, -32768.0), 32767.0));
}

template <int KIND>
__global__ void __launch_bounds__(kThreads) resample_kernel(ResampleArgs a) {
  __shared__ double s_v[kSpanLds];

  const int tid = threadIdx.x;
  const long long blk = blockIdx.x;
  const int tile = (int)(blk % a.tiles);
  const long long sig = blk / a.tiles;
  const int i_lo = tile * kTile, i_hi = min(i_lo + kTile, a.length_out) - 1;   // the outputs of the tile, inclusive
  const int i = i_lo + tid;
  const bool live = i <= i_hi;

  // the span of the tile: from the first tap of its first output to the last tap of its last (both ascend with i)
  const long long lo = (long long)(i_lo / a.n) * a.o + a.first[i_lo % a.n];
  const int p_hi = i_hi % a.n;
  const int span = (int)((long long)(i_hi / a.n) * a.o + a.first[p_hi] + a.count[p_hi] - lo);
  const int p = live ? i % a.n : 0;
  const int cnt = live ? a.count[p] : 0;
  const int r0 = live ? (int)((long long)(i / a.n) * a.o + a.first[p] - lo) : 0;          // in [0, span - cnt]
  const int sh = a.pad_shift;

  const long long in0 = a.off + sig * a.st[0];
  const long long out0 = (sig * a.length_out + i) * a.C_out;
  for (int c = 0; c < a.C_out; ++c) {
    // stage: the channel (or the mix of the channels) of every sample of the span, once, as fp64; +0.0 outside the signal
    for (int idx = tid; idx < span; idx += kThreads) {
      const long long m = lo + idx;
      double v = 0.0;
      if (m >= 0 && m < a.L_in) {
        const long long at = in0 + m * a.st[1];
        if (a.has_mix) {
          v = a.mix[0] * load_sample<KIND>(a.src, at);
#pragma unroll
          for (int k = 1; k < kMaxC; ++k)
            if (k < a.C) v = v + a.mix[k] * load_sample<KIND>(a.src, at + k * a.st[2]);
        } else {
          v = load_sample<KIND>(a.src, at + c * a.st[2]);
        }
      }
      s_v[idx + (idx >> sh)] = v;
    }
    __syncthreads();
    if (live) {
      double acc = a.w[p] * s_v[r0 + (r0 >> sh)];
      for (int j = 1; j < cnt; ++j) {
        const int r = r0 + j;
        acc = acc + a.w[(long long)j * a.n + p] * s_v[r + (r >> sh)];
      }
      if (a.affine) acc = acc * a.gain + a.bias;
      store_sample<KIND>(a.dst, out0 + c, acc);
    }
    __syncthreads();                                         // (s_v is free for the next channel)
  }
}

bool is_aligned(const void* p, uintptr_t al) { return ((uintptr_t)p & (al - 1)) == 0; }

int gcd_of(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b, b = t;
  }
  return a;
}

// the rule of the header: rates -> o, n, or a refusal
int check_rates(const char* who, int32_t rate_in, int32_t rate_out, int& o, int& n) {
  RCB_REQUIRE(rate_in >= 1 && rate_out >= 1, RCB_ERR_SHAPE, "%s: rates of %d -> %d (at least 1 each)", who, rate_in, rate_out);
  const int g = gcd_of(rate_in, rate_out);
  o = rate_in / g, n = rate_out / g;
  if (o == n) return RCB_OK;
  RCB_REQUIRE(o <= 8ll * n, RCB_ERR_UNSUPPORTED, "%s: %d -> %d is %d : %d, more than 8 : 1 (%d taps at the most)", who, rate_in, rate_out,
              o, n, kMaxTaps);
  RCB_REQUIRE(n <= kMaxN && o <= kMaxO, RCB_ERR_UNSUPPORTED, "%s: %d -> %d is %d : %d in lowest terms (up to %d : %d)", who, rate_in,
              rate_out, o, n, kMaxO, kMaxN);
  return RCB_OK;
}

struct Filter {
  int o, n, width;
  double base, s;
  Filter(int o_, int n_) : o(o_), n(n_) {
    base = (double)std::min(o, n) * 0.99;
    width = (int)std::ceil(6.0 * (double)o / base);
    s = base / (double)o;
  }
  double t_of(int p, int k) const { return (-(double)p / (double)n + (double)k / (double)o) * base; }
  // phase p -> the first kept offset and the number of kept offsets; the weights to row (when not null)
  void phase(int p, int& first, int& count, double* row) const {
    if (o == n) {
      first = 0, count = 1;
      if (row) row[0] = 1.0;
      return;
    }
    first = 0, count = 0;
    for (int k = -width; k < width + o; ++k) {
      const double t = t_of(p, k);
      if (!(std::fabs(t) < 6.0)) continue;
      if (count == 0) first = k;
      if (row && count < kMaxTaps) {
        const double c = std::cos(((t * kPi) / 6.0) / 2.0);
        const double tp = t * kPi;
        row[count] = ((tp == 0.0 ? 1.0 : std::sin(tp) / tp) * (c * c)) * s;
      }
      ++count;
    }
  }
};

int longest_count(const Filter& f) {
  int longest = 0, first, count;
  for (int p = 0; p < f.n; ++p) {
    f.phase(p, first, count, nullptr);
    longest = std::max(longest, count);
  }
  return longest;
}

long long length_of(long long L_in, int o, int n) { return (n * L_in + o - 1) / o; }

// device table: int32 first [n], count [n] (8 n bytes), then double w [K][n], K the longest tap row
long long table_bytes_of(int n, int K) { return 8ll * n + 8ll * (long long)K * n; }

}  // namespace

extern "C" int rcb_resample_taps(int32_t rate_in, int32_t rate_out, int32_t* o_out, int32_t* n_out, int32_t* first, int32_t* count,
                                 double* w, int32_t max_taps) {
  const char* who = "resample_taps";
  int o, n;
  if (const int err = check_rates(who, rate_in, rate_out, o, n)) return err;
  RCB_REQUIRE(o_out && n_out, RCB_ERR_ARG, "%s: null o or n", who);
  const bool query = !first && !count && !w;
  RCB_REQUIRE(query || (first && count && w), RCB_ERR_ARG, "%s: first, count and w are given together, or none of them", who);
  const Filter f(o, n);
  const int longest = longest_count(f);
  RCB_REQUIRE(longest <= kMaxTaps, RCB_ERR_UNSUPPORTED, "%s: rows of %d taps (%d at the most)", who, longest, kMaxTaps);
  RCB_REQUIRE(query || max_taps >= longest, RCB_ERR_SHAPE, "%s: rows of %d taps, %d -> %d needs %d", who, max_taps, rate_in, rate_out,
              longest);
  *o_out = o, *n_out = n;
  if (query) return longest;
  std::vector<double> row(kMaxTaps);
  for (int p = 0; p < n; ++p) {
    int fi, cn;
    f.phase(p, fi, cn, row.data());
    double* out = w + (long long)p * max_taps;
    for (int j = 0; j < max_taps; ++j) out[j] = j < cn ? row[j] : 0.0;
    first[p] = fi, count[p] = cn;
  }
  return longest;
}

extern "C" int64_t rcb_resample_length(int64_t L_in, int32_t rate_in, int32_t rate_out) {
  int o, n;
  if (check_rates("resample_length", rate_in, rate_out, o, n)) return -1;
  if (L_in < 1 || L_in > 0x7fffffffLL) {
    fail(RCB_ERR_SHAPE, "resample_length: %lld samples (1 .. 2^31 - 1)", (long long)L_in);
    return -1;
  }
  return length_of(L_in, o, n);
}

extern "C" int64_t rcb_resample_table_bytes(int32_t rate_in, int32_t rate_out) {
  int o, n;
  if (check_rates("resample_table_bytes", rate_in, rate_out, o, n)) return -1;
  return table_bytes_of(n, longest_count(Filter(o, n)));
}

extern "C" int rcb_resample(const void* src, int64_t src_elems, int32_t kind, int64_t n_sig, int32_t L_in, int32_t C,
                            const int64_t* strides, int64_t offset, int32_t rate_in, int32_t rate_out, const double* mix, double gain,
                            double bias, int32_t length_out, void* dst, void* table, int64_t table_bytes, rcb_stream_t stream) {
  const char* who = "resample";
  RCB_REQUIRE(kind == 1 || kind == 3, RCB_ERR_ARG, "%s: kind %d (1 = fp32, 3 = s16; images are rcb_resize's)", who, kind);
  RCB_REQUIRE(C >= 1 && C <= kMaxC, RCB_ERR_SHAPE, "%s: %d channels (1 .. %d)", who, C, kMaxC);
  RCB_REQUIRE(n_sig >= 0 && L_in >= 1, RCB_ERR_SHAPE, "%s: %lld signals of %d samples", who, (long long)n_sig, L_in);
  int o, n;
  if (const int err = check_rates(who, rate_in, rate_out, o, n)) return err;
  const long long L_out = length_of(L_in, o, n);
  RCB_REQUIRE(L_out <= 0x7fffffffLL, RCB_ERR_UNSUPPORTED, "%s: %d samples at %d : %d are %lld outputs (up to 2^31 - 1)", who, L_in, o, n,
              L_out);
  RCB_REQUIRE(length_out >= 1 && length_out <= L_out, RCB_ERR_SHAPE, "%s: %d outputs asked of %lld", who, length_out, L_out);
  RCB_REQUIRE(strides, RCB_ERR_ARG, "%s: null strides", who);
  for (int i = 0; i < 3; ++i)
    RCB_REQUIRE(strides[i] >= 0, RCB_ERR_ARG, "%s: a negative stride (%lld at entry %d)", who, (long long)strides[i], i);
  RCB_REQUIRE(offset >= 0, RCB_ERR_ARG, "%s: a negative offset (%lld)", who, (long long)offset);
  if (n_sig == 0) return RCB_OK;
  RCB_REQUIRE(src && dst && table, RCB_ERR_ARG, "%s: null src, dst or table", who);
  const Filter f(o, n);
  const int K = longest_count(f);
  RCB_REQUIRE(K <= kMaxTaps, RCB_ERR_UNSUPPORTED, "%s: rows of %d taps (%d at the most)", who, K, kMaxTaps);
  const long long need = table_bytes_of(n, K);
  RCB_REQUIRE(table_bytes >= need && is_aligned(table, 8), RCB_ERR_SHAPE, "%s: table of %lld bytes (8-byte aligned), %lld needed", who,
              (long long)table_bytes, need);
  // the farthest element read lies below src_elems (a stride that would overflow the product is caught by the division)
  {
    const long long dims[3] = {n_sig - 1, L_in - 1, C - 1};
    long long reach = offset;
    bool fits = reach < src_elems;
    for (int i = 0; i < 3 && fits; ++i) {
      fits = dims[i] == 0 || strides[i] <= (src_elems - 1 - reach) / dims[i];
      if (fits) reach += dims[i] * strides[i];
    }
    RCB_REQUIRE(fits, RCB_ERR_SHAPE, "%s: the signals reach past the %lld elements of the source", who, (long long)src_elems);
  }
  const int tiles = cdiv(length_out, kTile);
  RCB_REQUIRE(n_sig <= 0x7fffffffLL / tiles, RCB_ERR_UNSUPPORTED, "%s: %lld signals of %d tiles need more than 2^31 - 1 workgroups", who,
              (long long)n_sig, tiles);

  // the table: first and count per phase, the weights transposed to [tap][phase]
  std::vector<int64_t> host((size_t)need / 8);
  int* first = reinterpret_cast<int*>(host.data());
  int* count = first + n;
  double* w = reinterpret_cast<double*>(host.data()) + n;
  {
    std::vector<double> row(kMaxTaps);
    for (int p = 0; p < n; ++p) {
      f.phase(p, first[p], count[p], row.data());
      for (int j = 0; j < K; ++j) w[(long long)j * n + p] = j < count[p] ? row[j] : 0.0;
    }
  }
  // what the kernel relies on, proven for this table: the first and the end of the taps ascend with the output index (over the
  // wrap of the phase as well), and no tile of kTile outputs, wherever its first phase lies, spans more than kSpan samples
  int pad_shift = 31;
  {
    bool ascending = true;
    for (int p = 0; p < n && ascending; ++p) {
      const int nx = (p + 1) % n, step = p + 1 == n ? o : 0;
      ascending = count[p] >= 1 && first[nx] + step >= first[p] && first[nx] + count[nx] + step >= first[p] + count[p];
    }
    RCB_REQUIRE(ascending, RCB_ERR_UNSUPPORTED, "%s: the taps of %d : %d do not ascend with the output", who, o, n);
    long long widest = 0;
    for (int p = 0; p < n; ++p) {
      const long long e = p + kTile - 1;
      widest = std::max(widest, (e / n) * o + first[e % n] + count[e % n] - first[p]);
    }
    RCB_REQUIRE(widest <= kSpan, RCB_ERR_UNSUPPORTED, "%s: a tile of %d : %d spans %lld samples (%d at the most)", who, o, n, widest,
                kSpan);
    // an even whole ratio 2^a m: the padded index idx + (idx >> a) -- when the padded span fits, which it does up to 8 : 1
    if (o != n && o % (2 * n) == 0) {
      int d = o / n, sh = 0;
      while (!(d & 1)) d >>= 1, ++sh;
      if (widest + (widest >> sh) <= kSpanLds) pad_shift = sh;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(table, host.data(), (size_t)need, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail((int)e, "%s: table upload failed: %s", who, hipGetErrorString(e));

  ResampleArgs a;
  a.src = src, a.dst = dst;
  a.off = offset;
  for (int i = 0; i < 3; ++i) a.st[i] = strides[i];
  a.L_in = L_in, a.C = C, a.C_out = mix ? 1 : C, a.length_out = length_out, a.tiles = tiles;
  a.o = o, a.n = n;
  a.pad_shift = pad_shift;
  a.has_mix = mix ? 1 : 0;
  for (int c = 0; c < kMaxC; ++c) a.mix[c] = mix && c < C ? mix[c] : 0.0;
  a.gain = gain, a.bias = bias;
  a.affine = !(gain == 1.0 && bias == 0.0);
  a.first = static_cast<const int*>(table), a.count = a.first + n;
  a.w = static_cast<const double*>(table) + n;
  const unsigned blocks = (unsigned)(n_sig * tiles);
  if (kind == 1) resample_kernel<1><<<blocks, kThreads, 0, st>>>(a);
  else resample_kernel<3><<<blocks, kThreads, 0, st>>>(a);
  RCB_LAUNCH_CHECK();
  return RCB_OK;
}
