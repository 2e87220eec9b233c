// Stand-alone sweep of recombiner_amd/csrc/siren_route.h (host compiler, no HIP): every descriptor of the lattice of
// tools/siren_desc_digests.py that siren_check_desc accepts, crossed with mode, has_dpe, in16_rows, wave_variant and the
// (n_rows, n_cu) pairs that straddle the wave family's fill rule, then a few descriptors beyond the lattice (extras()), one line
// per case on stdout and "# ..." count lines.  `sweep extras` prints the extras alone: the form a -DRCB_SIREN_DEALT32 build runs.
// Exit status 1 with a message on stderr when
//   - a case gets neither exactly one family nor exactly one refusal,
//   - a named instance is not in its family's list,
//   - siren_layers differs from the closed form at uniform widths,
//   - a descriptor reaches the one-wave-per-row or the plain-FMA family that the two requirements those families' dispatchers
//     once began with would have refused (the evidence that they could never fire).
// tests/test_siren_route_cpu.py builds this with -fsanitize=address,undefined and holds the output to tests/golden/siren_routes.json.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "../recombiner_amd/csrc/siren_route.h"

static char g_text[512];
static rcb::SirenLayers g_layers;
int rcb::fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_text, sizeof(g_text), fmt, ap);
  va_end(ap);
  return code;
}

using namespace rcb;

static const int PRECISIONS[] = {-1, 0, 1, 2, 3};
static const int HIDDEN[] = {0, 1, 8, 16, 17, 24, 32, 33, 48, 64, 65};
static const char* const WIDTH_LISTS[] = {"none", "uniform", "mixed"};
static const int MIXED[4] = {24, 40, 8, 16};
static const int FEC[][3] = {{16, 16, 3}, {16, 16, 1}, {18, 16, 3}, {16, 0, 3}, {32, 32, 32}, {34, 32, 3}, {16, 16, 33}, {15, 16, 3}, {16, 12, 3}};
static const int N_PIX[] = {32, 33};
static const int ROWS_CU[][2] = {{4, 256}, {2048, 256}, {2500, 256}};
static const char* const FAMILY[] = {"refused", "fp32", "generic", "workgroup", "wave", "wide", "rowwave"};

static void die(const char* label, const char* what) {
  fprintf(stderr, "siren_route_sweep: %s: %s\n", label, what);
  exit(1);
}

static bool listed(const SirenRoute& r) {
  const int* p = r.p;
  bool in = false;
  switch (r.family) {
#define X3(a, b, c) in = in || (p[0] == a && p[1] == b && p[2] == c);
#define X4(a, b, c, e) in = in || (p[0] == a && p[1] == b && p[2] == c && p[3] == e);
#define X5(a, b, c, e, f) in = in || (p[0] == a && p[1] == b && p[2] == c && p[3] == e && p[4] == f);
    case SIREN_FP32: RCB_SIREN_FP32_INSTANCES(X3) break;
    case SIREN_WG: RCB_SIREN_WG_INSTANCES(X4) break;
    case SIREN_WAVE: RCB_SIREN_WAVE_INSTANCES(X4) break;
    case SIREN_WIDE: RCB_SIREN_WIDE_INSTANCES(X5) break;
    case SIREN_ROWWAVE: RCB_SIREN_ROWWAVE_INSTANCES(X3) break;
    case SIREN_GENERIC: in = p[0] == MAXL || p[0] == SIREN_MAX_LAYERS; break;
#undef X3
#undef X4
#undef X5
  }
  return in;
}

static void check_layers(const char* label, const rcb_siren_desc& d) {
  const SirenLayers L = siren_layers(&d);
  const long long in0 = d.fourier_dim + d.pe_dim, hw = d.hidden, nh = d.n_hidden, C = d.out_dim;
  if (L.nl != nh + 1 || L.dnet != hw * (in0 + 1) + (nh - 1) * hw * (hw + 1) + C * (hw + 1) ||
      L.wt != hw * in0 + (nh - 1) * hw * hw + C * hw)
    die(label, "siren_layers: dnet / wt differ from the closed form");
  for (int l = 0; l <= nh; ++l)
    if (L.in[l] != (l == 0 ? in0 : hw) || L.out[l] != (l == nh ? C : hw) ||
        L.off[l] != (l == 0 ? 0 : hw * (in0 + 1) + (l - 1) * hw * (hw + 1)))
      die(label, "siren_layers: a layer differs from the closed form");
}

static long long n_desc = 0, n_accepted = 0, n_cases = 0, by_family[7] = {0}, by_pm[3][3] = {{0}};

// the two requirements that left the dispatchers, then one line per case
static void route_cases(const char* label, rcb_siren_desc& d, bool every_switch) {
  const int prec = d.precision, hid = d.hidden, nh = d.n_hidden;
  const bool rowwave = prec >= 1 && (nh >= 5 || ((hid == 16 || hid == 24) && d.hidden_dims[0] == 0));
  const bool generic = prec == 0 && (hid != HID || d.hidden_dims[0] != 0 || nh > 4);
  if (rowwave && !(nh >= 1 && nh <= 7 && (hid == 16 || hid == 24 || (hid == 32 && nh >= 5)) && d.hidden_dims[0] == 0))
    die(label, "reaches the one-wave-per-row family outside 1..4 layers of width 16 / 24, 5..7 of 16 / 24 / 32");
  if (generic && !(d.precision == 0 && hid >= 1 && hid <= SIREN_MAX_WIDTH && nh + 1 <= SIREN_MAX_LAYERS && d.out_dim <= 32 &&
                   d.pixel_chunks <= 1))
    die(label, "reaches the plain-FMA family outside fp32, width 1..64, 8 linear layers, out_dim <= 32, one chunk");
  char line[512];
  for (int mode = 0; mode <= 2; ++mode)
    for (int dpe = every_switch ? 0 : 1; dpe <= 1; ++dpe)
      for (int in16 = every_switch ? 0 : 1; in16 <= 1; ++in16)
        for (int wv = every_switch ? 0 : 1; wv <= (every_switch ? 2 : 1); ++wv)
          for (const auto& rc : ROWS_CU)
            for (int dealt = 0; dealt <= (every_switch ? 0 : 1); ++dealt) {
              d.n_rows = rc[0];
              if (siren_check_desc(&d, g_layers) != RCB_OK) die(label, "the number of rows changes what the check accepts");
              const SirenRoute r = siren_route(&d, mode, dpe, in16, wv, rc[1], dealt);
              const bool named = r.family > SIREN_REFUSED && r.family <= SIREN_ROWWAVE;
              if (r.family < SIREN_REFUSED || r.family > SIREN_ROWWAVE || named == (r.text[0] != 0) || (!named && r.code == RCB_OK))
                die(label, "neither exactly one family nor exactly one refusal");
              if (named && !listed(r)) die(label, "the named instance is not in its family's list");
              if ((r.family == SIREN_ROWWAVE) != (rowwave && named) || (r.family == SIREN_GENERIC) != (generic && named))
                die(label, "family and predicate disagree");
              if (r.family == SIREN_WAVE && !(mode != MODE_FWD && prec == 1 && hid == HID))
                die(label, "the wave family outside width-32 bf16 loss / backward (where the caller asks the device for n_cu)");
              int n = snprintf(line, sizeof(line), "%s | m%d dpe%d in16=%d wv%d rows%d cu%d", label, mode, dpe, in16, wv, rc[0], rc[1]);
              if (!every_switch) n += snprintf(line + n, sizeof(line) - n, " dealt32=%d", dealt);
              if (named)
                snprintf(line + n, sizeof(line) - n, " -> %s(%d,%d,%d,%d,%d) in16=%d dpe=%d", FAMILY[r.family], r.p[0], r.p[1], r.p[2],
                         r.p[3], r.p[4], (int)r.in16, (int)r.dpe);
              else
                snprintf(line + n, sizeof(line) - n, " -> refused %d %s", r.code, r.text);
              puts(line);
              ++n_cases, ++by_family[r.family], ++by_pm[prec][mode];
            }
}

static rcb_siren_desc base_desc() {
  rcb_siren_desc d;
  memset(&d, 0, sizeof(d));
  d.n_rows = 4, d.samples = 2, d.w_row_stride = d.dw_bf16_stride = 1 << 16, d.w0 = 30.f;
  return d;
}

// what the lattice does not reach: F or E above 32 on the one-wave-per-row path, clock_probe, and RCB_SIREN_W32_DEALT (which only
// a -DRCB_SIREN_DEALT32 build of this program looks at); mode x dealt32 x the three row counts, the other switches on
static void extras() {
  static uint64_t probe[4];
  struct { const char* name; int prec, hid, nh, F, E, C; bool probe; } X[] = {
      {"w16 F34", 1, 16, 3, 34, 16, 3, false},       {"w24 E34", 2, 24, 2, 16, 34, 3, false},  {"w32 nh6 F34", 1, 32, 6, 34, 16, 3, false},
      {"w16 clock_probe", 1, 16, 3, 16, 16, 3, true}, {"w32 nh5 clock_probe", 2, 32, 5, 16, 16, 3, true},
      {"w32 clock_probe", 1, 32, 3, 16, 16, 3, true}, {"w64 clock_probe", 1, 64, 3, 16, 16, 3, true},
      {"fp32 clock_probe", 0, 32, 3, 16, 16, 3, true}, {"w32 audio", 1, 32, 3, 16, 16, 1, false},
      {"w32 video f16", 2, 32, 3, 18, 16, 3, false},  {"w32 nh2", 1, 32, 2, 16, 16, 3, false},  {"w32 nh4", 1, 32, 4, 16, 16, 3, false},
      {"w48", 2, 48, 3, 16, 16, 3, false}};
  for (const auto& x : X) {
    rcb_siren_desc d = base_desc();
    d.precision = x.prec, d.hidden = x.hid, d.n_hidden = x.nh, d.fourier_dim = x.F, d.pe_dim = x.E, d.out_dim = x.C, d.n_pix = 64;
    d.pe_bf16 = x.prec > 0 && x.E % 8 == 0, d.clock_probe = x.probe ? probe : nullptr;
    char label[160];
    snprintf(label, sizeof(label), "extra %s p%d", x.name, x.prec);
    ++n_desc;
    if (siren_check_desc(&d, g_layers) != RCB_OK) die(label, "not accepted");
    ++n_accepted;
    route_cases(label, d, false);
  }
}

int main(int argc, char** argv) {
  const bool only_extras = argc > 1 && !strcmp(argv[1], "extras");
  char label[160];
  for (int prec : PRECISIONS)
    for (int hid : HIDDEN)
      for (int nh = 0; nh <= 8 && !only_extras; ++nh)
        for (int wl = 0; wl < 3; ++wl)
          for (const auto& fec : FEC)
            for (int P : N_PIX)
              for (int chunks = 0; chunks <= 3; ++chunks)
                for (int pe16 = 0; pe16 <= 1; ++pe16)
                  for (int dw16 = 0; dw16 <= 1; ++dw16) {
                    rcb_siren_desc d = base_desc();
                    d.precision = prec, d.hidden = hid, d.n_hidden = nh;
                    for (int i = 0; i < 4; ++i) d.hidden_dims[i] = wl == 0 ? 0 : wl == 1 ? hid : MIXED[i];
                    d.fourier_dim = fec[0], d.pe_dim = fec[1], d.out_dim = fec[2], d.n_pix = P;
                    d.pixel_chunks = chunks, d.pe_bf16 = pe16, d.dw_bf16 = dw16 ? (void*)g_text : nullptr;
                    ++n_desc;
                    if (siren_check_desc(&d, g_layers) != RCB_OK) continue;
                    ++n_accepted;
                    snprintf(label, sizeof(label), "p%d w%d nh%d %s F%d E%d C%d P%d ch%d pe16=%d dw16=%d", prec, hid, nh, WIDTH_LISTS[wl],
                             fec[0], fec[1], fec[2], P, chunks, pe16, dw16);
                    if (wl != 2) check_layers(label, d);
                    route_cases(label, d, true);
                  }
  printf("# descriptors %lld accepted %lld cases %lld\n", n_desc, n_accepted, n_cases);
  extras();
  printf("# with extras: descriptors %lld accepted %lld cases %lld\n", n_desc, n_accepted, n_cases);
  for (int f = 0; f < 7; ++f) printf("# family %s %lld\n", FAMILY[f], by_family[f]);
  for (int p = 0; p < 3; ++p)
    for (int m = 0; m < 3; ++m) printf("# precision %d mode %d %lld\n", p, m, by_pm[p][m]);
  return 0;
}
