// Stand-alone reader of recombiner_amd/csrc/siren_route.h (host compiler, no HIP) for the case lists of tests/siren_emul.py:
// prints the fp32 instance list of the header ("instance fp32 NH KS NB", "instance generic ML"), then for every argument
// "hidden,nh,F,E,C,P,rows,S,w0,w1,w2,w3" (w*: the per-layer hidden widths, 0 where none are listed) one line
// "route <argument> -> fp32 NH KS NB | generic ML | refused <code> <text>".  A precision-0 descriptor that siren_check_desc refuses,
// or whose three modes do not name the same instance, ends the program with status 1.
// tests/test_siren_emul_cpu.py builds and runs this.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "../recombiner_amd/csrc/siren_route.h"

static char g_text[512];
int rcb::fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_text, sizeof(g_text), fmt, ap);
  va_end(ap);
  return code;
}

using namespace rcb;

int main(int argc, char** argv) {
#define X(NH, KS, NB) printf("instance fp32 %d %d %d\n", NH, KS, NB);
  RCB_SIREN_FP32_INSTANCES(X)
#undef X
  printf("instance generic %d\ninstance generic %d\n", MAXL, SIREN_MAX_LAYERS);
  for (int i = 1; i < argc; ++i) {
    int v[12];
    if (sscanf(argv[i], "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10,
               v + 11) != 12) {
      fprintf(stderr, "siren_case_routes: cannot read %s\n", argv[i]);
      return 1;
    }
    rcb_siren_desc d;
    memset(&d, 0, sizeof(d));
    d.hidden = v[0], d.n_hidden = v[1], d.fourier_dim = v[2], d.pe_dim = v[3], d.out_dim = v[4], d.n_pix = v[5], d.n_rows = v[6];
    d.samples = v[7], d.w0 = 30.f, d.precision = 0;
    for (int k = 0; k < 4; ++k) d.hidden_dims[k] = v[8 + k];
    SirenLayers L;
    d.w_row_stride = siren_layers(&d).dnet;
    if (siren_check_desc(&d, L) != RCB_OK) {
      fprintf(stderr, "siren_case_routes: %s is refused: %s\n", argv[i], g_text);
      return 1;
    }
    SirenRoute r[3];
    for (int mode = 0; mode < 3; ++mode) r[mode] = siren_route(&d, mode, d.pe_dim > 0 && mode != MODE_FWD, false, 1, 256);
    for (int mode = 1; mode < 3; ++mode)
      if (r[mode].family != r[0].family || memcmp(r[mode].p, r[0].p, sizeof(r[0].p)) != 0) {
        fprintf(stderr, "siren_case_routes: %s: mode %d names another instance than the forward pass\n", argv[i], mode);
        return 1;
      }
    if (r[0].family == SIREN_FP32)
      printf("route %s -> fp32 %d %d %d\n", argv[i], r[0].p[0], r[0].p[1], r[0].p[2]);
    else if (r[0].family == SIREN_GENERIC)
      printf("route %s -> generic %d\n", argv[i], r[0].p[0]);
    else
      printf("route %s -> refused %d %s\n", argv[i], r[0].code, r[0].text);
  }
  return 0;
}
