// Stand-alone check of the HOST side of csrc/ftl_train.hip under AddressSanitizer and UBSan, on the CPU: the split and
// scratch-size arithmetic of the 3x3 weight gradient (csrc/ftl_train_plan.h, through the query entry and directly), the
// output-size range, and every argument check of the compute entries. No call here reaches a launch (each is refused
// first), so no GPU is needed and none is touched. Build and run, from the package directory:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I ../include -I csrc \
//         csrc/ftl_train.hip csrc/host_check/ftl_train_host_check.cpp -o ftl_train_host_check && ./ftl_train_host_check
//
// It supplies the two error-plumbing functions of api.hip itself, so that ftl_train.hip links alone.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "ftl_train_plan.h"
#include "hrnet_hip.h"

static char g_err[512];
static int g_launch_checks = 0;

void hr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int hr_check_launch(const char*) {
  ++g_launch_checks;            // reached only after a launch: must stay 0 here
  return HR_E_LAUNCH;
}

static int failures = 0;

static void expect(bool ok, const char* what) {
  if (!ok) {
    ++failures;
    printf("FAILED: %s (last error: %s)\n", what, g_err);
  }
}

static void refused(int rc, const char* needle, const char* what) {
  expect(rc == HR_E_BADARG && strstr(g_err, needle) != nullptr, what);
  g_err[0] = 0;
}

int main() {
  const int big = 0x7fffffff;
  long long bytes = -1, per = -1;
  int nsplit = -1;

  // the query over the head's shapes and well beyond: the splits cover the tiles, none is empty, the scratch is exactly
  // splits * (blocks * 9 * 256 + 16 cot) floats with a 4-channel input planned as one 16-channel block, and asking twice
  // gives the same answer
  const int cins[] = {4, 8, 20, 56, 240, 256, 480, 4096};
  const int couts[] = {1, 16, 21, 240, 256, 480, 4097};
  const int exts[] = {1, 2, 3, 8, 9, 10, 16, 17, 18, 33, 64, 256, 4096};
  int asked = 0;
  for (int cin : cins)
    for (int cout : couts)
      for (int n : {1, 3, 4, 16, 1000})
        for (int h : exts)
          for (int w : {1, 5, 16, 18, 33, 368}) {
            const int rc = hrnet_conv2d_3x3g_wgrad_scratch(HR_F32, n, h, w, cin, cout, &bytes, &nsplit, &per);
            const long long tiles = (long long)n * ((h + 7) / 8) * ((w + 15) / 16);
            const long long cot = (cout + 15) / 16, cit = (cin + 15) / 16;
            expect(rc == HR_OK && nsplit >= 1 && nsplit <= KXW_MAX_SPLIT && nsplit <= tiles, "wgrad_scratch: splits");
            expect(bytes == (long long)nsplit * (cot * cit * 9 * 256 + cot * 16) * 4, "wgrad_scratch: bytes");
            expect(per >= 1 && (long long)(nsplit - 1) * per < tiles && tiles <= (long long)nsplit * per,
                   "wgrad_scratch: the splits cover the tiles, the last one not empty");
            long long b2 = -1, p2 = -1;
            int n2 = -1;
            expect(hrnet_conv2d_3x3g_wgrad_scratch(HR_F32, n, h, w, cin, cout, &b2, &n2, &p2) == HR_OK && b2 == bytes &&
                       n2 == nsplit && p2 == per, "wgrad_scratch: the same shape, the same plan");
            KxwPlan p;
            expect(g3w_plan(n, h, w, cin, cout, &p) == 1 && p.nsplit == nsplit && p.per == per && p.bytes == bytes &&
                       p.tiles == tiles && p.cin4 == 0 && p.units == 9, "g3w_plan agrees with the entry");
            ++asked;
          }
  expect(asked > 10000, "wgrad_scratch was hardly asked");
  // the head's layers at B x V = 1 x 4
  expect(hrnet_conv2d_3x3g_wgrad_scratch(HR_F32, 4, 18, 18, 480, 240, &bytes, &nsplit, &per) == HR_OK && nsplit == 3 && per == 8,
         "encoder_head.1: 24 tiles of 450 blocks in 3 splits");
  expect(hrnet_conv2d_3x3g_wgrad_scratch(HR_F32, 4, 33, 33, 256, 256, &bytes, &nsplit, nullptr) == HR_OK && nsplit == 4,
         "decoder.1, roles swapped: 60 tiles of 256 blocks in 4 splits, split_tiles not asked");
  expect(hrnet_conv2d_3x3g_wgrad_scratch(HR_F32, 1 << 20, 64, 256, 16384, 16384, &bytes, &nsplit, &per) == HR_OK &&
             bytes == (long long)nsplit * (1048576LL * 9 * 256 + 16384) * 4 && bytes > (1LL << 32), "wgrad_scratch: 64-bit bytes");
  refused(hrnet_conv2d_3x3g_wgrad_scratch(HR_F32, big, big, big, 128, 128, &bytes, &nsplit, &per), "pixel tiles",
          "wgrad_scratch: the tile count must not overflow");
  refused(hrnet_conv2d_3x3g_wgrad_scratch(HR_BF16, 1, 4, 4, 32, 32, &bytes, &nsplit, &per), "only f32", "wgrad_scratch bf16");
  refused(hrnet_conv2d_3x3g_wgrad_scratch(HR_F32, 1, 4, 4, 32, 32, nullptr, &nsplit, &per), "null", "wgrad_scratch null");
  refused(hrnet_conv2d_3x3g_wgrad_scratch(HR_F32, 1, 4, 4, 6, 32, &bytes, &nsplit, &per), "Cin = 6", "wgrad_scratch Cin");
  refused(hrnet_conv2d_3x3g_wgrad_scratch(HR_F32, 1, 0, 4, 32, 32, &bytes, &nsplit, &per), "Ho = 0", "wgrad_scratch Ho = 0");

  // the size range is the forward's: Conv2d(3, 2, 2) takes 64 -> 33 and 33 -> 18, and a transposed layer's output gradient
  // of 2 H - 3 + op rows has the layer's H input rows in range for op 0 and 1
  long long lo = -1, hi = -1;
  g3w_size_range(64, 2, 2, &lo, &hi);
  expect(lo == 32 && hi == 33, "size range of 64 at stride 2, pad_lo 2");
  g3w_size_range(33, 2, 2, &lo, &hi);
  expect(lo == 17 && hi == 18, "size range of 33 at stride 2, pad_lo 2");
  for (int h = 2; h < 200; ++h)
    for (int op = 0; op < 2; ++op) {
      g3w_size_range(2 * h - 3 + op, 2, 2, &lo, &hi);
      expect(lo <= h && h <= hi, "a transposed layer's input height lies in the range of its output gradient");
    }
  g3w_size_range(1, 1, 0, &lo, &hi);
  expect(lo == 1 && hi == 1, "size range of one row without padding");
  g3w_size_range(0x3fffffff, 1, 2, &lo, &hi);
  expect(lo == 0x3fffffff && hi == 0x3fffffffLL + 2, "size range near the largest map");

  alignas(16) float buf[256] = {0};
  float* a = buf;
  float* b = buf + 64;
  float* c = buf + 128;
  float* d = buf + 192;
  const long long room = 1 << 24;
  //                                  x  dy scr       dw N  H  W  Cin real ldx xo Cout ldy yo Ho Wo s  p
  refused(hrnet_conv2d_3x3g_wgrad(HR_BF16, a, b, c, room, d, 1, 4, 8, 16, 16, 16, 0, 16, 16, 0, 3, 5, 2, 2, nullptr), "only f32", "wgrad bf16");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, nullptr, b, c, room, d, 1, 4, 8, 16, 16, 16, 0, 16, 16, 0, 3, 5, 2, 2, nullptr), "null", "wgrad null x");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, nullptr, room, d, 1, 4, 8, 16, 16, 16, 0, 16, 16, 0, 3, 5, 2, 2, nullptr), "null", "wgrad null scratch");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, room, d, 1, 4, 8, 16, 16, 16, 0, 16, 16, 0, 3, 5, 3, 2, nullptr), "stride = 3", "wgrad stride");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, room, d, 1, 4, 8, 16, 16, 16, 0, 16, 16, 0, 3, 5, 2, 3, nullptr), "pad_lo = 3", "wgrad pad_lo");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, room, d, 1, 4, 8, 16, 16, 16, 0, 16, 16, 0, 4, 5, 2, 2, nullptr), "Ho x Wo", "wgrad Ho above the range");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, room, d, 1, 4, 8, 16, 16, 16, 0, 16, 16, 0, 1, 5, 2, 2, nullptr), "Ho x Wo", "wgrad Ho below the range");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, room, d, 1, 4, 8, 16, 16, 16, 0, 16, 16, 0, 3, 6, 2, 2, nullptr), "Ho x Wo", "wgrad Wo above the range");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, room, d, 1, 0, 8, 16, 16, 16, 0, 16, 16, 0, 3, 5, 2, 2, nullptr), "H = 0", "wgrad H = 0");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, room, d, 1, 4, 8, 16, 17, 16, 0, 16, 16, 0, 3, 5, 2, 2, nullptr), "17 real", "wgrad real Cin");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, room, d, 1, 4, 8, 16, 0, 16, 0, 16, 16, 0, 3, 5, 2, 2, nullptr), "0 real", "wgrad no real Cin");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, room, d, 1, 4, 8, 16, 16, 18, 0, 16, 16, 0, 3, 5, 2, 2, nullptr), "ldx = 18", "wgrad ldx");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, room, d, 1, 4, 8, 16, 16, 16, 4, 16, 16, 0, 3, 5, 2, 2, nullptr), "outside ldx", "wgrad x slice");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, room, d, 1, 4, 8, 16, 16, 16, 0, 16, 16, 1, 3, 5, 2, 2, nullptr), "outside ldy", "wgrad dy slice");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, room, d, 1, 4, 8, 16, 16, 16, 0, 16, 16, -1, 3, 5, 2, 2, nullptr), "outside ldy", "wgrad y_off < 0");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a + 1, b, c, room, d, 1, 4, 8, 16, 16, 16, 0, 16, 16, 0, 3, 5, 2, 2, nullptr), "16-byte", "wgrad x alignment");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, (9 * 256 + 16) * 4 - 1, d, 1, 4, 8, 16, 16, 16, 0, 16, 16, 0, 3, 5, 2, 2, nullptr),
          "scratch of", "wgrad scratch one byte short");
  refused(hrnet_conv2d_3x3g_wgrad(HR_F32, a, b, c, 0xffffffffLL, d, 1 << 20, 127, 511, 16384, 16384, 16384, 0, 16384, 16384, 0, 64, 256, 2, 2, nullptr),
          "scratch of", "wgrad: 2^32 - 1 bytes offered where far more are needed (no 32-bit wrap)");

  //                           src coef dst B  V  H  W  C  ld off ...
  refused(hrnet_ftl_gather_bwd(nullptr, b, c, 1, 3, 3, 4, 20, 60, 0, 20, 20, 0, nullptr), "null", "gather_bwd null");
  refused(hrnet_ftl_gather_bwd(a, b, c, 1, 3, 4, 4, 20, 60, 0, 20, 20, 0, nullptr), "triplets", "gather_bwd 16 pixels");
  refused(hrnet_ftl_gather_bwd(a, b, c, 1, 3, 3, 4, 20, 60, 0, 16, 20, 0, nullptr), "slice = 16", "gather_bwd slice below C");
  refused(hrnet_ftl_gather_bwd(a, b, c, 1, 3, 3, 4, 20, 60, 0, 22, 20, 0, nullptr), "slice = 22", "gather_bwd slice alignment");
  refused(hrnet_ftl_gather_bwd(a, b, c, 1, 3, 3, 4, 18, 60, 0, 20, 20, 0, nullptr), "multiples of 4", "gather_bwd C");
  refused(hrnet_ftl_gather_bwd(a, b, c, 1, 3, 3, 4, 20, 64, 2, 20, 20, 0, nullptr), "multiples of 4", "gather_bwd d_off");
  refused(hrnet_ftl_gather_bwd(a, b, c, 1, 3, 3, 4, 20, 56, 0, 20, 20, 0, nullptr), "outside ld", "gather_bwd: the slices of the views outside ldd");
  refused(hrnet_ftl_gather_bwd(a, b, c, 1, 3, 3, 4, 20, 60, 0, 20, 20, 4, nullptr), "outside ld", "gather_bwd dx slice");
  refused(hrnet_ftl_gather_bwd(a + 1, b, c, 1, 3, 3, 4, 20, 60, 0, 20, 20, 0, nullptr), "16-byte", "gather_bwd alignment");
  refused(hrnet_ftl_gather_bwd(a, b, a, 1, 3, 3, 4, 20, 60, 0, 20, 20, 0, nullptr), "aliased", "gather_bwd dx == dcat");
  refused(hrnet_ftl_gather_bwd(a, b, c, big, 3, 3, 4, 20, 60, 0, 20, 20, 0, nullptr), "B V", "gather_bwd B V beyond 2^31");
  refused(hrnet_ftl_scatter_bwd(a, nullptr, c, 1, 3, 3, 4, 20, 20, 0, 20, 0, nullptr), "null", "scatter_bwd null coef");
  refused(hrnet_ftl_scatter_bwd(a, b, c, 1, 3, 2, 2, 20, 20, 0, 20, 0, nullptr), "triplets", "scatter_bwd 4 pixels");
  refused(hrnet_ftl_scatter_bwd(a, b, c, 1, 0, 3, 4, 20, 20, 0, 20, 0, nullptr), "V = 0", "scatter_bwd V");
  refused(hrnet_ftl_scatter_bwd(a, b, c, 1, 3, 3, 4, 20, 20, 4, 20, 0, nullptr), "outside ld", "scatter_bwd dy slice");
  refused(hrnet_ftl_scatter_bwd(a, b, c, 1, 3, 3, 4, 20, 20, 0, 20, -4, nullptr), "outside ld", "scatter_bwd f_off < 0");
  refused(hrnet_ftl_scatter_bwd(a, b, c, 1, 3, 3, 4, 20, 22, 0, 20, 0, nullptr), "multiples of 4", "scatter_bwd ldy");

  for (int i = 0; i < 256; ++i) expect(buf[i] == 0.f, "a refused call wrote");
  expect(g_launch_checks == 0, "an argument check let a call through to a launch");
  printf(failures ? "ftl_train host check: %d FAILED\n" : "ftl_train host check: all answered as expected (%d)\n",
         failures ? failures : asked);
  return failures ? 1 : 0;
}
