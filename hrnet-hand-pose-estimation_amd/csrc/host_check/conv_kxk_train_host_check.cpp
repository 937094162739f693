// Stand-alone check of the HOST side of csrc/conv_kxk_train.hip under AddressSanitizer and UBSan, on the CPU: the split
// and scratch-size arithmetic of the weight gradient (csrc/conv_kxk_split.h, through the query entry and directly) and
// every argument check of the compute entries. No call here reaches a launch (each is refused first), so no GPU is
// needed and none is touched. Build and run, from the package directory:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I ../include -I csrc \
//         csrc/conv_kxk_train.hip csrc/host_check/conv_kxk_train_host_check.cpp -o conv_kxk_train_host_check && \
//         ./conv_kxk_train_host_check
//
// It supplies the two error-plumbing functions of api.hip itself, so that conv_kxk_train.hip links alone.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "conv_kxk_split.h"
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

  // the query over every shape the network uses and well beyond: the splits cover the tiles, none is empty, the scratch
  // is exactly splits * (blocks * units * 256 + 16 cot) floats, and asking twice gives the same answer
  const int kss[] = {1, 3, 5, 7, 9, 11};
  const int cins[] = {4, 8, 20, 32, 56, 128, 512, 4096};
  const int couts[] = {1, 16, 22, 32, 128, 512, 4097};
  const int exts[] = {1, 2, 7, 8, 9, 16, 17, 32, 46, 256, 368, 4096};
  int asked = 0;
  for (int ks : kss)
    for (int cin : cins)
      for (int cout : couts)
        for (int n : {1, 3, 16, 1000})
          for (int h : exts)
            for (int w : {1, 16, 33, 368}) {
              const int rc = hrnet_conv2d_kxk_wgrad_scratch(HR_F32, n, h, w, cin, cout, ks, &bytes, &nsplit, &per);
              const long long tiles = (long long)n * ((h + 7) / 8) * ((w + 15) / 16);
              const long long cot = (cout + 15) / 16, cit = cin == 4 ? 1 : (cin + 15) / 16;
              const long long units = cin == 4 ? ks * ((ks + 3) / 4) : ks * ks;
              expect(rc == HR_OK && nsplit >= 1 && nsplit <= KXW_MAX_SPLIT && nsplit <= tiles, "wgrad_scratch: splits");
              expect(bytes == (long long)nsplit * (cot * cit * units * 256 + cot * 16) * 4, "wgrad_scratch: bytes");
              expect(per >= 1 && (long long)(nsplit - 1) * per < tiles && tiles <= (long long)nsplit * per,
                     "wgrad_scratch: the splits cover the tiles, the last one not empty");
              long long b2 = -1, p2 = -1;
              int n2 = -1;
              expect(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, n, h, w, cin, cout, ks, &b2, &n2, &p2) == HR_OK && b2 == bytes &&
                         n2 == nsplit && p2 == per, "wgrad_scratch: the same shape, the same plan");
              KxwPlan p;
              expect(kxw_plan(n, h, w, cin, cout, ks, &p) == 1 && p.nsplit == nsplit && p.per == per && p.bytes == bytes &&
                         p.tiles == tiles, "kxw_plan agrees with the entry");
              ++asked;
            }
  expect(asked > 10000, "wgrad_scratch was hardly asked");
  // the layers of the network: 11x11 128 -> 128 on 32 x 32 maps fills the device at one image and at sixteen
  expect(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, 1, 32, 32, 128, 128, 11, &bytes, &nsplit, &per) == HR_OK && nsplit == 8 &&
             per == 1, "11x11 128 -> 128, B = 1: 8 tiles, 8 splits of 64 blocks");
  expect(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, 16, 32, 32, 128, 128, 11, &bytes, &nsplit, &per) == HR_OK && nsplit == 16 &&
             per == 8 && bytes == 16LL * (64 * 121 * 256 + 128) * 4, "11x11 128 -> 128, B = 16: 128 tiles, 16 splits");
  expect(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, 16, 256, 256, 4, 128, 9, &bytes, &nsplit, nullptr) == HR_OK && nsplit == 128,
         "9x9 image layer, B = 16: 8192 tiles in 128 splits, split_tiles not asked");
  // counts beyond 32 bits
  expect(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, 1 << 20, 64, 256, 4096, 4096, 11, &bytes, &nsplit, &per) == HR_OK &&
             bytes == (long long)nsplit * (65536LL * 121 * 256 + 4096) * 4 && bytes > (1LL << 32), "wgrad_scratch: 64-bit bytes");
  refused(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, big, big, big, 128, 128, 3, &bytes, &nsplit, &per), "pixel tiles",
          "wgrad_scratch: the tile count must not overflow");
  refused(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, big, 8, 32, 128, 128, 3, &bytes, &nsplit, &per), "pixel tiles",
          "wgrad_scratch: 2^32 tiles");
  refused(hrnet_conv2d_kxk_wgrad_scratch(HR_BF16, 1, 4, 4, 32, 32, 3, &bytes, &nsplit, &per), "only f32", "wgrad_scratch bf16");
  refused(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, 1, 4, 4, 32, 32, 3, nullptr, &nsplit, &per), "null", "wgrad_scratch null");
  refused(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, 1, 4, 4, 32, 32, 4, &bytes, &nsplit, &per), "ks = 4", "wgrad_scratch even ks");
  refused(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, 1, 4, 4, 32, 32, 13, &bytes, &nsplit, &per), "ks = 13", "wgrad_scratch ks 13");
  refused(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, 1, 4, 4, 6, 32, 3, &bytes, &nsplit, &per), "Cin = 6", "wgrad_scratch Cin");
  refused(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, 1, 0, 4, 32, 32, 3, &bytes, &nsplit, &per), "H = 0", "wgrad_scratch H = 0");
  refused(hrnet_conv2d_kxk_wgrad_scratch(HR_F32, 1, 4, 4, 32, 0, 3, &bytes, &nsplit, &per), "Cout = 0", "wgrad_scratch Cout");

  alignas(16) float buf[256] = {0};
  float* a = buf;
  float* b = buf + 64;
  float* c = buf + 128;
  float* d = buf + 192;
  const long long room = 1 << 24;
  refused(hrnet_conv2d_kxk_wgrad(HR_BF16, a, b, c, room, d, nullptr, 1, 2, 2, 16, 16, 16, 0, 16, 16, 0, 3, nullptr), "only f32", "wgrad bf16");
  refused(hrnet_conv2d_kxk_wgrad(HR_F32, a, b, c, room, d, nullptr, 1, 2, 2, 16, 16, 16, 0, 16, 16, 0, 2, nullptr), "ks = 2", "wgrad ks");
  refused(hrnet_conv2d_kxk_wgrad(HR_F32, nullptr, b, c, room, d, nullptr, 1, 2, 2, 16, 16, 16, 0, 16, 16, 0, 3, nullptr), "null", "wgrad null x");
  refused(hrnet_conv2d_kxk_wgrad(HR_F32, a, b, nullptr, room, d, nullptr, 1, 2, 2, 16, 16, 16, 0, 16, 16, 0, 3, nullptr), "null", "wgrad null scratch");
  refused(hrnet_conv2d_kxk_wgrad(HR_F32, a, b, c, room, d, nullptr, 1, 2, 2, 16, 17, 16, 0, 16, 16, 0, 3, nullptr), "17 real", "wgrad real Cin");
  refused(hrnet_conv2d_kxk_wgrad(HR_F32, a, b, c, room, d, nullptr, 1, 2, 2, 16, 0, 16, 0, 16, 16, 0, 3, nullptr), "0 real", "wgrad no real Cin");
  refused(hrnet_conv2d_kxk_wgrad(HR_F32, a, b, c, room, d, nullptr, 1, 2, 2, 16, 16, 18, 0, 16, 16, 0, 3, nullptr), "ldx = 18", "wgrad ldx");
  refused(hrnet_conv2d_kxk_wgrad(HR_F32, a, b, c, room, d, nullptr, 1, 2, 2, 16, 16, 16, 4, 16, 16, 0, 3, nullptr), "outside ldx", "wgrad x slice");
  refused(hrnet_conv2d_kxk_wgrad(HR_F32, a, b, c, room, d, nullptr, 1, 2, 2, 16, 16, 16, 0, 16, 16, 1, 3, nullptr), "outside ldy", "wgrad dy slice");
  refused(hrnet_conv2d_kxk_wgrad(HR_F32, a, b, c, room, d, nullptr, 1, 2, 2, 16, 16, 16, 0, 16, 16, -1, 3, nullptr), "outside ldy", "wgrad y_off < 0");
  refused(hrnet_conv2d_kxk_wgrad(HR_F32, a + 1, b, c, room, d, nullptr, 1, 2, 2, 16, 16, 16, 0, 16, 16, 0, 3, nullptr), "16-byte", "wgrad x alignment");
  refused(hrnet_conv2d_kxk_wgrad(HR_F32, a, b, c, (9 * 256 + 16) * 4 - 1, d, nullptr, 1, 2, 2, 16, 16, 16, 0, 16, 16, 0, 3, nullptr),
          "scratch of", "wgrad scratch one byte short");
  refused(hrnet_conv2d_kxk_wgrad(HR_F32, a, b, c, 0xffffffffLL, d, nullptr, 1 << 20, 64, 256, 4096, 4096, 4096, 0, 4096, 4096, 0, 11, nullptr),
          "scratch of", "wgrad: 2^32 - 1 bytes offered where far more are needed (no 32-bit wrap)");

  refused(hrnet_conv2d_kxk_dgrad(HR_BF16, a, b, c, nullptr, 1, 2, 2, 16, 16, 0, 16, 16, 0, 0, 0, 3, 0, nullptr), "only f32", "dgrad bf16");
  refused(hrnet_conv2d_kxk_dgrad(HR_F32, a, nullptr, c, nullptr, 1, 2, 2, 16, 16, 0, 16, 16, 0, 0, 0, 3, 0, nullptr), "null", "dgrad null w");
  refused(hrnet_conv2d_kxk_dgrad(HR_F32, a, b, c, nullptr, 1, 2, 2, 16, 16, 0, 16, 16, 0, 0, 0, 13, 0, nullptr), "ks = 13", "dgrad ks");
  refused(hrnet_conv2d_kxk_dgrad(HR_F32, a, b, c, nullptr, 1, 2, 2, 22, 24, 0, 16, 16, 0, 0, 0, 3, 0, nullptr), "Cout = 22", "dgrad Cout");
  refused(hrnet_conv2d_kxk_dgrad(HR_F32, a, b, c, nullptr, 1, 2, 2, 16, 16, 4, 16, 16, 0, 0, 0, 3, 0, nullptr), "outside ldy", "dgrad dy slice");
  refused(hrnet_conv2d_kxk_dgrad(HR_F32, a, b, c, nullptr, 1, 2, 2, 16, 16, 0, 16, 16, 1, 0, 0, 3, 0, nullptr), "outside ldx", "dgrad dx slice");
  refused(hrnet_conv2d_kxk_dgrad(HR_F32, a, b, c, d, 1, 2, 2, 16, 16, 0, 16, 16, 0, 16, 1, 3, 0, nullptr), "outside ldm", "dgrad mask slice");
  refused(hrnet_conv2d_kxk_dgrad(HR_F32, a, b, c, nullptr, 1, 2, 2, 16, 16, 0, 16, 16, 0, 0, 0, 3, 2, nullptr), "accumulate = 2", "dgrad accumulate");
  refused(hrnet_conv2d_kxk_dgrad(HR_F32, a, b, a, nullptr, 1, 2, 2, 16, 16, 0, 16, 16, 0, 0, 0, 3, 0, nullptr), "aliased", "dgrad dx == dy");
  refused(hrnet_conv2d_kxk_dgrad(HR_F32, a, b, c, nullptr, big, big, big, 16, 16, 0, 16, 16, 0, 0, 0, 3, 0, nullptr), "pixel tiles", "dgrad count");

  refused(hrnet_maxpool2d_3x3s2_bwd(nullptr, b, c, 1, 2, 2, 4, 4, 0, 4, 0, 4, 0, 0, nullptr), "null", "pool_bwd null");
  refused(hrnet_maxpool2d_3x3s2_bwd(a, b, c, 1, 0, 2, 4, 4, 0, 4, 0, 4, 0, 0, nullptr), "H = 0", "pool_bwd H");
  refused(hrnet_maxpool2d_3x3s2_bwd(a, b, c, 1, 2, 2, 4, 4, 1, 4, 0, 4, 0, 0, nullptr), "in ldx = 4", "pool_bwd x slice");
  refused(hrnet_maxpool2d_3x3s2_bwd(a, b, c, 1, 2, 2, 4, 4, 0, 4, 1, 4, 0, 0, nullptr), "in lddy = 4", "pool_bwd dy slice");
  refused(hrnet_maxpool2d_3x3s2_bwd(a, b, c, 1, 2, 2, 4, 4, 0, 4, 0, 4, -1, 0, nullptr), "in lddx = 4", "pool_bwd dx slice");
  refused(hrnet_maxpool2d_3x3s2_bwd(a, b, a, 1, 2, 2, 4, 4, 0, 4, 0, 4, 0, 0, nullptr), "aliased", "pool_bwd dx == x");
  refused(hrnet_maxpool2d_3x3s2_bwd(a, b, c, 1, 2, 2, 4, 4, 0, 4, 0, 4, 0, 2, nullptr), "relu_mask = 2", "pool_bwd relu_mask");

  for (int i = 0; i < 256; ++i) expect(buf[i] == 0.f, "a refused call wrote");
  expect(g_launch_checks == 0, "an argument check let a call through to a launch");
  printf(failures ? "conv_kxk_train host check: %d FAILED\n" : "conv_kxk_train host check: all answered as expected (%d)\n",
         failures ? failures : asked);
  return failures ? 1 : 0;
}
