// Stand-alone check of the HOST side of csrc/pointwise.hip under AddressSanitizer and UBSan, on the CPU: the two query
// functions and every argument check of the forward and the backward. No call here reaches a launch (each is refused
// first), so no GPU is needed and none is touched. Build and run, from the package directory:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I ../include -I csrc \
//         csrc/pointwise.hip csrc/host_check/pointwise_host_check.cpp -o pointwise_host_check && ./pointwise_host_check
//
// It supplies the two error-plumbing functions of api.hip itself, so that pointwise.hip links alone.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

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

  expect(hrnet_pointwise_nchw_supported(HR_F32, 480, 32) == 1 && hrnet_pointwise_nchw_supported(HR_F32, 1, 1) == 1 &&
             hrnet_pointwise_nchw_supported(HR_F32, 65536, 64) == 1 && hrnet_pointwise_nchw_supported(HR_F32, 3, 21) == 1,
         "supported: shapes inside the limits");
  expect(hrnet_pointwise_nchw_supported(HR_BF16, 480, 32) == 0 && hrnet_pointwise_nchw_supported(HR_F32, 0, 32) == 0 &&
             hrnet_pointwise_nchw_supported(HR_F32, 480, 0) == 0 && hrnet_pointwise_nchw_supported(HR_F32, 480, 65) == 0 &&
             hrnet_pointwise_nchw_supported(HR_F32, 65537, 32) == 0 && hrnet_pointwise_nchw_supported(HR_F32, -4, -16) == 0 &&
             hrnet_pointwise_nchw_supported(7, 480, 32) == 0,
         "supported: bf16, zero, negative and oversized channel counts");

  // parts: one row per 32 tiles of 16 pixels until 256 rows are in use; no row is empty; 0 outside the limits
  int asked = 0;
  for (int n : {1, 2, 3, 12, 64, 65535})
    for (long long p : {1LL, 15LL, 16LL, 17LL, 100LL, 256LL, 512LL, 513LL, 4096LL, 65536LL, 1LL << 30}) {
      const int parts = hrnet_pointwise_nchw_parts(n, p);
      const long long tiles = (long long)n * ((p + 15) / 16);
      const long long want = (tiles + 31) / 32;
      expect(parts >= 1 && parts <= 256 && parts <= tiles, "parts within 1..min(256, tiles)");
      if (want <= 256) expect(parts == want, "parts: one per 32 tiles");
      const long long per = (tiles + parts - 1) / parts;
      expect((long long)(parts - 1) * per < tiles, "parts: the last row is not empty");
      ++asked;
    }
  expect(asked == 66, "parts was hardly asked");
  expect(hrnet_pointwise_nchw_parts(1, 1) == 1 && hrnet_pointwise_nchw_parts(2, 4096) == 16 &&
             hrnet_pointwise_nchw_parts(12, 4096) == 96 && hrnet_pointwise_nchw_parts(65535, 1LL << 30) == 256,
         "parts at known sizes");
  expect(hrnet_pointwise_nchw_parts(0, 16) == 0 && hrnet_pointwise_nchw_parts(-1, 16) == 0 &&
             hrnet_pointwise_nchw_parts(1, 0) == 0 && hrnet_pointwise_nchw_parts(1, -7) == 0 &&
             hrnet_pointwise_nchw_parts(65536, 16) == 0 && hrnet_pointwise_nchw_parts(1, (1LL << 30) + 1) == 0 &&
             hrnet_pointwise_nchw_parts(big, 0x7fffffffffffffffLL) == 0,
         "parts outside the limits");

  float buf[128] = {0};
  float* a = buf;
  float* b = buf + 32;
  float* c = buf + 64;
  float* d = buf + 96;

  refused(hrnet_pointwise_nchw(HR_BF16, a, b, c, d, 1, 4, 4, 1, nullptr), "only f32", "forward bf16");
  refused(hrnet_pointwise_nchw(HR_F32, a, b, c, d, 1, 0, 4, 1, nullptr), "Cin = 0", "forward Cin = 0");
  refused(hrnet_pointwise_nchw(HR_F32, a, b, c, d, 1, 4, 65, 1, nullptr), "Cout = 65", "forward Cout = 65");
  refused(hrnet_pointwise_nchw(HR_F32, a, b, c, d, 1, 4, -1, 1, nullptr), "Cout = -1", "forward Cout < 0");
  refused(hrnet_pointwise_nchw(HR_F32, a, b, c, d, 0, 4, 4, 1, nullptr), "N = 0", "forward N = 0");
  refused(hrnet_pointwise_nchw(HR_F32, a, b, c, d, 65536, 4, 4, 1, nullptr), "N = 65536", "forward N beyond the grid");
  refused(hrnet_pointwise_nchw(HR_F32, a, b, c, d, 1, 4, 4, 0, nullptr), "P = 0", "forward P = 0");
  refused(hrnet_pointwise_nchw(HR_F32, a, b, c, d, 1, 4, 4, -3, nullptr), "P = -3", "forward P < 0");
  refused(hrnet_pointwise_nchw(HR_F32, a, b, c, d, 1, 4, 4, (1LL << 30) + 1, nullptr), "2^30", "forward P beyond 2^30");
  refused(hrnet_pointwise_nchw(HR_F32, a, b, c, d, 65535, 65536, 64, 1LL << 30, nullptr), "2^40",
          "forward: more than 2^40 elements (no 64-bit wrap)");
  refused(hrnet_pointwise_nchw(HR_F32, nullptr, b, c, d, 1, 4, 4, 1, nullptr), "null", "forward null x");
  refused(hrnet_pointwise_nchw(HR_F32, a, nullptr, c, d, 1, 4, 4, 1, nullptr), "null", "forward null w");
  refused(hrnet_pointwise_nchw(HR_F32, a, b, c, nullptr, 1, 4, 4, 1, nullptr), "null", "forward null y");
  refused(hrnet_pointwise_nchw(HR_F32, a, b, nullptr, a, 1, 4, 4, 1, nullptr), "aliases", "forward y == x");

  const long long need = 4 * 4 + 4;     // one part of Cout * Cin + Cout floats
  refused(hrnet_pointwise_nchw_bwd(HR_BF16, a, b, c, d, d, d, d, need, 1, 4, 4, 1, nullptr), "only f32", "backward bf16");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, d, d, d, d, need, 1, 4, 0, 1, nullptr), "Cout = 0", "backward Cout = 0");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, d, d, d, d, need, 1, 65537, 4, 1, nullptr), "Cin = 65537",
          "backward Cin beyond the limit");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, d, d, d, d, need, -1, 4, 4, 1, nullptr), "N = -1", "backward N < 0");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, d, d, d, d, need, 1, 4, 4, 0, nullptr), "P = 0", "backward P = 0");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, d, d, d, d, need, 65535, 65536, 64, 1LL << 30, nullptr), "2^40",
          "backward: more than 2^40 elements");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, nullptr, b, c, d, d, d, d, need, 1, 4, 4, 1, nullptr), "null", "backward null x");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, nullptr, c, d, d, d, d, need, 1, 4, 4, 1, nullptr), "null", "backward null w");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, nullptr, d, d, d, d, need, 1, 4, 4, 1, nullptr), "null", "backward null dy");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, nullptr, nullptr, nullptr, d, need, 1, 4, 4, 1, nullptr), "all null",
          "backward with nothing to compute");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, c, nullptr, nullptr, d, need, 1, 4, 4, 1, nullptr), "aliases",
          "backward dx == dy");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, a, nullptr, nullptr, d, need, 1, 4, 4, 1, nullptr), "aliases",
          "backward dx == x");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, nullptr, d, nullptr, nullptr, need, 1, 4, 4, 1, nullptr), "null scratch",
          "backward dw without scratch");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, nullptr, nullptr, d, nullptr, need, 1, 4, 4, 1, nullptr), "null scratch",
          "backward db without scratch");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, nullptr, d, nullptr, d, need - 1, 1, 4, 4, 1, nullptr), "scratch of",
          "backward scratch one float short");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, nullptr, d, d, d, 0, 1, 4, 4, 1, nullptr), "scratch of",
          "backward scratch of no floats");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, nullptr, d, d, d, -5, 1, 4, 4, 1, nullptr), "scratch of",
          "backward scratch of a negative size");
  // 96 rows of 480 * 32 + 32 floats are needed at the model's size: one float short, and a 32-bit wrap of the product
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, nullptr, d, d, d, 96LL * 15392 - 1, 12, 480, 32, 4096, nullptr), "scratch of",
          "backward scratch one float short at (12, 480, 32, 4096)");
  refused(hrnet_pointwise_nchw_bwd(HR_F32, a, b, c, nullptr, d, d, d, 1LL << 30, 2048, 65536, 64, 8192, nullptr), "scratch of",
          "backward: 2^30 floats offered where 256 * (2^22 + 64) are needed (the product is formed in 64 bits)");

  expect(g_launch_checks == 0, "an argument check let a call through to a launch");
  printf(failures ? "pointwise host check: %d FAILED\n" : "pointwise host check: all answered as expected (%d)\n", failures);
  return failures ? 1 : 0;
}
