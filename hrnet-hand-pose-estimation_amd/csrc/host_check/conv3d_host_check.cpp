// Stand-alone check of the HOST side of csrc/conv3d.hip under AddressSanitizer and UBSan, on the CPU: the pure query
// and every argument check of the compute entries. No call here reaches a launch (each is refused first), so no GPU is
// needed and none is touched. Build and run, from the package directory:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I ../include -I csrc \
//         csrc/conv3d.hip csrc/host_check/conv3d_host_check.cpp -o conv3d_host_check && ./conv3d_host_check
//
// It supplies the two error-plumbing functions of api.hip itself, so that conv3d.hip links alone.
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
  // the query: every (Cin, Cout, ks) up to beyond the limits, both dtypes
  int yes = 0;
  for (int dtype = -1; dtype <= 2; ++dtype)
    for (int cin = -4; cin <= 4100; ++cin)
      for (int cout = -16; cout <= 4112; cout += (cout % 16 == 0 && cout > 64 && cout < 4080) ? 16 : 1)
        for (int ks = -1; ks <= 8; ++ks) {
          const int r = hrnet_conv3d_supported(dtype, cin, cout, ks);
          const bool want = dtype == HR_F32 && cin >= 4 && cin <= 4096 && cin % 4 == 0 && cout >= 16 && cout <= 4096 &&
                            cout % 16 == 0 && (ks == 1 || ks == 3 || ks == 7);
          if (r != (want ? 1 : 0)) expect(false, "hrnet_conv3d_supported");
          yes += r;
        }
  expect(yes > 0, "hrnet_conv3d_supported never answers 1");
  expect(hrnet_conv3d_supported(HR_BF16, 32, 32, 3) == 0, "bf16 must be unsupported");

  float buf[64] = {0};
  float* x = buf;
  float* y = buf + 32;
  const int big = 0x7fffffff;
  refused(hrnet_conv3d(HR_BF16, x, x, nullptr, x, nullptr, y, 1, 4, 4, 4, 32, 32, 3, 0, nullptr), "only f32", "conv3d bf16");
  refused(hrnet_conv3d(HR_F32, x, x, nullptr, x, nullptr, y, 0, 4, 4, 4, 32, 32, 3, 0, nullptr), "N = 0", "conv3d N = 0");
  refused(hrnet_conv3d(HR_F32, x, x, nullptr, x, nullptr, y, 1, -1, 4, 4, 32, 32, 3, 0, nullptr), "D = -1", "conv3d D < 0");
  refused(hrnet_conv3d(HR_F32, x, x, nullptr, x, nullptr, y, 1, 4, 4, 4, 30, 32, 3, 0, nullptr), "Cin = 30", "conv3d Cin");
  refused(hrnet_conv3d(HR_F32, x, x, nullptr, x, nullptr, y, 1, 4, 4, 4, 32, 24, 3, 0, nullptr), "Cout = 24", "conv3d Cout");
  refused(hrnet_conv3d(HR_F32, x, x, nullptr, x, nullptr, y, 1, 4, 4, 4, big, big, 3, 0, nullptr), "Cin =", "conv3d huge C");
  refused(hrnet_conv3d(HR_F32, x, x, nullptr, x, nullptr, y, big, big, big, big, 32, 32, 3, 0, nullptr), "voxels",
          "conv3d voxel count beyond 2^36 (the product must not overflow)");
  refused(hrnet_conv3d(HR_F32, x, x, nullptr, x, nullptr, y, 1, 4, 4, 4, 32, 32, 5, 0, nullptr), "ks = 5", "conv3d ks");
  refused(hrnet_conv3d(HR_F32, nullptr, x, nullptr, x, nullptr, y, 1, 4, 4, 4, 32, 32, 3, 0, nullptr), "null", "conv3d null x");
  refused(hrnet_conv3d(HR_F32, x, x, nullptr, nullptr, nullptr, y, 1, 4, 4, 4, 32, 32, 3, 0, nullptr), "null", "conv3d null shift");
  refused(hrnet_conv3d(HR_F32, x, x, nullptr, x, nullptr, x, 1, 4, 4, 4, 32, 32, 3, 0, nullptr), "aliases", "conv3d y == x");
  refused(hrnet_conv3d(HR_F32, x, x, nullptr, x, y, y, 1, 4, 4, 4, 32, 32, 3, 0, nullptr), "aliases", "conv3d y == res");

  refused(hrnet_deconv3d_k2s2(HR_BF16, x, x, x, x, nullptr, y, 1, 2, 2, 2, 32, 32, 1, nullptr), "only f32", "deconv bf16");
  refused(hrnet_deconv3d_k2s2(HR_F32, x, x, x, x, nullptr, y, 1, 2, 0, 2, 32, 32, 1, nullptr), "H = 0", "deconv H = 0");
  refused(hrnet_deconv3d_k2s2(HR_F32, x, x, x, x, nullptr, y, 1, 2, 2, 2, 32, 33, 1, nullptr), "Cout = 33", "deconv Cout");
  refused(hrnet_deconv3d_k2s2(HR_F32, x, x, x, x, nullptr, y, 1 << 12, 1 << 8, 1 << 8, 1 << 8, 32, 32, 1, nullptr),
          "output voxels", "deconv output voxel count");
  refused(hrnet_deconv3d_k2s2(HR_F32, x, nullptr, x, x, nullptr, y, 1, 2, 2, 2, 32, 32, 1, nullptr), "null", "deconv null w");
  refused(hrnet_deconv3d_k2s2(HR_F32, x, x, x, x, y, y, 1, 2, 2, 2, 32, 32, 1, nullptr), "aliases", "deconv y == add");

  refused(hrnet_maxpool3d(HR_BF16, x, y, 1, 2, 2, 2, 32, nullptr), "only f32", "maxpool bf16");
  refused(hrnet_maxpool3d(HR_F32, x, y, 1, 3, 2, 2, 32, nullptr), "must be even", "maxpool odd D");
  refused(hrnet_maxpool3d(HR_F32, x, y, 1, 2, 5, 2, 32, nullptr), "must be even", "maxpool odd H");
  refused(hrnet_maxpool3d(HR_F32, x, y, 1, 2, 2, 7, 32, nullptr), "must be even", "maxpool odd W");
  refused(hrnet_maxpool3d(HR_F32, x, y, 1, 1, 2, 2, 32, nullptr), "D = 1", "maxpool D = 1");
  refused(hrnet_maxpool3d(HR_F32, x, y, 1, 2, 2, 2, 30, nullptr), "C = 30", "maxpool C");
  refused(hrnet_maxpool3d(HR_F32, x, x, 1, 2, 2, 2, 32, nullptr), "aliased", "maxpool y == x");
  refused(hrnet_maxpool3d(HR_F32, x, y, big, big - 1, big - 1, big - 1, 4096, nullptr), "output voxels", "maxpool count");
  refused(hrnet_maxpool3d(HR_F32, x, y, 1 << 9, 1 << 10, 1 << 10, 1 << 10, 4096, nullptr), "outputs (at most", "maxpool grid");

  refused(hrnet_pack_weights3d(HR_BF16, x, y, 16, 4, 3, 16, 4, 0, nullptr), "only f32", "pack bf16");
  refused(hrnet_pack_weights3d(HR_F32, nullptr, y, 16, 4, 3, 16, 4, 0, nullptr), "null", "pack null");
  refused(hrnet_pack_weights3d(HR_F32, x, y, 16, 4, 4, 16, 4, 0, nullptr), "ks = 4", "pack ks");
  refused(hrnet_pack_weights3d(HR_F32, x, y, 21, 4, 3, 16, 4, 0, nullptr), "Cout = 21 in 16", "pack Cout_pad < Cout");
  refused(hrnet_pack_weights3d(HR_F32, x, y, 16, 2, 3, 16, 2, 0, nullptr), "Cin = 2 in 2", "pack Cin_pad not a multiple of 4");
  refused(hrnet_pack_weights3d(HR_F32, x, y, 0, 4, 3, 16, 4, 1, nullptr), "Cout = 0", "pack Cout = 0");

  expect(g_launch_checks == 0, "an argument check let a call through to a launch");
  printf(failures ? "conv3d host check: %d FAILED\n" : "conv3d host check: all refused as expected (%d)\n", failures);
  return failures ? 1 : 0;
}
