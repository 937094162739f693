// Stand-alone check of the HOST side of csrc/conv3d_train.hip under AddressSanitizer and UBSan, on the CPU: the scratch
// and split query, the partial-row query and every argument check of the compute entries. No call here reaches a launch
// (each is refused first), so no GPU is needed and none is touched. Build and run, from the package directory:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I ../include -I csrc \
//         csrc/conv3d_train.hip csrc/host_check/conv3d_train_host_check.cpp -o conv3d_train_host_check && \
//         ./conv3d_train_host_check
//
// It supplies the two error-plumbing functions of api.hip itself, so that conv3d_train.hip links alone.
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
  long long bytes = -1;
  int nsplit = -1;
  long long per = -1;

  // the query over every size the network uses and well beyond: splits within 1..256, the scratch is exactly
  // splits * taps * Cout * ceil16(Cin) floats, and the splits cover the voxels
  const int kss[] = {1, 3, 7};
  const int cins[] = {4, 16, 32, 64, 128, 4096};
  const int couts[] = {16, 32, 48, 64, 128, 4096};
  const int exts[] = {1, 2, 3, 7, 16, 64, 512, 2048};
  int asked = 0;
  for (int ks : kss)
    for (int cin : cins)
      for (int cout : couts)
        for (int n : {1, 2, 8, 64})
          for (int e : exts) {
            const long long nvox = (long long)n * e * e * e;
            const int rc = hrnet_conv3d_wgrad_scratch(HR_F32, n, e, e, e, cin, cout, ks, 0, &bytes, &nsplit, &per);
            if (nvox > (1LL << 36)) {
              refused(rc, "voxels", "wgrad_scratch beyond 2^36 voxels");
              continue;
            }
            const long long cin16 = (cin + 15) / 16 * 16;
            expect(rc == HR_OK && nsplit >= 1 && nsplit <= 256 &&
                       bytes == (long long)nsplit * ks * ks * ks * cout * cin16 * 4,
                   "wgrad_scratch: splits or bytes");
            expect(per % 16 == 0 && (long long)(nsplit - 1) * per < nvox && nvox <= (long long)nsplit * per,
                   "wgrad_scratch: the splits of split_voxels each cover the voxels, the last one not empty");
            expect(nvox <= 2048 ? nsplit == 1 : nsplit >= 2, "wgrad_scratch: one split up to 2048 voxels, more beyond");
            ++asked;
          }
  expect(asked > 1000, "wgrad_scratch was hardly asked");
  // counts and sizes beyond 32 bits
  expect(hrnet_conv3d_wgrad_scratch(HR_F32, 64, 512, 512, 512, 128, 128, 3, 0, &bytes, &nsplit, &per) == HR_OK && nsplit == 256 &&
             bytes == 256LL * 27 * 128 * 128 * 4, "wgrad_scratch at 2^33 voxels");
  expect(hrnet_conv3d_wgrad_scratch(HR_F32, 16, 1024, 1024, 4096, 4096, 4096, 7, 0, &bytes, &nsplit, &per) == HR_OK &&
             nsplit == 256 && bytes == 256LL * 343 * 4096 * 4096 * 4 && bytes > (1LL << 42),
         "wgrad_scratch at 2^36 voxels: 5.9e12 bytes of scratch");
  expect(hrnet_conv3d_wgrad_scratch(HR_F32, 8, 1024, 1024, 1024, 128, 128, 2, 1, &bytes, &nsplit, &per) == HR_OK,
         "wgrad_scratch deconvolution: 2^33 input voxels are 2^36 output voxels");
  refused(hrnet_conv3d_wgrad_scratch(HR_F32, 16, 1024, 1024, 1024, 128, 128, 2, 1, &bytes, &nsplit, &per), "output voxels",
          "wgrad_scratch deconvolution beyond 2^36 output voxels");
  refused(hrnet_conv3d_wgrad_scratch(HR_F32, big, big, big, big, 32, 32, 3, 0, &bytes, &nsplit, &per), "voxels",
          "wgrad_scratch: the product must not overflow");
  refused(hrnet_conv3d_wgrad_scratch(HR_BF16, 1, 4, 4, 4, 32, 32, 3, 0, &bytes, &nsplit, &per), "only f32", "wgrad_scratch bf16");
  refused(hrnet_conv3d_wgrad_scratch(HR_F32, 1, 4, 4, 4, 32, 32, 3, 0, nullptr, &nsplit, &per), "null", "wgrad_scratch null");
  refused(hrnet_conv3d_wgrad_scratch(HR_F32, 1, 4, 4, 4, 32, 32, 2, 0, &bytes, &nsplit, &per), "ks = 2", "wgrad_scratch ks 2 conv");
  refused(hrnet_conv3d_wgrad_scratch(HR_F32, 1, 4, 4, 4, 32, 32, 3, 1, &bytes, &nsplit, &per), "ks = 3", "wgrad_scratch ks 3 deconv");
  refused(hrnet_conv3d_wgrad_scratch(HR_F32, 1, 4, 4, 4, 6, 32, 3, 0, &bytes, &nsplit, &per), "Cin = 6", "wgrad_scratch Cin");
  refused(hrnet_conv3d_wgrad_scratch(HR_F32, 1, 4, 4, 4, 32, 8, 3, 0, &bytes, &nsplit, &per), "Cout = 8", "wgrad_scratch Cout");
  refused(hrnet_conv3d_wgrad_scratch(HR_F32, 1, 0, 4, 4, 32, 32, 3, 0, &bytes, &nsplit, &per), "D = 0", "wgrad_scratch D = 0");

  expect(hrnet_bn3d_parts(0) == 0 && hrnet_bn3d_parts(-5) == 0 && hrnet_bn3d_parts(1) == 1 && hrnet_bn3d_parts(256) == 1 &&
             hrnet_bn3d_parts(257) == 2 && hrnet_bn3d_parts(1LL << 36) == 256 && hrnet_bn3d_parts(0x7fffffffffffffffLL - 300) == 256,
         "bn3d_parts");

  float buf[96] = {0};
  float* a = buf;
  float* b = buf + 32;
  float* c = buf + 64;
  long long nbt = 0;

  refused(hrnet_conv3d_wgrad(HR_BF16, a, b, c, 1 << 20, c, 1, 2, 2, 2, 16, 16, 16, 16, 3, 0, 0, nullptr), "only f32", "wgrad bf16");
  refused(hrnet_conv3d_wgrad(HR_F32, a, b, c, 1 << 20, c, 1, 2, 2, 2, 16, 16, 16, 16, 5, 0, 0, nullptr), "ks = 5", "wgrad ks");
  refused(hrnet_conv3d_wgrad(HR_F32, a, b, c, 1 << 20, c, big, big, big, big, 16, 16, 16, 16, 3, 0, 0, nullptr), "voxels", "wgrad count");
  refused(hrnet_conv3d_wgrad(HR_F32, a, b, c, 1 << 20, c, 1, 2, 2, 2, 16, 16, 17, 16, 3, 0, 0, nullptr), "17 real", "wgrad real Cin");
  refused(hrnet_conv3d_wgrad(HR_F32, a, b, c, 1 << 20, c, 1, 2, 2, 2, 16, 16, 16, 0, 3, 0, 0, nullptr), "0 real", "wgrad real Cout");
  refused(hrnet_conv3d_wgrad(HR_F32, nullptr, b, c, 1 << 20, c, 1, 2, 2, 2, 16, 16, 16, 16, 3, 0, 0, nullptr), "null", "wgrad null x");
  refused(hrnet_conv3d_wgrad(HR_F32, a, b, c, 27 * 16 * 16 * 4 - 1, c, 1, 2, 2, 2, 16, 16, 16, 16, 3, 0, 0, nullptr), "scratch of",
          "wgrad scratch one byte short");
  refused(hrnet_conv3d_wgrad(HR_F32, a, b, c, 0xffffffffLL, c, 16, 1024, 1024, 4096, 4096, 4096, 4096, 4096, 7, 0, 0, nullptr),
          "scratch of", "wgrad: 2^32 - 1 bytes offered where 5.9e12 are needed (no 32-bit wrap)");

  refused(hrnet_bn3d_stats(HR_BF16, a, a, a, b, c, c, c, c, nullptr, nullptr, nullptr, 1, 2, 2, 2, 16, 16, 0.1f, 1e-5f, nullptr),
          "only f32", "bn3d_stats bf16");
  refused(hrnet_bn3d_stats(HR_F32, a, a, a, b, c, c, c, c, nullptr, nullptr, nullptr, 1, 1, 1, 1, 16, 16, 0.1f, 1e-5f, nullptr),
          "Expected more than 1 value per channel when training", "bn3d_stats one row");
  refused(hrnet_bn3d_stats(HR_F32, a, a, a, b, c, c, c, c, nullptr, nullptr, nullptr, 1, 2, 2, 2, 2048, 16, 0.1f, 1e-5f, nullptr),
          "C = 2048", "bn3d_stats C beyond one workgroup");
  refused(hrnet_bn3d_stats(HR_F32, a, a, a, b, c, c, c, c, nullptr, nullptr, nullptr, 1, 2, 2, 2, 16, 0, 0.1f, 1e-5f, nullptr),
          "0 are real", "bn3d_stats Creal");
  refused(hrnet_bn3d_stats(HR_F32, a, a, a, b, c, c, c, c, a, nullptr, nullptr, 1, 2, 2, 2, 16, 16, 0.1f, 1e-5f, nullptr),
          "one running statistic", "bn3d_stats running_mean alone");
  refused(hrnet_bn3d_stats(HR_F32, a, a, a, b, c, c, c, c, a, a, &nbt, 1, 2, 2, 2, 16, 16, 1.5f, 1e-5f, nullptr), "momentum",
          "bn3d_stats momentum");
  refused(hrnet_bn3d_stats(HR_F32, a, a, a, nullptr, c, c, c, c, a, a, &nbt, 1, 2, 2, 2, 16, 16, 0.1f, 1e-5f, nullptr), "null",
          "bn3d_stats null scratch");
  refused(hrnet_bn3d_stats(HR_F32, a, a, a, b, c, c, c, c, a, a, &nbt, big, big, big, 2, 16, 16, 0.1f, 1e-5f, nullptr), "voxels",
          "bn3d_stats count");
  expect(nbt == 0, "a refused bn3d_stats touched num_batches_tracked");

  refused(hrnet_bn3d_apply(HR_F32, a, a, a, nullptr, b, 1, 2, 2, 2, 6, 1, 0, nullptr), "C = 6", "bn3d_apply C");
  refused(hrnet_bn3d_apply(HR_F32, a, a, nullptr, nullptr, b, 1, 2, 2, 2, 16, 1, 0, nullptr), "null", "bn3d_apply null");
  refused(hrnet_bn3d_apply(HR_F32, a, a, a, b, b, 1, 2, 2, 2, 16, 1, 0, nullptr), "aliases", "bn3d_apply y == other");
  refused(hrnet_bn3d_apply(HR_F32, a, a, a, nullptr, b, 16, 1024, 1024, 4096, 4096, 1, 0, nullptr), "elements (at most",
          "bn3d_apply: 2^36 rows of 4096 channels are more 16-byte elements than a grid of 2^32 - 1 workgroups holds");
  refused(hrnet_bn3d_apply(HR_BF16, a, a, a, nullptr, b, 1, 2, 2, 2, 16, 1, 0, nullptr), "only f32", "bn3d_apply bf16");

  refused(hrnet_bn3d_bwd(HR_F32, a, b, nullptr, a, a, a, a, c, c + 16, nullptr, nullptr, nullptr, nullptr, 1, 2, 2, 2, 24, 24, 0, 0,
                         0, nullptr), "C = 24", "bn3d_bwd C");
  refused(hrnet_bn3d_bwd(HR_F32, a, b, nullptr, a, a, a, a, nullptr, c, nullptr, nullptr, nullptr, nullptr, 1, 2, 2, 2, 16, 16, 0, 0,
                         0, nullptr), "null", "bn3d_bwd null scratch");
  refused(hrnet_bn3d_bwd(HR_F32, a, b, nullptr, a, a, a, nullptr, c, c + 16, nullptr, nullptr, nullptr, nullptr, 1, 2, 2, 2, 16, 16,
                         0, 0, 0, nullptr), "null", "bn3d_bwd null invstd");
  refused(hrnet_bn3d_bwd(HR_F32, a, b, nullptr, a, a, a, a, c, a, nullptr, nullptr, nullptr, nullptr, 1, 2, 2, 2, 16, 16, 0, 0, 0,
                         nullptr), "aliases", "bn3d_bwd dz == dy");
  refused(hrnet_bn3d_bwd(HR_F32, a, b, nullptr, a, a, a, a, c, c + 16, a, nullptr, nullptr, nullptr, 1, 2, 2, 2, 16, 16, 0, 0, 0,
                         nullptr), "aliases", "bn3d_bwd dother == dy");
  refused(hrnet_bn3d_bwd(HR_F32, a, b, b, a, a, a, a, c, c + 16, nullptr, nullptr, nullptr, nullptr, 1, 2, 2, 2, 16, 16, 1, 0, 0,
                         nullptr), "both", "bn3d_bwd saved output and recomputed mask");
  refused(hrnet_bn3d_bwd(HR_F32, a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c, c + 16, nullptr, nullptr, nullptr, b, 1,
                         2, 2, 2, 16, 16, 0, 0, 0, nullptr), "without z", "bn3d_bwd dz without a BatchNorm");

  refused(hrnet_bn3d_bwd(HR_F32, a, b, nullptr, a, a, a, a, c, c + 16, nullptr, nullptr, nullptr, nullptr, 16, 1024, 1024, 4096,
                         1024, 1024, 0, 0, 0, nullptr), "elements (at most", "bn3d_bwd grid");
  expect(hrnet_conv3d_wgrad_scratch(HR_F32, 1, 16, 16, 20, 16, 32, 3, 0, &bytes, &nsplit, nullptr) == HR_OK && nsplit == 3,
         "wgrad_scratch without split_voxels");

  refused(hrnet_maxpool3d_bwd(HR_BF16, a, b, c, 1, 2, 2, 2, 32, 0, nullptr), "only f32", "maxpool_bwd bf16");
  refused(hrnet_maxpool3d_bwd(HR_F32, a, b, c, 1, 3, 2, 2, 32, 0, nullptr), "must be even", "maxpool_bwd odd D");
  refused(hrnet_maxpool3d_bwd(HR_F32, a, b, c, 1, 2, 2, 2, 30, 0, nullptr), "C = 30", "maxpool_bwd C");
  refused(hrnet_maxpool3d_bwd(HR_F32, a, b, a, 1, 2, 2, 2, 32, 0, nullptr), "aliased", "maxpool_bwd dx == x");
  refused(hrnet_maxpool3d_bwd(HR_F32, a, b, c, big, big - 1, big - 1, big - 1, 4096, 0, nullptr), "output voxels", "maxpool_bwd count");
  refused(hrnet_maxpool3d_bwd(HR_F32, a, b, c, 1 << 9, 1 << 10, 1 << 10, 1 << 10, 4096, 0, nullptr), "outputs (at most", "maxpool_bwd grid");

  refused(hrnet_pack_weights3d_dgrad(HR_BF16, a, b, 16, 4, 3, 16, 16, nullptr), "only f32", "pack_dgrad bf16");
  refused(hrnet_pack_weights3d_dgrad(HR_F32, a, nullptr, 16, 4, 3, 16, 16, nullptr), "null", "pack_dgrad null");
  refused(hrnet_pack_weights3d_dgrad(HR_F32, a, b, 16, 4, 2, 16, 16, nullptr), "ks = 2", "pack_dgrad ks");
  refused(hrnet_pack_weights3d_dgrad(HR_F32, a, b, 16, 4, 3, 16, 4, nullptr), "Cin = 4 in 4", "pack_dgrad Cin_pad not a multiple of 16");
  refused(hrnet_pack_weights3d_dgrad(HR_F32, a, b, 21, 4, 3, 16, 16, nullptr), "Cout = 21 in 16", "pack_dgrad Cout_pad < Cout");

  refused(hrnet_deconv3d_k2s2_dgrad(HR_BF16, a, b, c, 1, 2, 2, 2, 32, 32, 0, nullptr), "only f32", "deconv_dgrad bf16");
  refused(hrnet_deconv3d_k2s2_dgrad(HR_F32, a, b, c, 1, 2, 2, 2, 4, 32, 0, nullptr), "Cin = 4", "deconv_dgrad Cin");
  refused(hrnet_deconv3d_k2s2_dgrad(HR_F32, a, b, c, 1 << 12, 1 << 8, 1 << 8, 1 << 8, 32, 32, 0, nullptr), "output voxels",
          "deconv_dgrad output voxel count");
  refused(hrnet_deconv3d_k2s2_dgrad(HR_F32, a, b, a, 1, 2, 2, 2, 32, 32, 0, nullptr), "aliased", "deconv_dgrad dx == dz");
  refused(hrnet_deconv3d_k2s2_dgrad(HR_F32, a, nullptr, c, 1, 2, 2, 2, 32, 32, 0, nullptr), "null", "deconv_dgrad null w");

  expect(g_launch_checks == 0, "an argument check let a call through to a launch");
  printf(failures ? "conv3d_train host check: %d FAILED\n" : "conv3d_train host check: all answered as expected (%d)\n", failures);
  return failures ? 1 : 0;
}
