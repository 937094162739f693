// Stand-alone check of the HOST side of csrc/transformer.hip under AddressSanitizer and UBSan, on the CPU: the two query
// functions and every argument check of every entry. No call here reaches a launch (each is refused first), so no GPU is
// needed and none is touched. Build and run, from the package directory:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I ../include -I csrc \
//         csrc/transformer.hip csrc/host_check/transformer_host_check.cpp -o transformer_host_check && \
//         ./transformer_host_check
//
// It supplies the two error-plumbing functions of api.hip itself, so that transformer.hip links alone.
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
  const long long huge = 0x7fffffffffffffffLL;

  // the query
  expect(hrnet_tf_supported(HR_TF_LAYERNORM, 32, 0) == 1 && hrnet_tf_supported(HR_TF_LAYERNORM, 672, 0) == 1 &&
             hrnet_tf_supported(HR_TF_LAYERNORM, 1, 0) == 1 && hrnet_tf_supported(HR_TF_LAYERNORM, 65536, 0) == 1,
         "supported: layernorm widths inside the limits");
  expect(hrnet_tf_supported(HR_TF_LAYERNORM, 0, 0) == 0 && hrnet_tf_supported(HR_TF_LAYERNORM, -3, 0) == 0 &&
             hrnet_tf_supported(HR_TF_LAYERNORM, 65537, 0) == 0 && hrnet_tf_supported(HR_TF_LAYERNORM, big, 0) == 0,
         "supported: layernorm widths outside the limits");
  expect(hrnet_tf_supported(HR_TF_LINEAR, 2, 32) == 1 && hrnet_tf_supported(HR_TF_LINEAR, 672, 42) == 1 &&
             hrnet_tf_supported(HR_TF_LINEAR, 1344, 672) == 1 && hrnet_tf_supported(HR_TF_LINEAR, 672, 2016) == 1,
         "supported: the model's linear shapes");
  expect(hrnet_tf_supported(HR_TF_LINEAR, 0, 32) == 0 && hrnet_tf_supported(HR_TF_LINEAR, 32, 0) == 0 &&
             hrnet_tf_supported(HR_TF_LINEAR, 65537, 32) == 0 && hrnet_tf_supported(HR_TF_LINEAR, 32, -1) == 0,
         "supported: linear shapes outside the limits");
  expect(hrnet_tf_supported(HR_TF_ATTENTION, 21, 4) == 1 && hrnet_tf_supported(HR_TF_ATTENTION, 9, 84) == 1 &&
             hrnet_tf_supported(HR_TF_ATTENTION, 1, 1) == 1 && hrnet_tf_supported(HR_TF_ATTENTION, 64, 128) == 1,
         "supported: attention shapes inside the limits");
  expect(hrnet_tf_supported(HR_TF_ATTENTION, 65, 4) == 0 && hrnet_tf_supported(HR_TF_ATTENTION, 9, 129) == 0 &&
             hrnet_tf_supported(HR_TF_ATTENTION, 0, 4) == 0 && hrnet_tf_supported(HR_TF_ATTENTION, 9, 0) == 0 &&
             hrnet_tf_supported(HR_TF_ATTENTION, -1, -1) == 0,
         "supported: N = 65, hd = 129, zero and negative");
  expect(hrnet_tf_supported(HR_TF_FRAME_MEAN, 9, 0) == 1 && hrnet_tf_supported(HR_TF_FRAME_MEAN, 1, 0) == 1 &&
             hrnet_tf_supported(HR_TF_FRAME_MEAN, 0, 0) == 0 && hrnet_tf_supported(HR_TF_FRAME_MEAN, 65535, 0) == 0,
         "supported: frame counts");
  expect(hrnet_tf_supported(4, 1, 1) == 0 && hrnet_tf_supported(-1, 1, 1) == 0, "supported: an unknown op");

  // layernorm scratch: 2 floats per row and 2 C per 64 rows; 0 outside the limits; formed in 64 bits
  expect(hrnet_tf_layernorm_scratch(1, 32) == 2 + 64 && hrnet_tf_layernorm_scratch(64, 32) == 128 + 64 &&
             hrnet_tf_layernorm_scratch(65, 32) == 130 + 128 && hrnet_tf_layernorm_scratch(756, 32) == 1512 + 12 * 64 &&
             hrnet_tf_layernorm_scratch(36, 672) == 72 + 1344,
         "layernorm scratch at known sizes");
  expect(hrnet_tf_layernorm_scratch(1LL << 22, 65536) == (2LL << 22) + 65536LL * 2 * 65536, "layernorm scratch at the limits");
  expect(hrnet_tf_layernorm_scratch(0, 32) == 0 && hrnet_tf_layernorm_scratch(-1, 32) == 0 &&
             hrnet_tf_layernorm_scratch(1, 0) == 0 && hrnet_tf_layernorm_scratch((1LL << 22) + 1, 32) == 0 &&
             hrnet_tf_layernorm_scratch(huge, big) == 0,
         "layernorm scratch outside the limits");

  float buf[160] = {0};
  float* a = buf;
  float* b = buf + 32;
  float* c = buf + 64;
  float* d = buf + 96;
  float* e = buf + 128;

  refused(hrnet_tf_layernorm(a, b, c, d, 0, 32, 1e-6f, nullptr), "rows = 0", "layernorm rows = 0");
  refused(hrnet_tf_layernorm(a, b, c, d, (1LL << 22) + 1, 32, 1e-6f, nullptr), "rows =", "layernorm too many rows");
  refused(hrnet_tf_layernorm(a, b, c, d, 1, 0, 1e-6f, nullptr), "C = 0", "layernorm C = 0");
  refused(hrnet_tf_layernorm(a, b, c, d, 1, 65537, 1e-6f, nullptr), "C = 65537", "layernorm C beyond the limit");
  refused(hrnet_tf_layernorm(a, b, c, d, 1, 32, 0.f, nullptr), "eps", "layernorm eps = 0");
  refused(hrnet_tf_layernorm(a, b, c, d, 1, 32, -1.f, nullptr), "eps", "layernorm eps < 0");
  refused(hrnet_tf_layernorm(nullptr, b, c, d, 1, 32, 1e-6f, nullptr), "null", "layernorm null x");
  refused(hrnet_tf_layernorm(a, nullptr, c, d, 1, 32, 1e-6f, nullptr), "null", "layernorm null gamma");
  refused(hrnet_tf_layernorm(a, b, nullptr, d, 1, 32, 1e-6f, nullptr), "null", "layernorm null beta");
  refused(hrnet_tf_layernorm(a, b, c, nullptr, 1, 32, 1e-6f, nullptr), "null", "layernorm null y");
  refused(hrnet_tf_layernorm(a, b, c, a, 1, 32, 1e-6f, nullptr), "aliases", "layernorm y == x");

  const long long need = hrnet_tf_layernorm_scratch(1, 32);
  refused(hrnet_tf_layernorm_bwd(a, b, c, d, e, e, e, need, -2, 32, 1e-6f, nullptr), "rows = -2", "layernorm_bwd rows < 0");
  refused(hrnet_tf_layernorm_bwd(a, b, c, d, e, e, e, need, 1, -5, 1e-6f, nullptr), "C = -5", "layernorm_bwd C < 0");
  refused(hrnet_tf_layernorm_bwd(a, b, c, d, e, e, e, need, 1, 32, 0.f, nullptr), "eps", "layernorm_bwd eps = 0");
  refused(hrnet_tf_layernorm_bwd(nullptr, b, c, d, e, e, e, need, 1, 32, 1e-6f, nullptr), "null", "layernorm_bwd null x");
  refused(hrnet_tf_layernorm_bwd(a, b, nullptr, d, e, e, e, need, 1, 32, 1e-6f, nullptr), "null", "layernorm_bwd null dy");
  refused(hrnet_tf_layernorm_bwd(a, b, c, nullptr, nullptr, nullptr, e, need, 1, 32, 1e-6f, nullptr), "all null",
          "layernorm_bwd with nothing to compute");
  refused(hrnet_tf_layernorm_bwd(a, nullptr, c, d, nullptr, nullptr, e, need, 1, 32, 1e-6f, nullptr), "gamma is null",
          "layernorm_bwd dx without gamma");
  refused(hrnet_tf_layernorm_bwd(a, b, c, a, nullptr, nullptr, e, need, 1, 32, 1e-6f, nullptr), "aliases",
          "layernorm_bwd dx == x");
  refused(hrnet_tf_layernorm_bwd(a, b, c, c, nullptr, nullptr, e, need, 1, 32, 1e-6f, nullptr), "aliases",
          "layernorm_bwd dx == dy");
  refused(hrnet_tf_layernorm_bwd(a, b, c, d, e, nullptr, nullptr, need, 1, 32, 1e-6f, nullptr), "null scratch",
          "layernorm_bwd dgamma without scratch");
  refused(hrnet_tf_layernorm_bwd(a, b, c, d, nullptr, e, e, need - 1, 1, 32, 1e-6f, nullptr), "scratch of",
          "layernorm_bwd scratch one float short");
  refused(hrnet_tf_layernorm_bwd(a, b, c, d, nullptr, e, e, -1, 1, 32, 1e-6f, nullptr), "scratch of",
          "layernorm_bwd scratch of a negative size");
  refused(hrnet_tf_layernorm_bwd(a, b, c, d, e, e, e, 1LL << 31, 1LL << 22, 65536, 1e-6f, nullptr), "scratch of",
          "layernorm_bwd: 2^31 floats offered where 2^33 + 2^23 are needed (formed in 64 bits)");

  refused(hrnet_tf_linear(a, b, c, nullptr, nullptr, d, nullptr, 0, 4, 4, 0, nullptr), "rows = 0", "linear rows = 0");
  refused(hrnet_tf_linear(a, b, c, nullptr, nullptr, d, nullptr, 1, 0, 4, 0, nullptr), "Cin = 0", "linear Cin = 0");
  refused(hrnet_tf_linear(a, b, c, nullptr, nullptr, d, nullptr, 1, 4, 65537, 0, nullptr), "Cout = 65537",
          "linear Cout beyond the limit");
  refused(hrnet_tf_linear(a, b, c, nullptr, nullptr, d, nullptr, 1, 4, 4, 2, nullptr), "act = 2", "linear unknown act");
  refused(hrnet_tf_linear(a, b, c, nullptr, nullptr, d, nullptr, 1, 4, 4, -1, nullptr), "act = -1", "linear act < 0");
  refused(hrnet_tf_linear(a, b, c, nullptr, nullptr, d, nullptr, 1LL << 22, 65536, 65536, 0, nullptr), "for the grid",
          "linear: more row blocks than the grid takes");
  refused(hrnet_tf_linear(nullptr, b, c, nullptr, nullptr, d, nullptr, 1, 4, 4, 0, nullptr), "null", "linear null x");
  refused(hrnet_tf_linear(a, nullptr, c, nullptr, nullptr, d, nullptr, 1, 4, 4, 0, nullptr), "null", "linear null W");
  refused(hrnet_tf_linear(a, b, c, nullptr, nullptr, nullptr, nullptr, 1, 4, 4, 0, nullptr), "null", "linear null y");
  refused(hrnet_tf_linear(a, b, c, nullptr, nullptr, a, nullptr, 1, 4, 4, 0, nullptr), "aliases", "linear y == x");
  refused(hrnet_tf_linear(a, b, c, nullptr, nullptr, b, nullptr, 1, 4, 4, 0, nullptr), "aliases", "linear y == W");
  refused(hrnet_tf_linear(a, b, c, nullptr, nullptr, d, e, 1, 4, 4, 0, nullptr), "without an activation",
          "linear pre without GELU");
  refused(hrnet_tf_linear(a, b, c, nullptr, nullptr, d, d, 1, 4, 4, 1, nullptr), "pre aliases", "linear pre == y");
  refused(hrnet_tf_linear(a, b, c, nullptr, nullptr, d, a, 1, 4, 4, 1, nullptr), "pre aliases", "linear pre == x");

  refused(hrnet_tf_linear_bwd(a, b, c, nullptr, nullptr, d, e, e, -1, 4, 4, 0, nullptr), "rows = -1", "linear_bwd rows < 0");
  refused(hrnet_tf_linear_bwd(a, b, c, nullptr, nullptr, d, e, e, 1, 4, 0, 0, nullptr), "Cout = 0", "linear_bwd Cout = 0");
  refused(hrnet_tf_linear_bwd(a, b, c, nullptr, nullptr, d, e, e, 1, 4, 4, 7, nullptr), "act = 7", "linear_bwd unknown act");
  refused(hrnet_tf_linear_bwd(a, b, nullptr, nullptr, nullptr, d, e, e, 1, 4, 4, 0, nullptr), "dy is null",
          "linear_bwd null dy");
  refused(hrnet_tf_linear_bwd(a, b, c, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 4, 4, 0, nullptr), "all null",
          "linear_bwd with nothing to compute");
  refused(hrnet_tf_linear_bwd(a, b, c, nullptr, nullptr, d, e, e, 1, 4, 4, 1, nullptr), "pre", "linear_bwd GELU without pre");
  refused(hrnet_tf_linear_bwd(a, nullptr, c, nullptr, nullptr, d, nullptr, nullptr, 1, 4, 4, 0, nullptr), "W is null",
          "linear_bwd dx without W");
  refused(hrnet_tf_linear_bwd(nullptr, b, c, nullptr, nullptr, nullptr, e, nullptr, 1, 4, 4, 0, nullptr), "x is null",
          "linear_bwd dW without x");
  refused(hrnet_tf_linear_bwd(a, b, c, nullptr, nullptr, c, nullptr, nullptr, 1, 4, 4, 0, nullptr), "dx aliases",
          "linear_bwd dx == dy");
  refused(hrnet_tf_linear_bwd(a, b, c, nullptr, nullptr, a, nullptr, nullptr, 1, 4, 4, 0, nullptr), "dx aliases",
          "linear_bwd dx == x");
  refused(hrnet_tf_linear_bwd(a, b, c, nullptr, nullptr, nullptr, b, nullptr, 1, 4, 4, 0, nullptr), "dW aliases",
          "linear_bwd dW == W");
  refused(hrnet_tf_linear_bwd(a, b, c, nullptr, nullptr, nullptr, c, nullptr, 1, 4, 4, 0, nullptr), "dW aliases",
          "linear_bwd dW == dy");

  refused(hrnet_tf_attention(a, b, 1, 65, 2, 4, 1.f, nullptr), "N = 65", "attention N = 65");
  refused(hrnet_tf_attention(a, b, 1, 9, 2, 129, 1.f, nullptr), "hd = 129", "attention hd = 129");
  refused(hrnet_tf_attention(a, b, 1, 0, 2, 4, 1.f, nullptr), "N = 0", "attention N = 0");
  refused(hrnet_tf_attention(a, b, 0, 4, 2, 4, 1.f, nullptr), "S = 0", "attention S = 0");
  refused(hrnet_tf_attention(a, b, 1, 4, 0, 4, 1.f, nullptr), "heads = 0", "attention heads = 0");
  refused(hrnet_tf_attention(a, b, big, 4, big, 4, 1.f, nullptr), "too many", "attention S * heads beyond the grid");
  refused(hrnet_tf_attention(a, b, 1, 4, 1024, 128, 1.f, nullptr), "too many", "attention heads * hd beyond a row");
  refused(hrnet_tf_attention(nullptr, b, 1, 4, 2, 4, 1.f, nullptr), "null", "attention null qkv");
  refused(hrnet_tf_attention(a, nullptr, 1, 4, 2, 4, 1.f, nullptr), "null", "attention null out");
  refused(hrnet_tf_attention(a, a, 1, 4, 2, 4, 1.f, nullptr), "aliases", "attention out == qkv");
  refused(hrnet_tf_attention_bwd(a, b, c, 1, 65, 2, 4, 1.f, nullptr), "N = 65", "attention_bwd N = 65");
  refused(hrnet_tf_attention_bwd(a, b, c, 1, 4, 2, -4, 1.f, nullptr), "hd = -4", "attention_bwd hd < 0");
  refused(hrnet_tf_attention_bwd(a, b, c, -1, 4, 2, 4, 1.f, nullptr), "S = -1", "attention_bwd S < 0");
  refused(hrnet_tf_attention_bwd(nullptr, b, c, 1, 4, 2, 4, 1.f, nullptr), "null", "attention_bwd null qkv");
  refused(hrnet_tf_attention_bwd(a, nullptr, c, 1, 4, 2, 4, 1.f, nullptr), "null", "attention_bwd null dout");
  refused(hrnet_tf_attention_bwd(a, b, nullptr, 1, 4, 2, 4, 1.f, nullptr), "null", "attention_bwd null dqkv");
  refused(hrnet_tf_attention_bwd(a, b, a, 1, 4, 2, 4, 1.f, nullptr), "aliases", "attention_bwd dqkv == qkv");
  refused(hrnet_tf_attention_bwd(a, b, b, 1, 4, 2, 4, 1.f, nullptr), "aliases", "attention_bwd dqkv == dout");

  refused(hrnet_tf_frame_mean(a, b, c, d, 1, 0, 4, nullptr), "F = 0", "frame_mean F = 0");
  refused(hrnet_tf_frame_mean(a, b, c, d, 1, 65535, 4, nullptr), "F = 65535", "frame_mean F beyond the grid");
  refused(hrnet_tf_frame_mean(a, b, c, d, 1, 4, 0, nullptr), "D = 0", "frame_mean D = 0");
  refused(hrnet_tf_frame_mean(a, b, c, d, 1, 4, (1LL << 24) + 1, nullptr), "D =", "frame_mean D beyond the limit");
  refused(hrnet_tf_frame_mean(a, b, c, d, 0, 4, 4, nullptr), "S = 0", "frame_mean S = 0");
  refused(hrnet_tf_frame_mean(a, b, c, d, 1LL << 22, 65534, 1 << 24, nullptr), "2^31", "frame_mean: more than 2^31 elements");
  refused(hrnet_tf_frame_mean(nullptr, b, c, d, 1, 4, 4, nullptr), "null", "frame_mean null x");
  refused(hrnet_tf_frame_mean(a, nullptr, c, d, 1, 4, 4, nullptr), "null", "frame_mean null w");
  refused(hrnet_tf_frame_mean(a, b, c, nullptr, 1, 4, 4, nullptr), "null", "frame_mean null y");
  refused(hrnet_tf_frame_mean(a, b, c, a, 1, 4, 4, nullptr), "aliases", "frame_mean y == x");
  refused(hrnet_tf_frame_mean_bwd(a, b, c, d, e, e, 1, -1, 4, nullptr), "F = -1", "frame_mean_bwd F < 0");
  refused(hrnet_tf_frame_mean_bwd(a, b, c, d, e, e, huge, 4, 4, nullptr), "S =", "frame_mean_bwd S beyond the limit");
  refused(hrnet_tf_frame_mean_bwd(a, b, nullptr, d, e, e, 1, 4, 4, nullptr), "dy is null", "frame_mean_bwd null dy");
  refused(hrnet_tf_frame_mean_bwd(a, b, c, nullptr, nullptr, nullptr, 1, 4, 4, nullptr), "all null",
          "frame_mean_bwd with nothing to compute");
  refused(hrnet_tf_frame_mean_bwd(a, nullptr, c, d, nullptr, nullptr, 1, 4, 4, nullptr), "w is null",
          "frame_mean_bwd dx without w");
  refused(hrnet_tf_frame_mean_bwd(nullptr, b, c, nullptr, e, nullptr, 1, 4, 4, nullptr), "x is null",
          "frame_mean_bwd dw without x");
  refused(hrnet_tf_frame_mean_bwd(a, b, c, c, nullptr, nullptr, 1, 4, 4, nullptr), "aliases", "frame_mean_bwd dx == dy");
  refused(hrnet_tf_frame_mean_bwd(a, b, c, a, nullptr, nullptr, 1, 4, 4, nullptr), "aliases", "frame_mean_bwd dx == x");

  refused(hrnet_tf_add_rows(a, b, c, 0, 4, 1, nullptr), "rows = 0", "add_rows rows = 0");
  refused(hrnet_tf_add_rows(a, b, c, 4, 0, 1, nullptr), "C = 0", "add_rows C = 0");
  refused(hrnet_tf_add_rows(a, b, c, 4, 4, 0, nullptr), "period = 0", "add_rows period = 0");
  refused(hrnet_tf_add_rows(a, b, c, 4, 4, 3, nullptr), "does not divide", "add_rows period not dividing rows");
  refused(hrnet_tf_add_rows(a, b, c, 4, 4, -2, nullptr), "period = -2", "add_rows period < 0");
  refused(hrnet_tf_add_rows(nullptr, b, c, 4, 4, 2, nullptr), "null", "add_rows null x");
  refused(hrnet_tf_add_rows(a, nullptr, c, 4, 4, 2, nullptr), "null", "add_rows null pos");
  refused(hrnet_tf_add_rows(a, b, nullptr, 4, 4, 2, nullptr), "null", "add_rows null y");

  expect(g_launch_checks == 0, "an argument check let a call through to a launch");
  printf(failures ? "transformer host check: %d FAILED\n" : "transformer host check: all answered as expected (%d)\n",
         failures);
  return failures ? 1 : 0;
}
