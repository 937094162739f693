// K x K convolution (odd ks <= 11, stride 1, padding ks/2) as an implicit GEMM on the f32 MFMA, and the two pools of the
// Convolutional Pose Machine (lib/models/CPM.py): MaxPool2d(3, 2, 1) and the centre map's AvgPool2d(9, 8, 1).
//
// hrnet_conv2d serves ks 1 and 3 only: its tile body keeps a (tile + 2)-wide halo. CPM is 5x5, 9x9 and 11x11 layers, so
// here the halo is a run-time size: a workgroup owns an 8 x 16 pixel tile and a block of output channels, stages the
// (8 + ks - 1) x (16 + ks - 1) input window of 16 input channels in LDS ONCE and all ks*ks taps read it from there
// (no im2col in global memory). Weights are the packed [Cout_pad][ks*ks][Cin] of hrnet_pack_weights mode 0, read by
// each lane as 16 bytes straight from global memory (L1/L2: the same 16 x 64 bytes serve every pixel tile of a
// workgroup) a few taps ahead of the MFMAs that use them.
//
// Both sides carry a row length and a channel offset (x [N,H,W,ldx] from x_off, y [N,H,W,ldy] from y_off): a layer reads
// and writes a channel slice of a wider map, so CPM's torch.cat([features, heat maps, centre map]) is never a copy.
// Only the real Cout channels are stored (masked), nothing outside [y_off, y_off + Cout) is touched.
//
// Summation order of one output (fixed: no atomics, no split K, the same for every launch geometry, so two runs and
// two batch sizes give equal bits):
//   acc = 0; for c0 = 0, 16, ... < Cin; for r = 0 .. ks-1:
//       part = 0; for s = 0 .. ks-1; for j = 0 .. 3:
//           part = mfma_16x16x4(w[co][r ks + s][c0 + 4 g + j], x[pixel + (r, s)][c0 + 4 g + j], g = 0 .. 3, part)
//       acc += part
//   y = acc + bias; ReLU.
// (one partial sum per kernel row and channel pass: 16 ks terms each, so the rounding error of an 11 x 11 x 128 layer
// grows like that of ~180-term sums, not of one 15 488-term chain)
// Cin == 4 (the image layers, 3 channels + one zero) would waste 3/4 of every MFMA's K that way; there the four K
// slots of an MFMA are four neighbouring taps of one kernel row instead:
//   acc = 0; for r = 0 .. ks-1; for s0 = 0, 4, ... < ks; for j = 0 .. 3:
//       acc = mfma_16x16x4(w[co][r*ks + s0 + g][j], x[pixel + (r, s0 + g)][j], g = 0 .. 3 (s0 + g < ks), acc)
// The tile body lives in conv_kxk_body.h: the data gradient of csrc/conv_kxk_train.hip runs on it too.
#include "conv_kxk_body.h"

namespace {

// MaxPool2d(3, 2, 1): one thread per (output pixel, channel); a window never lies wholly in the padding, and padding
// never wins (it is skipped, not read as zero)
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H,
                                                           int W, int C, int ldx, int x_off, int ldy, int y_off, int Ho,
                                                           int Wo) {
  const long long total = (long long)N * Ho * Wo * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % C);
    long long p = i / C;
    const int wo = (int)(p % Wo);
    p /= Wo;
    const int ho = (int)(p % Ho), n = (int)(p / Ho);
    float m = -INFINITY;
    for (int dh = -1; dh <= 1; ++dh) {
      const int h = 2 * ho + dh;
      if (h < 0 || h >= H) continue;
      for (int dw = -1; dw <= 1; ++dw) {
        const int w = 2 * wo + dw;
        if (w < 0 || w >= W) continue;
        const float v = x[(((size_t)n * H + h) * W + w) * ldx + x_off + c];
        m = (v > m || v != v) ? v : m;   // a NaN propagates, as in torch
      }
    }
    y[(((size_t)n * Ho + ho) * Wo + wo) * ldy + y_off + c] = m;
  }
}

// AvgPool2d(9, 8, 1), count_include_pad: the 81 window values (zeros in the padding) summed row by row, divided by 81
__global__ __launch_bounds__(256) void avgpool9s8_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H,
                                                         int W, int ldy, int y_off, int Ho, int Wo) {
  const long long total = (long long)N * Ho * Wo;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int wo = (int)(i % Wo);
    const int ho = (int)((i / Wo) % Ho), n = (int)(i / ((long long)Wo * Ho));
    float sum = 0.f;
    for (int dh = 0; dh < 9; ++dh) {
      const int h = 8 * ho - 1 + dh;
      if (h < 0 || h >= H) continue;
      for (int dw = 0; dw < 9; ++dw) {
        const int w = 8 * wo - 1 + dw;
        if (w < 0 || w >= W) continue;
        sum += x[((size_t)n * H + h) * W + w];
      }
    }
    y[(((size_t)n * Ho + ho) * Wo + wo) * ldy + y_off] = sum / 81.f;
  }
}

unsigned kx_ew_grid(long long total) {
  const long long b = (total + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

}  // namespace

extern "C" hr_value_t hrnet_conv_kxk_tile(int which) {
  switch (which) {
    case 0: return KX_TH;
    case 1: return KX_TW;
    case 2: return KX_KC;
    case 3: return KX_MAXKS;
    default: return 0;
  }
}

extern "C" int hrnet_conv2d_kxk(int dtype, const void* x, const void* w, const float* bias, void* y, int N, int H, int W,
                                int Cin, int ldx, int x_off, int Cout, int ldy, int y_off, int ks, int relu,
                                hr_stream_t stream) {
  HR_REQUIRE(dtype == HR_F32, "conv2d_kxk: dtype = %d: only f32 (HR_F32 = 0) is built", dtype);
  HR_REQUIRE(x && w && y, "conv2d_kxk: null argument");
  HR_REQUIRE(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "conv2d_kxk: N = %d, H = %d, W = %d, Cin = %d, Cout = %d",
             N, H, W, Cin, Cout);
  HR_REQUIRE(ks >= 1 && ks <= KX_MAXKS && (ks & 1), "conv2d_kxk: ks = %d (odd, 1 .. %d)", ks, KX_MAXKS);
  HR_REQUIRE(Cin % 4 == 0 && ldx % 4 == 0 && x_off % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0,
             "conv2d_kxk: Cin = %d, ldx = %d, x_off = %d: multiples of 4, x and w 16-byte aligned", Cin, ldx, x_off);
  HR_REQUIRE(x_off >= 0 && (long long)x_off + Cin <= ldx, "conv2d_kxk: channels [%d, %d + %d) outside ldx = %d", x_off,
             x_off, Cin, ldx);
  HR_REQUIRE(y_off >= 0 && (long long)y_off + Cout <= ldy, "conv2d_kxk: channels [%d, %d + %d) outside ldy = %d", y_off,
             y_off, Cout, ldy);
  HR_REQUIRE(((uintptr_t)y & 3) == 0 && (relu == 0 || relu == 1), "conv2d_kxk: y alignment / relu = %d", relu);
  KxkArgs a;
  a.x = (const float*)x; a.w = (const float*)w; a.bias = bias; a.y = (float*)y;
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ldx = ldx; a.x_off = x_off; a.Cout = Cout;
  a.ldy = ldy; a.y_off = y_off; a.ks = ks; a.relu = relu;
  a.vec_store = ldy % 4 == 0 && y_off % 4 == 0 && ((uintptr_t)y & 15) == 0;
  a.mask = nullptr; a.ldm = 0; a.m_off = 0; a.accumulate = 0;
  return kx_dispatch<false>(a, "conv2d_kxk", (hipStream_t)stream);   // the launch geometry: conv_kxk_body.h
}

extern "C" int hrnet_maxpool2d_3x3s2(const float* x, float* y, int N, int H, int W, int C, int ldx, int x_off, int ldy,
                                     int y_off, hr_stream_t stream) {
  HR_REQUIRE(x && y, "maxpool2d_3x3s2: null argument");
  HR_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 1, "maxpool2d_3x3s2: N = %d, H = %d, W = %d, C = %d", N, H, W, C);
  HR_REQUIRE(x_off >= 0 && (long long)x_off + C <= ldx && y_off >= 0 && (long long)y_off + C <= ldy,
             "maxpool2d_3x3s2: channels [%d, +%d) in ldx = %d, [%d, +%d) in ldy = %d", x_off, C, ldx, y_off, C, ldy);
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(kx_ew_grid((long long)N * Ho * Wo * C)), dim3(256), 0, (hipStream_t)stream, x,
                     y, N, H, W, C, ldx, x_off, ldy, y_off, Ho, Wo);
  return hr_check_launch("maxpool2d_3x3s2");
}

extern "C" int hrnet_avgpool2d_9s8(const float* x, float* y, int N, int H, int W, int ldy, int y_off, hr_stream_t stream) {
  HR_REQUIRE(x && y, "avgpool2d_9s8: null argument");
  HR_REQUIRE(N >= 1 && H >= 7 && W >= 7, "avgpool2d_9s8: N = %d, H = %d, W = %d (a 9-wide window with padding 1 needs 7)", N,
             H, W);
  HR_REQUIRE(y_off >= 0 && y_off < ldy, "avgpool2d_9s8: channel %d outside ldy = %d", y_off, ldy);
  const int Ho = (H - 7) / 8 + 1, Wo = (W - 7) / 8 + 1;
  hipLaunchKernelGGL(avgpool9s8_kernel, dim3(kx_ew_grid((long long)N * Ho * Wo)), dim3(256), 0, (hipStream_t)stream, x, y, N,
                     H, W, ldy, y_off, Ho, Wo);
  return hr_check_launch("avgpool2d_9s8");
}
