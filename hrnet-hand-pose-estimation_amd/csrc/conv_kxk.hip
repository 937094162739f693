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
#include "common.h"

namespace {

constexpr int KX_TH = 8, KX_TW = 16, KX_KC = 16, KX_MAXKS = 11;

struct KxkArgs {
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  int N, H, W, Cin, ldx, x_off, Cout, Cout_pad, ldy, y_off, ks, relu, tiles_h, tiles_w, vec_store;
};

// LDS slot of channel group g (4 floats) of halo pixel p: a bijection in g for every p that spreads the 16-lane groups
// of ds_read_b128 over the 256-byte bank row
__device__ __forceinline__ int kx_slot(int p, int g) {
  return p * 4 + ((((0x9c >> (2 * g)) & 3) ^ (p >> 2)) & 3);   // g -> {0, 3, 1, 2}[g] ^ (p / 4)
}

// acc[m][q] += A[m] (16 output channels x 16 k) * B[q] (16 k x 16 pixels) as four 16x16x4 MFMAs per tile, issued k
// slice by k slice over ALL tiles: neighbouring MFMAs are independent (a 16x16x4 result is ready after 40 cycles, the
// next one issues after 32), and every accumulator still sees its k slices in the order 0, 1, 2, 3
template <int MT, int NT>
__device__ __forceinline__ void kx_mma(const V16 (&av)[MT], const V16 (&bv)[NT], f32x4 (&acc)[MT][NT]) {
  f32x4 af[MT], bf[NT];
#pragma unroll
  for (int m = 0; m < MT; ++m) af[m] = __builtin_bit_cast(f32x4, av[m]);
#pragma unroll
  for (int q = 0; q < NT; ++q) bf[q] = __builtin_bit_cast(f32x4, bv[q]);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int q = 0; q < NT; ++q) acc[m][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[m][j], bf[q][j], acc[m][q], 0, 0, 0);
}

// MT x NT MFMA tiles (16 output channels x one row of 16 pixels) per wave, WM x WN waves: a workgroup covers
// 16 MT WM output channels and NT WN = KX_TH pixel rows. PF: how many taps ahead of the MFMAs a lane requests its
// weights (a ring of PF register sets): the fewer MFMAs a tap has, the deeper the ring that covers an L2 round trip
template <int MT, int NT, int WM, int WN, int PF, bool CIN4>
__global__ __launch_bounds__(256) void conv_kxk_kernel(const KxkArgs a) {
  static_assert(WM * WN == 4 && NT * WN == KX_TH, "tile");
  extern __shared__ V16 kx_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int wm = wave / WN, wn = wave % WN;
  int t = blockIdx.x;
  const int tw = t % a.tiles_w;
  t /= a.tiles_w;
  const int th = t % a.tiles_h, n = t / a.tiles_h;
  const int ks = a.ks, pad = ks >> 1, taps = ks * ks;
  const int h0 = th * KX_TH, w0 = tw * KX_TW;
  const int HH = KX_TH + ks - 1, WH = KX_TW + ks - 1;
  const int co_base = ((int)blockIdx.y * WM + wm) * MT * 16;
  const int row_base = wn * NT;
  const int Cin = a.Cin;
  const size_t wrow = (size_t)taps * Cin;
  const float* xn = a.x + (size_t)n * a.H * a.W * a.ldx + a.x_off;

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[m][q] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this lane's weight rows (one per M tile); rows past the packed weights are never dereferenced
  const float* wl[MT];
  bool wok[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int co = co_base + m * 16 + li;
    wok[m] = co < a.Cout_pad;
    wl[m] = a.w + (size_t)(wok[m] ? co : 0) * wrow;
  }

  if constexpr (CIN4) {
    // the whole input window, 4 channels = one 16-byte vector per pixel
    for (int p = tid; p < HH * WH; p += 256) {
      const int hr = p / WH, wc = p - hr * WH;
      const int h = h0 + hr - pad, w = w0 + wc - pad;
      V16 v = v16_zero();
      if (h >= 0 && h < a.H && w >= 0 && w < a.W) v = *(const V16*)(xn + ((size_t)h * a.W + w) * a.ldx);
      kx_lds[p] = v;
    }
    __syncthreads();
    const int sgroups = (ks + 3) >> 2;
    // the weights of the next four taps are requested while the MFMAs of these four run
    V16 an[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) an[m] = lg < ks && wok[m] ? *(const V16*)(wl[m] + (size_t)lg * 4) : v16_zero();
    for (int r = 0; r < ks; ++r) {
      for (int sg = 0; sg < sgroups; ++sg) {
        const int s = sg * 4 + lg;
        V16 av[MT], bv[NT];
        const bool last = sg + 1 == sgroups;
        const int rn = last ? r + 1 : r, sn = last ? lg : s + 4;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          av[m] = an[m];
          an[m] = rn < ks && sn < ks && wok[m] ? *(const V16*)(wl[m] + (size_t)(rn * ks + sn) * 4) : v16_zero();
        }
        const int sb = s < ks ? s : 0;   // a tap past the kernel row multiplies a zero weight: read a pixel that exists
#pragma unroll
        for (int q = 0; q < NT; ++q) bv[q] = kx_lds[(row_base + q + r) * WH + li + sb];
        kx_mma<MT, NT>(av, bv, acc);
      }
    }
  } else {
    for (int c0 = 0; c0 < Cin; c0 += KX_KC) {
      __syncthreads();   // the taps of the previous chunk have read the window
      for (int v = tid; v < HH * WH * 4; v += 256) {
        const int p = v >> 2, g = v & 3;
        const int hr = p / WH, wc = p - hr * WH;
        const int h = h0 + hr - pad, w = w0 + wc - pad, c = c0 + g * 4;
        V16 val = v16_zero();
        if (h >= 0 && h < a.H && w >= 0 && w < a.W && c < Cin) val = *(const V16*)(xn + ((size_t)h * a.W + w) * a.ldx + c);
        kx_lds[kx_slot(p, g)] = val;
      }
      __syncthreads();
      const int c = c0 + lg * 4;
      const bool cok = c < Cin;   // a chunk past Cin: zero weights against the zero vectors staged above
      V16 ring[PF][MT];   // the weights of taps tap .. tap + PF - 1, set u holding the taps = u (mod PF)
#pragma unroll
      for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int m = 0; m < MT; ++m)
          ring[u][m] = cok && wok[m] && u < taps ? *(const V16*)(wl[m] + (size_t)u * Cin + c) : v16_zero();
      int r = 0, s = 0;
      f32x4 part[MT][NT];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < NT; ++q) part[m][q] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int tap0 = 0; tap0 < taps; tap0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
          const int tap = tap0 + u;
          if (tap >= taps) break;
          V16 av[MT], bv[NT];
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            av[m] = ring[u][m];
            ring[u][m] = cok && wok[m] && tap + PF < taps ? *(const V16*)(wl[m] + (size_t)(tap + PF) * Cin + c) : v16_zero();
          }
#pragma unroll
          for (int q = 0; q < NT; ++q) bv[q] = kx_lds[kx_slot((row_base + q + r) * WH + li + s, lg)];
          kx_mma<MT, NT>(av, bv, part);
          if (++s == ks) {   // a kernel row is done: its partial sum joins the total
            s = 0;
            ++r;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
              for (int q = 0; q < NT; ++q) {
                acc[m][q] += part[m][q];
                part[m][q] = f32x4{0.f, 0.f, 0.f, 0.f};
              }
          }
        }
      }
    }
  }

  // D of the 16x16 MFMA: column (pixel) = lane & 15, row (output channel) = 4 (lane >> 4) + register
  float* yn = a.y + (size_t)n * a.H * a.W * a.ldy + a.y_off;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int h = h0 + row_base + q, w = w0 + li;
    if (h >= a.H || w >= a.W) continue;
    float* yp = yn + ((size_t)h * a.W + w) * a.ldy;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int co = co_base + m * 16 + lg * 4;
      if (co >= a.Cout) continue;
      float o[4] = {acc[m][q].x, acc[m][q].y, acc[m][q].z, acc[m][q].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (a.bias && co + k < a.Cout) o[k] += a.bias[co + k];
        if (a.relu) o[k] = fmaxf(o[k], 0.f);
      }
      if (a.vec_store && co + 3 < a.Cout) {
        *(f32x4*)(yp + co) = f32x4{o[0], o[1], o[2], o[3]};
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (co + k < a.Cout) yp[co + k] = o[k];
      }
    }
  }
}

template <int MT, int NT, int WM, int WN, int PF>
void kx_launch(const KxkArgs& a, hipStream_t s) {
  const int HH = KX_TH + a.ks - 1, WH = KX_TW + a.ks - 1;
  const int cb = 16 * MT * WM;
  const dim3 grid((unsigned)(a.N * a.tiles_h * a.tiles_w), (unsigned)((a.Cout_pad + cb - 1) / cb));
  if (a.Cin == 4)
    hipLaunchKernelGGL((conv_kxk_kernel<MT, NT, WM, WN, PF, true>), grid, dim3(256), (size_t)HH * WH * 16, s, a);
  else
    hipLaunchKernelGGL((conv_kxk_kernel<MT, NT, WM, WN, PF, false>), grid, dim3(256), (size_t)HH * WH * 64, s, a);
}

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
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ldx = ldx; a.x_off = x_off; a.Cout = Cout; a.Cout_pad = (Cout + 15) / 16 * 16;
  a.ldy = ldy; a.y_off = y_off; a.ks = ks; a.relu = relu;
  a.tiles_h = (H + KX_TH - 1) / KX_TH;
  a.tiles_w = (W + KX_TW - 1) / KX_TW;
  a.vec_store = ldy % 4 == 0 && y_off % 4 == 0 && ((uintptr_t)y & 15) == 0;
  const long long ptiles = (long long)N * a.tiles_h * a.tiles_w;
  HR_REQUIRE(ptiles <= 0x7fffffffLL, "conv2d_kxk: %lld pixel tiles", ptiles);
  // 64 output channels per workgroup (8 MFMA tiles per wave and weight load) where that still gives every CU two
  // workgroups, 32 where that fills the device once, 16 below that (the 32 x 32 maps of one image); the sums do not
  // depend on the choice
  if (a.Cout_pad % 64 == 0 && ptiles * (a.Cout_pad / 64) >= 512)
    kx_launch<1, 8, 4, 1, 2>(a, (hipStream_t)stream);
  else if (ptiles * ((a.Cout_pad + 31) / 32) >= 256)
    kx_launch<1, 4, 2, 2, 4>(a, (hipStream_t)stream);
  else
    kx_launch<1, 2, 1, 4, 8>(a, (hipStream_t)stream);
  return hr_check_launch("conv2d_kxk");
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
