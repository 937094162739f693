// The tile body of the K x K implicit-GEMM convolution, shared by the forward (csrc/conv_kxk.hip, hrnet_conv2d_kxk) and
// the data gradient (csrc/conv_kxk_train.hip, hrnet_conv2d_kxk_dgrad: the same convolution of dy with the flipped,
// transposed weight). The two differ in the epilogue alone (template parameter DG); the loads, the MFMA order and so
// the summation order stated at the top of conv_kxk.hip are one piece of code.
#pragma once
#include "common.h"

namespace {

constexpr int KX_TH = 8, KX_TW = 16, KX_KC = 16, KX_MAXKS = 11;

struct KxkArgs {
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  int N, H, W, Cin, ldx, x_off, Cout, Cout_pad, ldy, y_off, ks, relu, tiles_h, tiles_w, vec_store;
  // data gradient only (DG): y = (mask > 0 ? acc : 0) (+ y if accumulate); mask [N,H,W,ldm] read at m_off
  const float* mask;
  int ldm, m_off, accumulate;
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
template <int MT, int NT, int WM, int WN, int PF, bool CIN4, bool DG>
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
      if constexpr (DG) {
        // the ReLU of the layer that produced this input (its saved output is the mask), then the other consumers' sum
        const float* mp = a.mask ? a.mask + (((size_t)n * a.H + h) * a.W + w) * a.ldm + a.m_off : nullptr;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (co + k >= a.Cout) continue;
          if (mp && !(mp[co + k] > 0.f)) o[k] = 0.f;
          if (a.accumulate) o[k] += yp[co + k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (a.bias && co + k < a.Cout) o[k] += a.bias[co + k];
          if (a.relu) o[k] = fmaxf(o[k], 0.f);
        }
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

template <int MT, int NT, int WM, int WN, int PF, bool DG>
void kx_launch(const KxkArgs& a, hipStream_t s) {
  const int HH = KX_TH + a.ks - 1, WH = KX_TW + a.ks - 1;
  const int cb = 16 * MT * WM;
  const dim3 grid((unsigned)(a.N * a.tiles_h * a.tiles_w), (unsigned)((a.Cout_pad + cb - 1) / cb));
  if (a.Cin == 4)
    hipLaunchKernelGGL((conv_kxk_kernel<MT, NT, WM, WN, PF, true, DG>), grid, dim3(256), (size_t)HH * WH * 16, s, a);
  else
    hipLaunchKernelGGL((conv_kxk_kernel<MT, NT, WM, WN, PF, false, DG>), grid, dim3(256), (size_t)HH * WH * 64, s, a);
}

// 64 output channels per workgroup (8 MFMA tiles per wave and weight load) where that still gives every CU two
// workgroups, 32 where that fills the device once, 16 below that (the 32 x 32 maps of one image); the sums do not
// depend on the choice. a.tiles_h / a.tiles_w / a.Cout_pad are filled in here.
template <bool DG>
int kx_dispatch(KxkArgs& a, const char* who, hipStream_t s) {
  a.tiles_h = (int)(((long long)a.H + KX_TH - 1) / KX_TH);
  a.tiles_w = (int)(((long long)a.W + KX_TW - 1) / KX_TW);
  const long long nth = (long long)a.N * a.tiles_h;   // < 2^59; times tiles_w only once it is known to be small
  const long long ptiles = nth <= 0x7fffffffLL ? nth * a.tiles_w : nth;
  HR_REQUIRE(ptiles <= 0x7fffffffLL, "%s: %lld pixel tiles", who, ptiles);
  HR_REQUIRE(a.Cout <= 0x7fffffff - 15, "%s: Cout = %d", who, a.Cout);
  a.Cout_pad = (a.Cout + 15) / 16 * 16;
  if (a.Cout_pad % 64 == 0 && ptiles * (a.Cout_pad / 64) >= 512)
    kx_launch<1, 8, 4, 1, 2, DG>(a, s);
  else if (ptiles * ((a.Cout_pad + 31) / 32) >= 256)
    kx_launch<1, 4, 2, 2, 4, DG>(a, s);
  else
    kx_launch<1, 2, 1, 4, 8, DG>(a, s);
  return hr_check_launch(who);
}

}  // namespace
